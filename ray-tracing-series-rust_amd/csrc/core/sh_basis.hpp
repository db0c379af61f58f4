// The real orthonormal spherical-harmonic basis of orders 0..2, the one statement of it that k_reduce_samples_sh (hip/gather.inc),
// the host checker (tests/gather_host_check.cpp) and every caller who wants the same bits share.
//
// Order of the functions: (l, m) = (0,0), (1,-1), (1,0), (1,1), (2,-2), (2,-1), (2,0), (2,1), (2,2) -- index l (l + 1) + m.
// With (x, y, z) a unit direction:
//   Y00 = 1/2 sqrt(1/pi)
//   Y1-1 = sqrt(3/(4 pi)) y            Y10 = sqrt(3/(4 pi)) z              Y11 = sqrt(3/(4 pi)) x
//   Y2-2 = 1/2 sqrt(15/pi) x y         Y2-1 = 1/2 sqrt(15/pi) y z          Y20 = 1/4 sqrt(5/pi) (3 z^2 - 1)
//   Y21  = 1/2 sqrt(15/pi) x z         Y22  = 1/4 sqrt(15/pi) (x^2 - y^2)
// so that the integral of Y_i Y_j over the sphere is 1 for i = j and 0 otherwise.  The constants are double literals (the
// correctly rounded values), and the order of operations is the one written below, every operation separately rounded in f64
// (-ffp-contract=off on every compilation of the project): the constant times the parenthesised polynomial, products before
// the sum, left to right.  The direction is used as given -- a caller who wants the basis on a unit vector passes one.
// Arithmetic is double in both compilations: an f32 scene widens its float direction first.
// No other header of the project is needed.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RT_SH_HD __host__ __device__ inline
#else
#define RT_SH_HD inline
#endif

#define RT_SH_MAX_ORDER 2
#define RT_SH_MAX_COEFFS 9

// Coefficients of an order: 1, 4, 9.
RT_SH_HD int sh_coeffs(int order) { return (order + 1) * (order + 1); }

// y[0 .. sh_coeffs(order) - 1] = Y_i(x, y, z), order 0..2.
RT_SH_HD void sh_basis_eval(int order, double x, double y, double z, double* out) {
  out[0] = 0.28209479177387814;  // 1/2 sqrt(1/pi)
  if (order < 1) return;
  const double c1 = 0.4886025119029199;  // sqrt(3/(4 pi))
  out[1] = c1 * y;
  out[2] = c1 * z;
  out[3] = c1 * x;
  if (order < 2) return;
  const double c2 = 1.0925484305920792;   // 1/2 sqrt(15/pi)
  const double c20 = 0.31539156525252005; // 1/4 sqrt(5/pi)
  const double c22 = 0.5462742152960396;  // 1/4 sqrt(15/pi)
  out[4] = c2 * (x * y);
  out[5] = c2 * (y * z);
  out[6] = c20 * (3.0 * (z * z) - 1.0);
  out[7] = c2 * (x * z);
  out[8] = c22 * (x * x - y * y);
}
