// The world box of one member of an instance tree, from its local box and its Translate / RotateY ops, and the outward
// narrowing of a box plane to f32.  ONE text for the flattener (host/flatten.cpp, which fills the ops itself: it is the judge of the rest), the host refit and rebuild (host/set_transforms.hpp, host/rebuild_instances.hpp) and the device's
// (hip/scene_update.inc, hip/scene_rebuild.inc): a refitted tree is judged bit for bit against a tree flattened from scratch, so
// all of them must round alike.  Everything here is f64 arithmetic whatever rt::real is -- the f32 compilation refits from the same
// doubles and narrows last, as its converter does (host/f32_layout.hpp).
//
// Bit-exactness between the host and the device build rests on two things the build already pins for the whole core:
// -ffp-contract=off (no fma for cos_t * x + sin_t * z in either build) and min / max / fabs that are exact in both.
#pragma once
#include "flat_types.hpp"

namespace rt {

// FlatXformOp with f64 parameters in either compilation (the layout of FlatXformOp where real = double, and of one element of
// RtxSlotOps::ops in include/rtx_abi.h).  translate: v = offset; rotate_y: v[0] = sin_theta, v[1] = cos_theta.
struct XformOp64 {
  int32_t op;
  int32_t pad;
  double v[3];
};

// local: the ordered union of the member's primitive boxes before any op (lo xyz, hi xyz).  ops: outermost first, so they are
// applied from ops[n_ops - 1] down to ops[0].  RotateY: min / max of the four rotated (x, z) corners with the stored sin / cos --
// the box hit.rs:857-885 computes; Translate: the offset added.  Every plane is then pushed OUTWARD by 2^-22 of the largest
// magnitude met on the way (coordinates before and after every op, offsets): see core/cull32.hpp, "boxes of transformed members".
RT_HD void member_box_through_ops(const double* local, const XformOp64* ops, int n_ops, double* b) {
  const double inf = __builtin_huge_val();
  for (int a = 0; a < 6; ++a) b[a] = local[a];
  double mag = 0.0;
  for (int a = 0; a < 6; ++a) mag = rt_fmax(mag, rt_fabs(b[a]));
  for (int k = n_ops - 1; k >= 0; --k) {
    const XformOp64& op = ops[k];
    if (op.op == XFORM_TRANSLATE) {
      for (int a = 0; a < 3; ++a) { b[a] += op.v[a]; b[3 + a] += op.v[a]; mag = rt_fmax(mag, rt_fabs(op.v[a])); }
    } else {
      const double sin_t = op.v[0], cos_t = op.v[1];
      double lo[3] = {inf, b[1], inf}, hi[3] = {-inf, b[4], -inf};
      for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) {
          const double x = i ? b[3] : b[0], z = j ? b[5] : b[2];
          const double nx = cos_t * x + sin_t * z, nz = -sin_t * x + cos_t * z;
          lo[0] = rt_fmin(lo[0], nx); hi[0] = rt_fmax(hi[0], nx);
          lo[2] = rt_fmin(lo[2], nz); hi[2] = rt_fmax(hi[2], nz);
        }
      for (int a = 0; a < 3; ++a) { b[a] = lo[a]; b[3 + a] = hi[a]; }
    }
    for (int a = 0; a < 6; ++a) mag = rt_fmax(mag, rt_fabs(b[a]));
  }
  const double pad = mag * 0x1.0p-22;
  for (int a = 0; a < 3; ++a) { b[a] -= pad; b[3 + a] += pad; }
}

// The f64 ops of member slot `slot`, whose entry in the world list is S, into ops[RT_MAX_XFORM_OPS]; returns how many (0: the
// member has no chain).  An f64 scene's entries hold them.  An f32 scene's went through a (float) cast, so it reads the f64 copy
// it keeps beside them: slot_ops64, RT_MAX_XFORM_OPS per slot (NULL and never read in the f64 compilation).
RT_HD int member_ops64(const FlatEntry& S, int32_t slot, const XformOp64* slot_ops64, XformOp64* ops) {
  if (S.kind != ENTRY_XFORM) return 0;
  const int n_ops = S.b < RT_MAX_XFORM_OPS ? S.b : RT_MAX_XFORM_OPS;
  for (int k = 0; k < n_ops; ++k) {
#ifdef RT_F32
    ops[k] = slot_ops64[(size_t)slot * RT_MAX_XFORM_OPS + k];
#else
    ops[k].op = S.ops[k].op; ops[k].pad = 0;
    for (int x = 0; x < 3; ++x) ops[k].v[x] = S.ops[k].v[x];
#endif
  }
  return n_ops;
}

// The world box of that member NOW: its local box through the ops it has at this moment.  What every refit and rebuild, on the
// host and on the device, starts from.
RT_HD void member_world_box(const FlatEntry& S, int32_t slot, const XformOp64* slot_ops64, const double* local, double* b) {
  XformOp64 ops[RT_MAX_XFORM_OPS];
  const int n_ops = member_ops64(S, slot, slot_ops64, ops);
  member_box_through_ops(local, ops, n_ops, b);
}

RT_HD bool box_is_finite(const double* b) {
  for (int a = 0; a < 6; ++a)
    if (!(rt_fabs(b[a]) < __builtin_huge_val())) return false;
  return true;
}

// x narrowed to f32 toward -inf / +inf: narrow_down / narrow_up of host/f32_layout.hpp (a round-to-nearest cast, then one step
// outward when it landed inside), without nextafterf so that the device rounds with the same text.
RT_HD float f32_from_bits(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
RT_HD uint32_t f32_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
RT_HD float f32_step_down(float f) {  // nextafterf(f, -inf) for a finite f or +inf
  const uint32_t u = f32_bits(f);
  if ((u & 0x7fffffffu) == 0u) return f32_from_bits(0x80000001u);
  return f32_from_bits((u >> 31) ? u + 1u : u - 1u);
}
RT_HD float f32_step_up(float f) {  // nextafterf(f, +inf) for a finite f or -inf
  const uint32_t u = f32_bits(f);
  if ((u & 0x7fffffffu) == 0u) return f32_from_bits(0x00000001u);
  return f32_from_bits((u >> 31) ? u - 1u : u + 1u);
}
RT_HD float f32_narrow_down(double x) { const float f = (float)x; return (double)f > x ? f32_step_down(f) : f; }
RT_HD float f32_narrow_up(double x) { const float f = (float)x; return (double)f < x ? f32_step_up(f) : f; }

}  // namespace rt
