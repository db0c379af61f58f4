// ORACLE O2f, second build -- TEST INFRASTRUCTURE.  o2_flat_f32.cpp once more with the five platform functions computed
// in double and rounded to float (core/rt_math.hpp: RT_F32_MATH_VIA_F64) instead of glibc's sinf cosf logf acosf atan2f,
// in namespaces of its own: exports oracle_o2g_render / oracle_o2g_sample.
#define O2F_VIA_F64 1
#include "o2_flat_f32.cpp"
