// Byte images of a flattened scene in the layouts of the f32 compilation: what crosses from the f64 side (which owns
// the flat arrays and converts them, host/f32_layout.hpp) to an f32 side (hip/render_f32.hip on the device, the float
// CPU checker oracle/o2_flat_f32.cpp on the host).  Nothing here mentions a type of either namespace, so every
// compilation sees the same declarations.
#pragma once
#include <cstddef>
#include <cstdint>

enum RtxF32Array : int {
  RTX32_SPHERES = 0, RTX32_MOVING_SPHERES, RTX32_RECTS, RTX32_TRIANGLES, RTX32_NODES, RTX32_NODES32, RTX32_REFS,
  RTX32_ENTRIES, RTX32_TOP_LEVEL, RTX32_MATERIALS, RTX32_TEXTURES, RTX32_PERLINS, RTX32_IMAGES, RTX32_TEXELS,
  RTX32_TOP_BOX32, RTX32_GRAVITY_SPHERES, RTX32_GRAVITY_Y, RTX32_MOTION32,
  // what a refit of an f32 scene starts from, in f64 (FlatScene::member_local_box, ::slot_ops64)
  RTX32_MEMBER_LOCAL_BOX, RTX32_SLOT_OPS64, RTX32_N_ARRAYS
};
struct RtxF32Blobs {
  const void* data[RTX32_N_ARRAYS];
  size_t bytes[RTX32_N_ARRAYS];
  size_t elem_bytes[RTX32_N_ARRAYS];  // what the converter believes one element occupies; checked against sizeof on the other side
  int32_t max_stack, n_bvh;
  uint32_t features;
};
