// Host checker of nearest-point queries (tests/test_nearest_cases.py, tests/test_gpu_nearest.py): the shared core
// (core/nearest.hpp) compiled for the CPU with the flags oracle/Makefile gives the O2 checker.  Two entries over a flat scene:
//   host_nearest             the culled walk, world_nearest<rt::F_ALL, true>, with its counters.  k_nearest must equal it bit for bit.
//   host_nearest_exhaustive  plain loops over every slot and every ref: no box, no ordering, no stack.  It shares prim_nearest and
//                            the key rule (nearest_offer) with the product and nothing else; the transforms are written out here.
// Built as it is (f64) and with -DNEAREST_HOST_F32 (the float judge: the four defines of oracle/o2_flat_f32.cpp, the scene
// narrowed by the product's converter through oracle_f32_images, p / time / r_max narrowed with the casts k_nearest uses).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#ifdef NEAREST_HOST_F32
#include "../ray-tracing-series-rust_amd/csrc/host/f32_blobs.hpp"
#define RT_F32 1
#define RT_REAL float
#define rt rt32
#define rtx rtx32
#include "../ray-tracing-series-rust_amd/csrc/core/cull32.hpp"
#endif
#include "../ray-tracing-series-rust_amd/csrc/core/nearest.hpp"
#include "../ray-tracing-series-rust_amd/csrc/host/flat_scene.hpp"

#ifdef NEAREST_HOST_F32
extern "C" int oracle_f32_images(const void* flat, RtxF32Blobs* blobs, void** keep);
extern "C" void oracle_f32_images_free(void* keep);

namespace {
template <class T>
bool take_blob(const RtxF32Blobs& b, int which, std::vector<T>* out) {  // csrc/hip/f32_entry.inc
  if (b.bytes[which] == 0) { out->clear(); return true; }
  if (b.elem_bytes[which] != sizeof(T) || b.bytes[which] % sizeof(T) != 0) return false;
  out->resize(b.bytes[which] / sizeof(T));
  memcpy((void*)out->data(), b.data[which], b.bytes[which]);
  return true;
}

bool narrow_scene(const void* flat, rtx::FlatScene* fs) {  // oracle/o2_flat_f32.cpp
  RtxF32Blobs b;
  void* keep = nullptr;
  if (oracle_f32_images(flat, &b, &keep) != 0) { oracle_f32_images_free(keep); return false; }
  bool ok = take_blob(b, RTX32_SPHERES, &fs->spheres) && take_blob(b, RTX32_MOVING_SPHERES, &fs->moving_spheres) &&
            take_blob(b, RTX32_RECTS, &fs->rects) && take_blob(b, RTX32_TRIANGLES, &fs->triangles) &&
            take_blob(b, RTX32_NODES, &fs->nodes) && take_blob(b, RTX32_NODES32, &fs->nodes32) &&
            take_blob(b, RTX32_REFS, &fs->refs) && take_blob(b, RTX32_ENTRIES, &fs->entries) &&
            take_blob(b, RTX32_TOP_LEVEL, &fs->top_level) && take_blob(b, RTX32_MATERIALS, &fs->materials) &&
            take_blob(b, RTX32_TEXTURES, &fs->textures) && take_blob(b, RTX32_PERLINS, &fs->perlins) &&
            take_blob(b, RTX32_IMAGES, &fs->images) && take_blob(b, RTX32_TEXELS, &fs->texels) &&
            take_blob(b, RTX32_TOP_BOX32, &fs->top_box32) && take_blob(b, RTX32_GRAVITY_SPHERES, &fs->gravity_spheres) &&
            take_blob(b, RTX32_GRAVITY_Y, &fs->gravity_y) && take_blob(b, RTX32_MOTION32, &fs->motion32);
  fs->max_stack = b.max_stack;
  fs->n_bvh = b.n_bvh;
  fs->features = b.features;
  oracle_f32_images_free(keep);
  return ok;
}
}  // namespace
#define NEAREST_ENTRY(name) name##_f32
#else
#define NEAREST_ENTRY(name) name
#endif

namespace {

// Every slot, every ref, in list order; a ConstantMedium's boundary with media, its XFORM chain walked by hand.
void exhaustive(const rt::SceneView& sv, rt::Vec3 p, rt::real time, rt::real r_max, bool media, rt::NearestBest* best,
                rt::NearestCounters* cnt) {
  rt::nearest_begin(best, r_max);
  for (int32_t i = 0; i < sv.n_top_level; ++i) {
    const rt::FlatEntry* e = &sv.entries[sv.top_level[i]];
    int32_t medium_mat = -1;
    if (e->kind == rt::ENTRY_MEDIUM) {
      if (!media) continue;
      medium_mat = e->b;
      e = &sv.entries[e->a];
    }
    const rt::FlatEntry* solid = e;
    rt::Vec3 pl = p;
    int nops = 0;
    if (e->kind == rt::ENTRY_XFORM) {
      nops = e->b;
      for (int k = 0; k < nops; ++k) {
        const rt::FlatXformOp& op = solid->ops[k];
        if (op.op == rt::XFORM_TRANSLATE) pl = rt::v3(pl.x - op.v[0], pl.y - op.v[1], pl.z - op.v[2]);
        else pl = rt::v3(op.v[1] * pl.x - op.v[0] * pl.z, pl.y, op.v[0] * pl.x + op.v[1] * pl.z);
      }
      e = &sv.entries[solid->a];
    }
    best->changed = false;
    if (e->kind == rt::ENTRY_PRIM) rt::nearest_offer<rt::F_ALL, true>(sv, (rt::PrimRef)e->a, i, 0u, pl, time, best, cnt);
    else if (e->kind == rt::ENTRY_GROUP)
      for (int32_t k = 0; k < e->b; ++k) rt::nearest_offer<rt::F_ALL, true>(sv, sv.refs[e->a + k], i, (uint32_t)k, pl, time, best, cnt);
    else if (e->kind == rt::ENTRY_BVH)
      for (int32_t k = 0; k < e->c; ++k) rt::nearest_offer<rt::F_ALL, true>(sv, sv.refs[e->b + k], i, (uint32_t)k, pl, time, best, cnt);
    if (!best->changed) continue;
    for (int k = nops - 1; k >= 0; --k) {
      const rt::FlatXformOp& op = solid->ops[k];
      const rt::Vec3 q = best->q;
      if (op.op == rt::XFORM_TRANSLATE) best->q = rt::v3(q.x + op.v[0], q.y + op.v[1], q.z + op.v[2]);
      else best->q = rt::v3(op.v[1] * q.x + op.v[0] * q.z, q.y, -op.v[0] * q.x + op.v[1] * q.z);
    }
    best->mat_override = medium_mat;
  }
}

int run(const void* flat, bool culled, int64_t n, const double* p, const double* time, const double* r_max, double r_max_all,
        int media, double* d, double* q, int32_t* ids, unsigned long long* counters) {
  if (!flat || n < 0 || (n > 0 && !p)) return 1;
#ifdef NEAREST_HOST_F32
  rtx::FlatScene narrowed;
  if (!narrow_scene(flat, &narrowed)) return 2;
  const rtx::FlatScene& fs = narrowed;
#else
  const rtx::FlatScene& fs = *(const rtx::FlatScene*)flat;
#endif
  if (fs.features & rt::F_GRAVITY_SPHERE) return 3;
  const rt::SceneView sv = fs.view();
  std::vector<rt::LocalStack<256>> stack(1);
  rt::NearestCounters cnt = {0, 0};
  for (int64_t r = 0; r < n; ++r) {
    const rt::Vec3 pt = rt::v3((rt::real)p[3 * r], (rt::real)p[3 * r + 1], (rt::real)p[3 * r + 2]);
    const rt::real t = (rt::real)(time ? time[r] : 0.0), rm = (rt::real)(r_max ? r_max[r] : r_max_all);
    rt::NearestBest best;
    if (culled) {
      stack[0].reset();
      rt::world_nearest<rt::F_ALL, true>(sv, pt, t, rm, media != 0, &best, stack[0], &cnt);
    } else {
      exhaustive(sv, pt, t, rm, media != 0, &best, &cnt);
    }
    if (d) d[r] = best.found ? (double)rt::rt_sqrt(best.d2) : (double)INFINITY;
    if (q) {
      q[3 * r] = best.found ? (double)best.q.x : 0.0;
      q[3 * r + 1] = best.found ? (double)best.q.y : 0.0;
      q[3 * r + 2] = best.found ? (double)best.q.z : 0.0;
    }
    if (ids) {
      ids[4 * r] = best.found ? rt::nearest_material(sv, best) : -1;
      ids[4 * r + 1] = best.found ? best.slot : -1;
      ids[4 * r + 2] = best.found ? (int32_t)rt::primref_type(best.ref) : -1;
      ids[4 * r + 3] = best.found ? (int32_t)rt::primref_index(best.ref) : -1;
    }
  }
  if (counters) { counters[0] = cnt.box_tests; counters[1] = cnt.prim_tests; }
  return 0;
}

}  // namespace

// The ref list of the BVH (or GROUP) below top-level slot `slot`, in list order -- position k is the `order` of the key -- as
// {PrimType, index in that type's array} pairs into refs[2 * cap]; returns the list's length, -1 for a slot that holds neither.
// Reads the flat arrays alone: nothing of core/nearest.hpp.
extern "C" int64_t NEAREST_ENTRY(host_slot_refs)(const void* flat, int32_t slot, int32_t* refs, int64_t cap) {
  const rtx::FlatScene& fs = *(const rtx::FlatScene*)flat;
  if (slot < 0 || slot >= (int32_t)fs.top_level.size()) return -1;
  const rt::FlatEntry* e = &fs.entries[fs.top_level[slot]];
  if (e->kind == rt::ENTRY_MEDIUM || e->kind == rt::ENTRY_XFORM) e = &fs.entries[e->a];
  if (e->kind == rt::ENTRY_XFORM) e = &fs.entries[e->a];
  int64_t first, count;
  if (e->kind == rt::ENTRY_BVH) { first = e->b; count = e->c; }
  else if (e->kind == rt::ENTRY_GROUP) { first = e->a; count = e->b; }
  else return -1;
  for (int64_t k = 0; k < count && k < cap; ++k) {
    refs[2 * k] = (int32_t)rt::primref_type(fs.refs[first + k]);
    refs[2 * k + 1] = (int32_t)rt::primref_index(fs.refs[first + k]);
  }
  return count;
}

// d [n], q [n][3], ids [n][4] (any may be NULL) of points 0 .. n - 1 (time NULL: 0; r_max NULL: r_max_all); counters (or NULL):
// {box tests, primitive tests} of the whole batch.  0 on success, 3 for a scene with GravitySpheres.
extern "C" int NEAREST_ENTRY(host_nearest)(const void* flat, int64_t n, const double* p, const double* time, const double* r_max,
                                           double r_max_all, int media, double* d, double* q, int32_t* ids,
                                           unsigned long long* counters) {
  return run(flat, true, n, p, time, r_max, r_max_all, media, d, q, ids, counters);
}
extern "C" int NEAREST_ENTRY(host_nearest_exhaustive)(const void* flat, int64_t n, const double* p, const double* time,
                                                      const double* r_max, double r_max_all, int media, double* d, double* q,
                                                      int32_t* ids, unsigned long long* counters) {
  return run(flat, false, n, p, time, r_max, r_max_all, media, d, q, ids, counters);
}
