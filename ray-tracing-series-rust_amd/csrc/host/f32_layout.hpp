// f64 flat arrays -> byte images in the layouts of the f32 compilation.  Pure host code: hip/f32_convert.inc uploads
// these images, the float CPU checker (oracle/o2_flat_f32.cpp) walks the same bytes.
//
// Each struct of core/flat_types.hpp is described once, as the sequence of its fields: r = real, d / u = real that must
// round down / up when it narrows (box planes: the narrowed box still contains the f64 one), i = 32-bit integer,
// l = 64-bit integer, each followed by a repeat count.  Offsets follow from natural alignment for either width of
// `real`; the f64 size is checked against sizeof here and the f32 size against sizeof in the other compilation
// (f32_entry.inc: take_blob), so a field added to a struct without its descriptor fails the first upload loudly.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "f32_blobs.hpp"
#include "flat_scene.hpp"

namespace rtx {

struct F32Field { char kind; uint32_t count; };
struct F32Layout {
  std::vector<F32Field> fields;
  size_t size64 = 0, size32 = 0;
};

static F32Layout f32_layout(const char* desc) {
  F32Layout L;
  size_t o64 = 0, o32 = 0, a64 = 1, a32 = 1;
  for (const char* p = desc; *p;) {
    while (*p == ' ') ++p;
    if (!*p) break;
    F32Field f; f.kind = *p++; f.count = (uint32_t)strtoul(p, (char**)&p, 10);
    const bool is_real = f.kind == 'r' || f.kind == 'd' || f.kind == 'u';
    const size_t w64 = f.kind == 'i' ? 4 : 8, w32 = is_real ? 4 : w64;
    o64 = (o64 + w64 - 1) / w64 * w64; o32 = (o32 + w32 - 1) / w32 * w32;
    o64 += w64 * f.count; o32 += w32 * f.count;
    a64 = std::max(a64, w64); a32 = std::max(a32, w32);
    L.fields.push_back(f);
  }
  L.size64 = (o64 + a64 - 1) / a64 * a64;
  L.size32 = (o32 + a32 - 1) / a32 * a32;
  return L;
}

static inline float narrow_down(double x) { float f = (float)x; return (double)f > x ? std::nextafterf(f, -INFINITY) : f; }
static inline float narrow_up(double x) { float f = (float)x; return (double)f < x ? std::nextafterf(f, INFINITY) : f; }

// n elements of size64 bytes each at `in` -> n elements of the f32 layout.  false when `desc` does not describe size64 bytes.
static bool f32_convert_bytes(const void* in, size_t n, size_t elem64, const char* desc, std::vector<unsigned char>* out,
                              size_t* elem_bytes) {
  const F32Layout L = f32_layout(desc);
  *elem_bytes = L.size32;
  if (L.size64 != elem64) return false;
  out->assign(n * L.size32, 0);
  for (size_t k = 0; k < n; ++k) {
    const unsigned char* s = (const unsigned char*)in + k * elem64;
    unsigned char* d = out->data() + k * L.size32;
    size_t o64 = 0, o32 = 0;
    for (const F32Field& f : L.fields) {
      const bool is_real = f.kind != 'i' && f.kind != 'l';
      const size_t w64 = f.kind == 'i' ? 4 : 8, w32 = is_real ? 4 : w64;
      o64 = (o64 + w64 - 1) / w64 * w64; o32 = (o32 + w32 - 1) / w32 * w32;
      for (uint32_t c = 0; c < f.count; ++c, o64 += w64, o32 += w32) {
        if (!is_real) { memcpy(d + o32, s + o64, w64); continue; }
        double x; memcpy(&x, s + o64, 8);
        const float y = f.kind == 'd' ? narrow_down(x) : (f.kind == 'u' ? narrow_up(x) : (float)x);
        memcpy(d + o32, &y, 4);
      }
    }
  }
  return true;
}

template <class T>
static bool f32_convert(const std::vector<T>& in, const char* desc, std::vector<unsigned char>* out, size_t* elem_bytes) {
  return f32_convert_bytes(in.data(), in.size(), sizeof(T), desc, out, elem_bytes);
}

// The descriptor of every array whose elements hold reals; the other arrays cross as they are.
struct F32Desc { RtxF32Array which; const char* name; const char* desc; };
static const F32Desc F32_DESCS[] = {
  {RTX32_SPHERES, "spheres", "r4 i2"},
  {RTX32_MOVING_SPHERES, "moving_spheres", "r9 i2"},
  {RTX32_RECTS, "rects", "r5 i2"},
  {RTX32_TRIANGLES, "triangles", "r12 i2"},
  {RTX32_NODES, "nodes", "d6 u6 i4"},
  {RTX32_ENTRIES, "entries", "i4 r2 i2 r3 i2 r3 i2 r3 i2 r3"},
  {RTX32_MATERIALS, "materials", "i2 r4 i2"},
  {RTX32_TEXTURES, "textures", "i4 r4"},
  {RTX32_PERLINS, "perlins", "r768 i768"},
  {RTX32_GRAVITY_SPHERES, "gravity_spheres", "r5 i2 l2"},
  {RTX32_TEXELS, "texels", "r1"},
  {RTX32_GRAVITY_Y, "gravity_y", "r1"},
};
static inline const char* f32_desc(RtxF32Array which) {
  for (const F32Desc& d : F32_DESCS) if (d.which == which) return d.desc;
  return nullptr;
}

// Every array of `fs` as the f32 compilation takes it: the converted ones live in img[], the others are shared with fs
// (both must outlive *b).  false when a descriptor does not match its struct.
static bool f32_images(const FlatScene& fs, std::vector<unsigned char> img[RTX32_N_ARRAYS], RtxF32Blobs* b) {
  memset(b, 0, sizeof(*b));
  bool ok = true;
#define CONVERT(WHICH, VEC) \
  ok = ok && f32_convert(fs.VEC, f32_desc(WHICH), &img[WHICH], &b->elem_bytes[WHICH]); b->data[WHICH] = img[WHICH].data(); b->bytes[WHICH] = img[WHICH].size()
#define SHARE(WHICH, VEC) \
  b->data[WHICH] = fs.VEC.data(); b->bytes[WHICH] = fs.VEC.size() * sizeof(fs.VEC[0]); b->elem_bytes[WHICH] = sizeof(fs.VEC[0])
  CONVERT(RTX32_SPHERES, spheres);
  CONVERT(RTX32_MOVING_SPHERES, moving_spheres);
  CONVERT(RTX32_RECTS, rects);
  CONVERT(RTX32_TRIANGLES, triangles);
  CONVERT(RTX32_NODES, nodes);
  CONVERT(RTX32_ENTRIES, entries);
  CONVERT(RTX32_MATERIALS, materials);
  CONVERT(RTX32_TEXTURES, textures);
  CONVERT(RTX32_PERLINS, perlins);
  CONVERT(RTX32_GRAVITY_SPHERES, gravity_spheres);
  CONVERT(RTX32_TEXELS, texels);
  CONVERT(RTX32_GRAVITY_Y, gravity_y);
  SHARE(RTX32_NODES32, nodes32);
  SHARE(RTX32_MOTION32, motion32);
  SHARE(RTX32_REFS, refs);
  SHARE(RTX32_TOP_LEVEL, top_level);
  SHARE(RTX32_IMAGES, images);
  SHARE(RTX32_TOP_BOX32, top_box32);
  SHARE(RTX32_MEMBER_LOCAL_BOX, member_local_box);
  {
    // the ops of every slot's chain as they are BEFORE the (float) cast above: a refit on the f32 side computes a member's box
    // in f64 from these, as the flattener did, and narrows the box -- never a box from narrowed ops
    std::vector<unsigned char>& im = img[RTX32_SLOT_OPS64];
    im.assign(fs.top_level.size() * RT_MAX_XFORM_OPS * sizeof(rt::XformOp64), 0);
    for (size_t k = 0; k < fs.top_level.size(); ++k) {
      const rt::FlatEntry* E = &fs.entries[(size_t)fs.top_level[k]];
      if (E->kind == rt::ENTRY_MEDIUM) E = &fs.entries[(size_t)E->a];
      if (E->kind != rt::ENTRY_XFORM) continue;
      for (int i = 0; i < E->b; ++i) {
        rt::XformOp64 op;
        op.op = E->ops[i].op; op.pad = 0;
        for (int a = 0; a < 3; ++a) op.v[a] = E->ops[i].v[a];
        memcpy(im.data() + (k * RT_MAX_XFORM_OPS + (size_t)i) * sizeof(op), &op, sizeof(op));
      }
    }
    b->data[RTX32_SLOT_OPS64] = im.data(); b->bytes[RTX32_SLOT_OPS64] = im.size(); b->elem_bytes[RTX32_SLOT_OPS64] = sizeof(rt::XformOp64);
  }
#undef CONVERT
#undef SHARE
  b->max_stack = fs.max_stack;
  b->n_bvh = fs.n_bvh;
  b->features = fs.features;
  return ok;
}

}  // namespace rtx
