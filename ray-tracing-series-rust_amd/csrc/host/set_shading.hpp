// rtx_flat_set_shading on the host, and everything of rtx_scene_set_shading that needs no device: the shadow a scene keeps of
// its shading tables, the check ladder, and the plan that resolves edits into write records (core/shading_edit.hpp).  Pure
// host code, compiled by abi.cpp, by both compilations of render.hip and by tests/set_shading_host_check.cpp; nothing here
// reads a `real` except through shading_write_apply.
//
// An edit replaces a colour, a noise scale, a metal's or a glass's parameters or a medium's density; the result must be the
// flat scene flatten_scene builds from scratch when the builder calls are made with the new values, byte for byte in
// `materials`, `textures` and `entries` (and, through them, the light table build_light_table derives).  Kinds, which texture
// a material names, a checker's children, Perlin tables and image texels stay as they are.
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <utility>
#include <vector>
#include "../../../include/rtx_abi.h"
#include "../core/shading_edit.hpp"
#include "flat_scene.hpp"

namespace rtx {

// What an edit is checked against and planned from, derived from the arrays alone: a flat scene builds it on the fly, a
// resident scene keeps it from its upload.  Kinds and cross references never change, so it never goes stale.
struct ShadingShadow {
  std::vector<int32_t> mat_kind, mat_tex;        // per material
  std::vector<int32_t> tex_kind;                 // per texture
  std::vector<std::vector<int32_t>> tex_users;   // per texture: the materials that hold a copy of its colour (flatten.cpp: run) --
                                                 // every Lambertian / DiffuseLight / Isotropic that names it when it is a SolidColor
  std::vector<int32_t> medium_entry;             // per top-level slot: the index of its ENTRY_MEDIUM, -1 for any other slot
  std::string broken;                            // not empty: the arrays are not what the flattener emits; the message says how
};

inline bool material_copies_colour(int32_t kind) { return kind == rt::MAT_LAMBERTIAN || kind == rt::MAT_DIFFUSE_LIGHT || kind == rt::MAT_ISOTROPIC; }

inline ShadingShadow build_shading_shadow(const FlatScene& fs) {
  ShadingShadow sh;
  sh.tex_kind.resize(fs.textures.size());
  sh.tex_users.resize(fs.textures.size());
  for (size_t t = 0; t < fs.textures.size(); ++t) sh.tex_kind[t] = fs.textures[t].kind;
  sh.mat_kind.resize(fs.materials.size());
  sh.mat_tex.resize(fs.materials.size());
  for (size_t m = 0; m < fs.materials.size(); ++m) {
    const int32_t kind = fs.materials[m].kind, tex = fs.materials[m].tex;
    sh.mat_kind[m] = kind;
    sh.mat_tex[m] = tex;
    if (!material_copies_colour(kind)) continue;
    if (tex < 0 || (size_t)tex >= fs.textures.size()) { sh.broken = "material " + std::to_string(m) + " names a texture outside the texture array"; return sh; }
    if (sh.tex_kind[(size_t)tex] == rt::TEX_SOLID) sh.tex_users[(size_t)tex].push_back((int32_t)m);
  }
  sh.medium_entry.assign(fs.top_level.size(), -1);
  for (size_t s = 0; s < fs.top_level.size(); ++s) {
    const int32_t e = fs.top_level[s];
    if (e < 0 || (size_t)e >= fs.entries.size()) { sh.broken = "slot " + std::to_string(s) + " names an entry outside the entry array"; return sh; }
    if (fs.entries[(size_t)e].kind == rt::ENTRY_MEDIUM) sh.medium_entry[s] = e;
  }
  return sh;
}

namespace shading_detail {
inline const char* mat_kind_name(int32_t k) {
  switch (k) {
    case rt::MAT_LAMBERTIAN: return "Lambertian";
    case rt::MAT_METAL: return "Metal";
    case rt::MAT_DIELECTRIC: return "Dielectric";
    case rt::MAT_DIFFUSE_LIGHT: return "DiffuseLight";
    case rt::MAT_ISOTROPIC: return "Isotropic";
    default: return "material of an unknown kind";
  }
}
inline const char* tex_kind_name(int32_t k) {
  switch (k) {
    case rt::TEX_SOLID: return "SolidColor";
    case rt::TEX_CHECKER: return "Checker";
    case rt::TEX_NOISE: return "Noise";
    case rt::TEX_IMAGE: return "Image";
    default: return "texture of an unknown kind";
  }
}
// 0 texture, 1 material, 2 slot: what `index` of an edit names; the values of v an edit uses
inline int target_class(int32_t what) { return what <= RTX_SHADE_NOISE_SCALE ? 0 : (what <= RTX_SHADE_DIELECTRIC ? 1 : 2); }
inline int used_values(int32_t what) { return what == RTX_SHADE_SOLID_COLOR ? 3 : (what == RTX_SHADE_METAL ? 4 : 1); }
// The spelling that works for a material the edit's `what` does not fit.
inline std::string material_advice(const ShadingShadow& sh, int32_t m) {
  const int32_t kind = sh.mat_kind[(size_t)m];
  if (material_copies_colour(kind)) {
    const int32_t tex = sh.mat_tex[(size_t)m];
    return std::string("a ") + mat_kind_name(kind) + " takes its colour from a texture: edit its texture `tex` (" + std::to_string(tex) + ", a " +
           tex_kind_name(sh.tex_kind[(size_t)tex]) + ")";
  }
  if (kind == rt::MAT_METAL) return "a Metal is edited with RTX_SHADE_METAL";
  if (kind == rt::MAT_DIELECTRIC) return "a Dielectric is edited with RTX_SHADE_DIELECTRIC";
  return "no edit applies to it";
}
inline std::string texture_advice(const ShadingShadow& sh, int32_t t) {
  const int32_t kind = sh.tex_kind[(size_t)t];
  if (kind == rt::TEX_SOLID) return "a SolidColor is edited with RTX_SHADE_SOLID_COLOR";
  if (kind == rt::TEX_NOISE) return "a Noise is edited with RTX_SHADE_NOISE_SCALE";
  if (kind == rt::TEX_CHECKER) return "a Checker holds no colour of its own: edit its children `a` and `b` where they are SolidColors";
  return "image texels are not edited";
}
}  // namespace shading_detail

// Step 1 of the ladder: what needs neither the scene nor an edit's contents.
inline bool check_shading_args(const char* who, const void* scene, const RtxShadingEdit* edits, int64_t n, std::string* err) {
  if (!scene) { *err = std::string(who) + ": the scene is NULL"; return false; }
  if (n < 0) { *err = std::string(who) + ": n < 0"; return false; }
  if (!edits && n > 0) { *err = std::string(who) + ": edits is NULL"; return false; }
  return true;
}

// Steps 2 and 3: per edit, in the order of the header (what, index, kind, finite, unused v); then a target named twice.
inline bool check_shading_edits(const char* who, const ShadingShadow& sh, const RtxShadingEdit* e, int64_t n, std::string* err) {
  using namespace shading_detail;
  auto bad = [&](int64_t i, const std::string& what) { *err = std::string(who) + ": edits[" + std::to_string(i) + "]" + what; return false; };
  if (!sh.broken.empty()) { *err = std::string(who) + ": " + sh.broken; return false; }
  for (int64_t i = 0; i < n; ++i) {
    const int32_t what = e[i].what, ix = e[i].index;
    if (what < RTX_SHADE_SOLID_COLOR || what > RTX_SHADE_MEDIUM_DENSITY) return bad(i, ".what is " + std::to_string(what) + ", not one of RTX_SHADE_*");
    const int cls = target_class(what);
    const size_t count = cls == 0 ? sh.tex_kind.size() : (cls == 1 ? sh.mat_kind.size() : sh.medium_entry.size());
    if (ix < 0 || (size_t)ix >= count)
      return bad(i, ".index is out of range (the scene has " + std::to_string(count) + (cls == 0 ? " textures)" : (cls == 1 ? " materials)" : " top-level slots)")));
    if (what == RTX_SHADE_SOLID_COLOR && sh.tex_kind[(size_t)ix] != rt::TEX_SOLID)
      return bad(i, ".index names a texture that is not a SolidColor: " + texture_advice(sh, ix));
    if (what == RTX_SHADE_NOISE_SCALE && sh.tex_kind[(size_t)ix] != rt::TEX_NOISE)
      return bad(i, ".index names a texture that is not a Noise: " + texture_advice(sh, ix));
    if (what == RTX_SHADE_METAL && sh.mat_kind[(size_t)ix] != rt::MAT_METAL)
      return bad(i, ".index names a material that is not a Metal: " + material_advice(sh, ix));
    if (what == RTX_SHADE_DIELECTRIC && sh.mat_kind[(size_t)ix] != rt::MAT_DIELECTRIC)
      return bad(i, ".index names a material that is not a Dielectric: " + material_advice(sh, ix));
    if (what == RTX_SHADE_MEDIUM_DENSITY && sh.medium_entry[(size_t)ix] < 0)
      return bad(i, ".index names a slot that is not a ConstantMedium (rtx_flat_top_level_kind 4)");
    const int used = used_values(what);
    for (int a = 0; a < used; ++a)
      if (!std::isfinite(e[i].v[a])) return bad(i, ".v[" + std::to_string(a) + "] is not finite");
    for (int a = used; a < 4; ++a)
      if (!(e[i].v[a] == 0.0)) return bad(i, ".v[" + std::to_string(a) + "] is not used by this edit and must be 0");
  }
  std::vector<std::pair<int32_t, int32_t>> targets((size_t)n);
  for (int64_t i = 0; i < n; ++i) targets[(size_t)i] = {target_class(e[i].what), e[i].index};
  std::sort(targets.begin(), targets.end());
  for (size_t i = 1; i < targets.size(); ++i)
    if (targets[i] == targets[i - 1]) {
      static const char* names[3] = {"texture", "material", "slot"};
      *err = std::string(who) + ": edits name " + names[targets[i].first] + " " + std::to_string(targets[i].second) + " twice (.index)";
      return false;
    }
  return true;
}

// Checked edits -> the write records, in edit order, a colour's copies behind the colour.  with_desc: the scene keeps
// k_trace_world's slot table (a resident scene).  *texture_edit: a batch after which a light table is recomputed.
inline std::vector<rt::ShadingWrite> plan_shading(const ShadingShadow& sh, const RtxShadingEdit* e, int64_t n, bool with_desc, bool* texture_edit) {
  std::vector<rt::ShadingWrite> out;
  *texture_edit = false;
  auto record = [&](int32_t tag, int32_t element, const double* v, int count) {
    rt::ShadingWrite w;
    w.tag = tag; w.element = element;
    for (int a = 0; a < 4; ++a) w.v[a] = a < count ? v[a] : 0.0;
    out.push_back(w);
  };
  for (int64_t i = 0; i < n; ++i) {
    double v[4];
    switch (e[i].what) {
      case RTX_SHADE_SOLID_COLOR:
        record(rt::SW_TEX_COLOR, e[i].index, e[i].v, 3);
        for (int32_t m : sh.tex_users[(size_t)e[i].index]) record(rt::SW_MAT_ALBEDO, m, e[i].v, 3);
        *texture_edit = true;
        break;
      case RTX_SHADE_NOISE_SCALE:
        record(rt::SW_TEX_SCALE, e[i].index, e[i].v, 1);
        *texture_edit = true;
        break;
      case RTX_SHADE_METAL:
        rt::shading_metal_values(e[i].v, e[i].v[3], v);
        record(rt::SW_MAT_SURFACE, e[i].index, v, 4);
        break;
      case RTX_SHADE_DIELECTRIC:
        rt::shading_dielectric_values(e[i].v[0], v);
        record(rt::SW_MAT_SURFACE, e[i].index, v, 4);
        break;
      default:  // RTX_SHADE_MEDIUM_DENSITY
        v[0] = rt::shading_medium_value(e[i].v[0]);
        record(rt::SW_ENTRY_DENSITY, sh.medium_entry[(size_t)e[i].index], v, 1);
        if (with_desc) record(rt::SW_DESC_DENSITY, e[i].index, v, 1);
        break;
    }
  }
  return out;
}

// rtx_flat_set_shading: every check first, then the edit.  false with *err set and *fs untouched.
inline bool flat_set_shading(const char* who, FlatScene* fs, const RtxShadingEdit* edits, int64_t n, std::string* err) {
  if (!check_shading_args(who, fs, edits, n, err)) return false;
  if (n == 0) return true;
  const ShadingShadow sh = build_shading_shadow(*fs);
  if (!check_shading_edits(who, sh, edits, n, err)) return false;
  bool texture_edit = false;
  for (const rt::ShadingWrite& w : plan_shading(sh, edits, n, false, &texture_edit))
    rt::shading_write_apply(w, fs->materials.data(), fs->textures.data(), fs->entries.data(), (rt::ShadingNoDesc*)nullptr);
  return true;
}

}  // namespace rtx
