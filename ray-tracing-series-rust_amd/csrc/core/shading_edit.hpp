// New shading parameters for a flattened scene (rtx_flat_set_shading / rtx_scene_set_shading): THE text of what an edit
// writes, shared by the host edit (host/set_shading.hpp) and the device kernel (hip/shading_update.inc: k_set_shading).
//
// An edit is resolved on the host into write records: which array, which element, up to four doubles.  The doubles are
// computed here with the builder's own arithmetic (scene_graph.cpp, flatten.cpp), always in f64; a record is applied here too,
// by one function, with a cast to the field's type -- `real` is double in the parity build and float in the fast mode, where
// the cast is the converter's plain (float) of host/f32_layout.hpp ('r' fields).  So the flat scene, a resident f64 scene and a
// resident f32 scene all end up with the bytes a fresh flatten (and upload) of the new values gives.
#pragma once
#include "flat_types.hpp"

namespace rt {

enum ShadingWriteTag : int32_t {
  SW_TEX_COLOR = 0,      // textures[element].color = v[0..3)
  SW_TEX_SCALE = 1,      // textures[element].scale = v[0]
  SW_MAT_ALBEDO = 2,     // materials[element].albedo = v[0..3): the flattener's copy of a SolidColor in a material that names it
  SW_MAT_SURFACE = 3,    // materials[element].albedo = v[0..3), .param = v[3]: a Metal or a Dielectric
  SW_ENTRY_DENSITY = 4,  // entries[element].f[0] = v[0]: a medium's -1 / density
  SW_DESC_DENSITY = 5,   // k_trace_world's slot record [element].neg_inv_density = v[0] (resident scenes only)
};
struct ShadingWrite {  // 40 B
  int32_t tag, element;
  double v[4];
};

// rtx_metal(rgb, fuzz) as the material record holds it: the colour, and the fuzz clamped from above only (scene_graph.cpp:
// SceneGraph::metal, hit.rs:1063) -- a negative fuzz passes as the builder passes it.
RT_HD void shading_metal_values(const double rgb[3], double fuzz, double out[4]) {
  out[0] = rgb[0]; out[1] = rgb[1]; out[2] = rgb[2];
  out[3] = fuzz < 1.0 ? fuzz : 1.0;
}
// rtx_dielectric(ir) as the material record holds it: dielectric_constants(ir) of shading.hpp in f64 whatever `real` is
// (the flattener runs it in f64 and the converter narrows the results), then ir itself.
RT_HD void shading_dielectric_values(double ir, double out[4]) {
  out[0] = 1.0 / ir;
  double r0 = (1.0 - out[0]) / (1.0 + out[0]);
  out[1] = r0 * r0;
  r0 = (1.0 - ir) / (1.0 + ir);
  out[2] = r0 * r0;
  out[3] = ir;
}
// rtx_constant_medium's density as the entry holds it (hit.rs:951: neg_inv_density); density 0 gives -inf there too.
RT_HD double shading_medium_value(double density) { return -1.0 / density; }

// A scene without a slot table (the host flat scene) applies records with this for DESC and desc = nullptr.
struct ShadingNoDesc { real neg_inv_density; };

// One write record applied to the arrays.  Every index was formed and checked by the host's plan (host/set_shading.hpp); a
// value is only ever stored.
template <class DESC>
RT_HD void shading_write_apply(const ShadingWrite& w, FlatMaterial* materials, FlatTexture* textures, FlatEntry* entries, DESC* desc) {
  switch (w.tag) {
    case SW_TEX_COLOR:
      for (int a = 0; a < 3; ++a) textures[w.element].color[a] = (real)w.v[a];
      break;
    case SW_TEX_SCALE:
      textures[w.element].scale = (real)w.v[0];
      break;
    case SW_MAT_ALBEDO:
    case SW_MAT_SURFACE:
      for (int a = 0; a < 3; ++a) materials[w.element].albedo[a] = (real)w.v[a];
      if (w.tag == SW_MAT_SURFACE) materials[w.element].param = (real)w.v[3];
      break;
    case SW_ENTRY_DENSITY:
      entries[w.element].f[0] = (real)w.v[0];
      break;
    case SW_DESC_DENSITY:
      if (desc) desc[w.element].neg_inv_density = (real)w.v[0];
      break;
    default:
      break;
  }
}

}  // namespace rt
