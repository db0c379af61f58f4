// Host checker of rtx_flat_set_shading (tests/test_set_shading_host.py builds it with the product's host sources under
// -fsanitize=address,undefined and runs it).  A CPU program with its own main; nothing of it is loaded into Python.
// Worlds: `look`: one SolidColor shared by a Lambertian, a DiffuseLight, an Isotropic and a checker, two metals, a glass and a
// noise-lit rectangle in a BVH world; `fog`: three media (around a sphere, a box and a moved box) beside a sphere light.  Each is
// built at rest, edited with full, partial and repeated edits and compared with the world flattened from scratch with those
// values (the light table included); edited back, every array must be what it was.  Then the refusals, in the ladder's order,
// each of which must leave the scene untouched.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../ray-tracing-series-rust_amd/csrc/host/light_table.hpp"
#include "../ray-tracing-series-rust_amd/csrc/host/set_shading.hpp"

namespace rtx {
// the GPU builder lives in csrc/hip/lbvh.hip: not part of a CPU-only program
int32_t build_bvh_gpu(const std::vector<double>&, int, std::vector<rt::FlatNode>*, std::vector<uint32_t>*, int32_t*, double*, std::string* err) {
  if (err) *err = "no GPU builder in the sanitizer program";
  return -1;
}
}  // namespace rtx

namespace {
// The values a world is built with: k-th of each kind, at rest or new per `mask` bit.
struct Vals {
  double color[3][3], scale, metal[2][4], ir, density[3];
};
Vals rest_vals() {
  return {{{1.6, 1.3, 0.9}, {0.2, 0.4, 0.9}, {6.0, 5.0, 3.0}}, 4.0, {{0.8, 0.8, 0.9, 0.1}, {0.9, 0.6, 0.3, 0.4}}, 1.5, {0.8, 0.6, 1.1}};
}
Vals new_vals() {
  return {{{0.3, 2.1, 0.6}, {0.9, 0.5, 0.1}, {0.0, 0.0, 0.0}}, 0.7, {{0.3, 0.9, 0.4, 1.5}, {0.5, 0.5, 0.9, -0.25}}, 2.4, {0.15, 0.0, 2.5}};
}
// value number k (0..2 colours, 3 scale, 4..5 metals, 6 ir, 7..9 densities) taken from `b` where the mask says so
Vals mix(const Vals& a, const Vals& b, unsigned mask) {
  Vals o = a;
  for (int k = 0; k < 3; ++k) if (mask >> k & 1) memcpy(o.color[k], b.color[k], sizeof(o.color[k]));
  if (mask >> 3 & 1) o.scale = b.scale;
  for (int k = 0; k < 2; ++k) if (mask >> (4 + k) & 1) memcpy(o.metal[k], b.metal[k], sizeof(o.metal[k]));
  if (mask >> 6 & 1) o.ir = b.ir;
  for (int k = 0; k < 3; ++k) if (mask >> (7 + k) & 1) o.density[k] = b.density[k];
  return o;
}

struct Built {
  rtx::SceneGraph g{5};
  int32_t world = -1;
  int32_t tex[3] = {-1, -1, -1}, noise = -1, metal[2] = {-1, -1}, glass = -1, slot[3] = {-1, -1, -1}, lambertian = -1, checker = -1;
};

int32_t list_of(rtx::SceneGraph& g, const std::vector<int32_t>& o) { const int32_t l = g.list_new(); for (int32_t x : o) g.list_add(l, x); return l; }

void make_world(Built* B, const std::string& name, const Vals& v) {
  rtx::SceneGraph& g = B->g;
  const double grey[3] = {0.5, 0.5, 0.5}, white[3] = {0.9, 0.9, 0.9};
  auto sphere = [&](double x, double y, double z, double r, int32_t mat) { const double c[3] = {x, y, z}; return g.sphere(c, r, mat); };
  if (name == "look") {
    B->tex[0] = g.solid_color(v.color[0]);
    B->checker = g.checker(B->tex[0], g.solid_color(white));
    B->lambertian = g.lambertian(B->tex[0]);
    B->noise = g.noise(v.scale);
    B->metal[0] = g.metal(v.metal[0], v.metal[0][3]);
    B->metal[1] = g.metal(v.metal[1], v.metal[1][3]);
    B->glass = g.dielectric(v.ir);
    B->tex[2] = g.solid_color(v.color[2]);
    std::vector<int32_t> o = {sphere(2.0, -500.0, 2.0, 500.0, g.lambertian(B->checker)), sphere(1.1, 0.8, 2.3, 0.8, B->lambertian),
                              sphere(3.1, 0.7, 3.3, 0.7, g.isotropic(B->tex[0])), sphere(4.3, 0.6, 1.2, 0.6, B->metal[0]),
                              sphere(0.7, 0.5, 4.1, 0.5, B->metal[1]), sphere(2.4, 0.9, 0.8, 0.9, B->glass)};
    B->world = list_of(g, {g.bvh_from_list(list_of(g, o), 0.0, 1.0), g.rect(rtx::H_XZ_RECT, 2.2, 3.6, 2.1, 3.5, 3.4, g.diffuse_light(B->tex[0])),
                           g.rect(rtx::H_XZ_RECT, 0.2, 1.4, 0.3, 1.5, 3.1, g.diffuse_light(B->noise)), sphere(4.5, 2.5, 4.4, 0.4, g.diffuse_light(B->tex[2]))});
  } else {  // fog
    const double p0[3] = {3.1, 0.2, 3.6}, p1[3] = {4.4, 1.5, 4.9}, q0[3] = {0.0, 0.0, 0.0}, q1[3] = {1.2, 1.6, 1.1}, t[3] = {4.2, 0.3, 0.9};
    const int32_t glass = g.dielectric(1.5), lam = g.lambertian(g.solid_color(grey));
    B->tex[2] = g.solid_color(v.color[2]);
    std::vector<int32_t> o = {sphere(2.0, -500.0, 2.0, 500.0, lam), sphere(1.71, 1.32, 2.93, 1.1, glass)};
    B->slot[0] = (int32_t)o.size(); o.push_back(g.constant_medium(v.color[1], v.density[0], sphere(1.71, 1.32, 2.93, 1.1, glass)));
    B->slot[1] = (int32_t)o.size(); o.push_back(g.constant_medium(white, v.density[1], g.rect_prism(p0, p1, lam)));
    B->slot[2] = (int32_t)o.size(); o.push_back(g.constant_medium(grey, v.density[2], g.translate(t, g.rotate_y(25.0, g.rect_prism(q0, q1, lam)))));
    o.push_back(sphere(4.5, 2.5, 4.4, 0.4, g.diffuse_light(B->tex[2])));
    B->world = list_of(g, o);
  }
}

bool flatten(const std::string& name, const Vals& v, Built* B, rtx::FlatScene* fs) {
  make_world(B, name, v);
  if (B->world < 0) { fprintf(stderr, "%s: the graph was refused: %s\n", name.c_str(), B->g.error.c_str()); return false; }
  std::string err;
  if (!rtx::flatten_scene(B->g, B->world, rtx::BuildOptions(), fs, &err)) { fprintf(stderr, "flatten: %s\n", err.c_str()); return false; }
  return true;
}

RtxShadingEdit edit(int32_t what, int32_t index, const double* v, int n) {
  RtxShadingEdit e;
  memset(&e, 0, sizeof(e));
  e.what = what; e.index = index;
  for (int a = 0; a < n; ++a) e.v[a] = v[a];
  return e;
}

// the edits that give the values of `mask` (as in mix) from v; the fog's colour through the medium's phase material
std::vector<RtxShadingEdit> edits_for(const Built& B, const rtx::FlatScene& fs, const std::string& name, const Vals& v, unsigned mask) {
  std::vector<RtxShadingEdit> e;
  if (name == "look") {
    if (mask >> 0 & 1) e.push_back(edit(RTX_SHADE_SOLID_COLOR, B.tex[0], v.color[0], 3));
    if (mask >> 2 & 1) e.push_back(edit(RTX_SHADE_SOLID_COLOR, B.tex[2], v.color[2], 3));
    if (mask >> 3 & 1) e.push_back(edit(RTX_SHADE_NOISE_SCALE, B.noise, &v.scale, 1));
    for (int k = 0; k < 2; ++k) if (mask >> (4 + k) & 1) e.push_back(edit(RTX_SHADE_METAL, B.metal[k], v.metal[k], 4));
    if (mask >> 6 & 1) e.push_back(edit(RTX_SHADE_DIELECTRIC, B.glass, &v.ir, 1));
  } else {
    if (mask >> 1 & 1) {
      const rt::FlatEntry& E = fs.entries[(size_t)fs.top_level[(size_t)B.slot[0]]];
      e.push_back(edit(RTX_SHADE_SOLID_COLOR, fs.materials[(size_t)E.b].tex, v.color[1], 3));
    }
    if (mask >> 2 & 1) e.push_back(edit(RTX_SHADE_SOLID_COLOR, B.tex[2], v.color[2], 3));
    for (int k = 0; k < 3; ++k) if (mask >> (7 + k) & 1) e.push_back(edit(RTX_SHADE_MEDIUM_DENSITY, B.slot[k], &v.density[k], 1));
  }
  return e;
}

template <class T>
bool same(const std::vector<T>& a, const std::vector<T>& b) { return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0); }
bool same_arrays(const rtx::FlatScene& a, const rtx::FlatScene& b, const char* what) {
  const rtx::LightTable la = rtx::build_light_table(a), lb = rtx::build_light_table(b);
  const bool ok = same(a.materials, b.materials) && same(a.textures, b.textures) && same(a.entries, b.entries) && same(a.top_level, b.top_level) &&
                  same(a.nodes, b.nodes) && same(a.nodes32, b.nodes32) && same(a.refs, b.refs) && same(a.rects, b.rects) && same(a.spheres, b.spheres) &&
                  same(a.top_box32, b.top_box32) && same(a.perlins, b.perlins) && same(la.lights, lb.lights) && same(la.slot_light, lb.slot_light);
  if (!ok) fprintf(stderr, "%s: the arrays differ\n", what);
  return ok;
}

int check_world(const std::string& name) {
  int bad = 0;
  const Vals rest = rest_vals(), now = new_vals();
  const unsigned all = name == "look" ? 0x7du : 0x386u, masks[] = {all, name == "look" ? 0x01u : 0x80u, name == "look" ? 0x58u : 0x302u};
  for (unsigned mask : masks) {
    Built B, F;
    rtx::FlatScene fs, fresh, first;
    if (!flatten(name, rest, &B, &fs) || !flatten(name, mix(rest, now, mask), &F, &fresh)) return 1;
    first = fs;
    std::string err;
    std::vector<RtxShadingEdit> e = edits_for(B, fs, name, now, mask);
    if (!rtx::flat_set_shading("check", &fs, e.data(), (int64_t)e.size(), &err)) { fprintf(stderr, "%s %x: refused: %s\n", name.c_str(), mask, err.c_str()); return 1; }
    bad += !same_arrays(fs, fresh, (name + " edited").c_str());
    bad += same(fs.materials, first.materials) && same(fs.textures, first.textures) && same(fs.entries, first.entries);  // the edit must show
    // repeated: the same edit again leaves the same bytes; then one at a time, back to rest
    if (!rtx::flat_set_shading("check", &fs, e.data(), (int64_t)e.size(), &err)) return 1;
    bad += !same_arrays(fs, fresh, (name + " edited twice").c_str());
    e = edits_for(B, fs, name, rest, mask);
    for (const RtxShadingEdit& one : e)
      if (!rtx::flat_set_shading("check", &fs, &one, 1, &err)) { fprintf(stderr, "%s: back refused: %s\n", name.c_str(), err.c_str()); return 1; }
    bad += !same_arrays(fs, first, (name + " back at rest").c_str());
  }
  return bad;
}

int check_refusals() {
  int bad = 0;
  Built B;
  rtx::FlatScene fs, first;
  if (!flatten("look", rest_vals(), &B, &fs)) return 1;
  first = fs;
  const double rgb[4] = {0.1, 0.2, 0.3, 0.0}, rgbf[4] = {0.1, 0.2, 0.3, 0.5}, one[1] = {1.5};
  const double nan3[3] = {0.1, std::nan(""), 0.3}, inf1[1] = {HUGE_VAL}, junk[4] = {0.1, 0.2, 0.3, 7.0};
  struct R { std::vector<RtxShadingEdit> e; int64_t n; bool null_edits; const char* word; };
  const RtxShadingEdit good = edit(RTX_SHADE_SOLID_COLOR, B.tex[0], rgb, 3);
  std::vector<R> rs = {
      {{good}, 1, true, "edits is NULL"},
      {{good}, -1, false, "n < 0"},
      {{good, edit(9, 0, rgb, 3)}, 2, false, "edits[1].what"},
      {{edit(-1, 0, rgb, 3)}, 1, false, "edits[0].what"},
      {{edit(RTX_SHADE_SOLID_COLOR, (int32_t)fs.textures.size(), rgb, 3)}, 1, false, "edits[0].index is out of range"},
      {{edit(RTX_SHADE_METAL, -1, rgbf, 4)}, 1, false, "edits[0].index is out of range"},
      {{edit(RTX_SHADE_MEDIUM_DENSITY, (int32_t)fs.top_level.size(), one, 1)}, 1, false, "edits[0].index is out of range"},
      {{edit(RTX_SHADE_METAL, B.lambertian, rgbf, 4)}, 1, false, "edit its texture `tex`"},
      {{edit(RTX_SHADE_SOLID_COLOR, B.checker, rgb, 3)}, 1, false, "Checker"},
      {{edit(RTX_SHADE_NOISE_SCALE, B.tex[0], one, 1)}, 1, false, "not a Noise"},
      {{edit(RTX_SHADE_DIELECTRIC, B.metal[0], one, 1)}, 1, false, "RTX_SHADE_METAL"},
      {{edit(RTX_SHADE_MEDIUM_DENSITY, 0, one, 1)}, 1, false, "not a ConstantMedium"},
      {{good, edit(RTX_SHADE_SOLID_COLOR, B.tex[2], nan3, 3)}, 2, false, "edits[1].v[1] is not finite"},
      {{edit(RTX_SHADE_DIELECTRIC, B.glass, inf1, 1)}, 1, false, "edits[0].v[0] is not finite"},
      {{edit(RTX_SHADE_SOLID_COLOR, B.tex[0], junk, 4)}, 1, false, "edits[0].v[3] is not used"},
      {{good, edit(RTX_SHADE_METAL, B.metal[0], rgbf, 4), good}, 3, false, "twice"},
  };
  for (const R& r : rs) {
    std::string err;
    const bool ok = rtx::flat_set_shading("check", &fs, r.null_edits ? nullptr : r.e.data(), r.n, &err);
    if (ok || err.find(r.word) == std::string::npos || err.find("check: ") != 0) { fprintf(stderr, "refusal '%s': ok %d, message '%s'\n", r.word, (int)ok, err.c_str()); ++bad; }
    bad += !same_arrays(fs, first, r.word);
  }
  std::string err;
  if (rtx::flat_set_shading("check", nullptr, &good, 1, &err) || err.find("scene is NULL") == std::string::npos) { fprintf(stderr, "NULL scene accepted\n"); ++bad; }
  // the ladder's order: an unknown `what` in edit 0 is named before the index of edit 0 and before a NaN in edit 1
  RtxShadingEdit order[2] = {edit(7, -5, nan3, 3), edit(RTX_SHADE_SOLID_COLOR, -1, nan3, 3)};
  if (rtx::flat_set_shading("check", &fs, order, 2, &err) || err.find("edits[0].what") == std::string::npos) { fprintf(stderr, "ladder order: %s\n", err.c_str()); ++bad; }
  order[0] = edit(RTX_SHADE_SOLID_COLOR, -5, nan3, 3);
  if (rtx::flat_set_shading("check", &fs, order, 2, &err) || err.find("edits[0].index") == std::string::npos) { fprintf(stderr, "ladder order: %s\n", err.c_str()); ++bad; }
  order[0] = edit(RTX_SHADE_SOLID_COLOR, B.checker, nan3, 3);
  if (rtx::flat_set_shading("check", &fs, order, 2, &err) || err.find("Checker") == std::string::npos) { fprintf(stderr, "ladder order: %s\n", err.c_str()); ++bad; }
  // a duplicate comes after every per-edit check: edit 2 is not finite
  RtxShadingEdit dup[3] = {good, good, edit(RTX_SHADE_SOLID_COLOR, B.tex[2], nan3, 3)};
  if (rtx::flat_set_shading("check", &fs, dup, 3, &err) || err.find("edits[2].v[1]") == std::string::npos) { fprintf(stderr, "ladder order: %s\n", err.c_str()); ++bad; }
  if (!rtx::flat_set_shading("check", &fs, nullptr, 0, &err)) { fprintf(stderr, "n = 0 refused\n"); ++bad; }
  bad += !same_arrays(fs, first, "after the refusals");
  // a good edit after all the refusals still goes through
  if (!rtx::flat_set_shading("check", &fs, &good, 1, &err) || same(fs.textures, first.textures)) { fprintf(stderr, "a good edit after the refusals failed\n"); ++bad; }
  return bad;
}
}  // namespace

int main() {
  int bad = check_world("look") + check_world("fog") + check_refusals();
  if (bad) { printf("set_shading host check: %d problems\n", bad); return 1; }
  printf("set_shading host check clean\n");
  return 0;
}
