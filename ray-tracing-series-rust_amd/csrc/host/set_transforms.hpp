// rtx_flat_set_transforms on the host, and the part of an update's checking that needs no scene (shared with
// rtx_scene_set_transforms).  Pure host code of the f64 side: abi.cpp and tests/set_transforms_host_check.cpp compile it.
//
// An update replaces the parameters of a slot's Translate / RotateY chain; the result must be the flat scene flatten_scene
// builds from scratch with those parameters, byte for byte where a transform reaches: `entries`, and for every instance tree
// that holds an updated member the boxes in `nodes`, `nodes32` and the static copy in `motion32`.  Topology (child, axis),
// sah_cost and every other array stay as they are.
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>
#include "../core/rt_math.hpp"
#include "f32_layout.hpp"
#include "tree_refit.hpp"
#include "update_shadow.hpp"

namespace rtx {

// NULL, n < 0, and per update: slot < 0, n_ops outside [0, RT_MAX_XFORM_OPS], an op kind that is neither, a value that is not
// finite, a slot named twice.  Looks at nothing but the caller's array.
inline bool check_slot_ops_shape(const char* who, const void* scene, const RtxSlotOps* u, int64_t n, std::string* err) {
  auto bad = [&](int64_t i, const std::string& what) { *err = std::string(who) + ": updates[" + std::to_string(i) + "]" + what; return false; };
  if (!scene) { *err = std::string(who) + ": the scene is NULL"; return false; }
  if (!u) { *err = std::string(who) + ": updates is NULL"; return false; }
  if (n < 0) { *err = std::string(who) + ": n < 0"; return false; }
  for (int64_t i = 0; i < n; ++i) {
    if (u[i].slot < 0) return bad(i, ".slot is out of range (negative)");
    if (u[i].n_ops < 0 || u[i].n_ops > RT_MAX_XFORM_OPS) return bad(i, ".n_ops is not in [0, " + std::to_string(RT_MAX_XFORM_OPS) + "]");
    for (int k = 0; k < u[i].n_ops; ++k) {
      const int32_t op = u[i].ops[k].op;
      if (op != RTX_XFORM_TRANSLATE && op != RTX_XFORM_ROTATE_Y) return bad(i, ".ops[" + std::to_string(k) + "].op is neither RTX_XFORM_TRANSLATE nor RTX_XFORM_ROTATE_Y");
      const int used = op == RTX_XFORM_TRANSLATE ? 3 : 1;
      for (int a = 0; a < used; ++a)
        if (!std::isfinite(u[i].ops[k].v[a])) return bad(i, ".ops[" + std::to_string(k) + "].v[" + std::to_string(a) + "] is not finite");
    }
  }
  std::vector<int32_t> slots((size_t)n);
  for (int64_t i = 0; i < n; ++i) slots[(size_t)i] = u[i].slot;
  std::sort(slots.begin(), slots.end());
  for (size_t i = 1; i < slots.size(); ++i)
    if (slots[i] == slots[i - 1]) { *err = std::string(who) + ": updates name slot " + std::to_string(slots[i]) + " twice (.slot)"; return false; }
  return true;
}

// The caller's ops as the flat arrays hold them: a rotate_y's angle becomes (sin, cos, 0) by SceneGraph::rotate_y's own steps
// (hit.rs:844-846), a translate keeps its offset; pads and the unused ops are zero.
inline std::vector<RtxSlotOps> resolve_slot_ops(const RtxSlotOps* u, int64_t n) {
  std::vector<RtxSlotOps> out((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    RtxSlotOps& r = out[(size_t)i];
    memset(&r, 0, sizeof(r));
    r.slot = u[i].slot;
    r.n_ops = u[i].n_ops;
    for (int k = 0; k < u[i].n_ops; ++k) {
      r.ops[k].op = u[i].ops[k].op;
      if (u[i].ops[k].op == RTX_XFORM_TRANSLATE) {
        for (int a = 0; a < 3; ++a) r.ops[k].v[a] = u[i].ops[k].v[a];
      } else {
        const double angle = rt::rt_to_radians(u[i].ops[k].v[0]);
        r.ops[k].v[0] = rt::rt_sin(angle);
        r.ops[k].v[1] = rt::rt_cos(angle);
      }
    }
  }
  return out;
}

// Instance tree t of fs, refitted bottom-up from the members' local boxes and the ops now in `entries`.
inline void refit_instance_tree(FlatScene* fs, const TreeShadow& t) {
  refit_tree_piece(fs, t.root, t.node_base, t.n_nodes, [&](int32_t code, double* b) {
    const int32_t slot = (int32_t)rt::leaf_first(code);  // a leaf of an instance tree is one member slot
    rt::member_world_box(fs->entries[(size_t)fs->top_level[(size_t)slot]], slot, nullptr,
                         &fs->member_local_box[6 * (size_t)(t.member_first + slot - t.first_slot)], b);
  });
}

// rtx_flat_set_transforms: every check first, then the edit.  false with *err set and *fs untouched.
inline bool flat_set_transforms(const char* who, FlatScene* fs, const RtxSlotOps* updates, int64_t n, std::string* err) {
  if (!check_slot_ops_shape(who, fs, updates, n, err)) return false;
  if (n == 0) return true;
  const std::vector<RtxSlotOps> u = resolve_slot_ops(updates, n);
  const UpdateShadow sh = build_update_shadow(*fs);
  if (!check_slot_ops_scene(who, sh, fs->member_local_box.data(), u.data(), n, err)) return false;
  std::vector<char> touched(sh.trees.size(), 0);
  for (const RtxSlotOps& r : u) {
    const SlotChain& c = sh.slots[(size_t)r.slot];
    rt::FlatEntry& E = fs->entries[(size_t)c.xform];
    for (int k = 0; k < c.n_ops; ++k) { E.ops[k].op = r.ops[k].op; E.ops[k].pad = 0; for (int a = 0; a < 3; ++a) E.ops[k].v[a] = r.ops[k].v[a]; }
    if (c.tree >= 0) touched[(size_t)c.tree] = 1;
  }
  for (size_t k = 0; k < sh.trees.size(); ++k)
    if (touched[k]) refit_instance_tree(fs, sh.trees[k]);
  return true;
}

}  // namespace rtx
