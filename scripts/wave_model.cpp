// A host model of one wave of k_trace_lds (csrc/hip/trace_lds.inc): WHICH LANES ARE ON when each block of the loop runs.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -I include scripts/wave_model.cpp ray-tracing-series-rust_amd/csrc/host/{scene_graph,flatten,bvh_build,scenes}.cpp -o wave_model
//   wave_model <scene id> <width> <aspect> <spp> <depth> <seed> [options]
//
// It builds a catalogue scene through csrc/host, flattens it, and runs waves of 64 lanes through the kernel's loop as it
// stands: the item order of core/item_order.hpp, chunks claimed from one counter, refill of the lanes without a path at the
// loop's top through a ring of ready primary rays, bounce begin with the entry pair of lds_entry_pair (the root for rays
// that are not finite), the cost-weighted node / leaf vote, threshold 1 once nothing can be refilled, carried walks, one
// shading block per outer iteration, and the miss-retire rule.  A path's arithmetic is csrc/core's
// (path_begin, cull32_may_hit, offer_prim, prim_finalize, path_bounce_end), so every sample it produces is the sample the
// product produces (--samples-out writes them, tests/test_wave_model.py compares them with the oracle's bit for bit): a
// policy that loses or repeats a path, or hands a lane another lane's slot, shows here before it is built.
//
// What it does NOT model: the time-aware boxes (a scene with moving spheres is walked through its static boxes, MOTION 0),
// memory and LDS latency, the other fifteen waves of a block, instruction issue.  It counts EXECUTED BLOCKS and prices each
// with a static instruction count of the device assembly (the options below).  The defaults were counted block by block in
// tools/_gen/render_gfx950.s, k_trace_lds<P_STATIC_SPHERES, ring, 0, ShardMap>, the way profiles/step_diet/README.md did:
// node step with latch and vote 84, single-primitive leaf step with them 127, shading block 443 without its rejection loop,
// that loop 51 per attempt (profiles/miss_retire/README.md); the outer head (take + bounce begin, 90) and the ring's top-up
// (251) are step_diet's and item_order's figures.  A wave pays for a block whatever the number of its lanes that are on,
// which is the whole point.
//
// The rejection loop of random_in_unit_sphere (Lambertian and Metal scatter) is NOT counted from the stream: each such hit
// draws its number of attempts from the geometric law with p = pi / 6 (the unit ball's share of the cube) out of a generator
// of the model's own, and a shading round pays for its slowest lane.  Dielectrics draw none.
//
// Options (defaults in brackets):
//   --group P [2]  --chunk N [512]  --ring N [64]  --waves N [16: waves that share the queue, advanced in turn]
//   --walk-threshold N [12]  --leaf-weight N [1]  --retire-done D [0]  --retire-min M [0]
//   --price-node [84] --price-leaf [127] --price-shade [443] --price-attempt [51] --price-outer [90] --price-topup [251]
//   --price-retire [120: a pass of misses only]  --price-skip [25: an outer iteration after a skipped pass, which takes and begins nothing]
//   --retire-step S [0 = D: after a skipped pass the next exit point lies S finished walks further]
//   --samples-out FILE   every sample, 3 doubles at slot (s * npix + j * width + i) * 3
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../ray-tracing-series-rust_amd/csrc/core/integrator.hpp"
#include "../ray-tracing-series-rust_amd/csrc/core/item_order.hpp"
#include "../ray-tracing-series-rust_amd/csrc/host/flat_scene.hpp"
#include "../ray-tracing-series-rust_amd/csrc/host/scenes.hpp"
#define __host__
#define __device__
namespace rtx {
#include "../ray-tracing-series-rust_amd/csrc/hip/lds_layout.inc"
#include "../ray-tracing-series-rust_amd/csrc/hip/lds_variant.inc"
// the GPU builder lives in csrc/hip/lbvh.hip: not part of a host program
int32_t build_bvh_gpu(const std::vector<double>&, int, std::vector<rt::FlatNode>*, std::vector<uint32_t>*, int32_t*, double*, std::string* err) {
  if (err) *err = "no GPU builder in the wave model";
  return -1;
}
}  // namespace rtx

namespace {

constexpr int32_t DONE = -1;  // a walk's item: node index >= 0, the flattener's leaf code < -1, done

struct Options {
  uint32_t group = 2, chunk = 512, ring = 64, waves = 16, walk_threshold = 12, leaf_weight = 1, retire_done = 0, retire_min = 0, retire_step = 0;
  double price_node = 84, price_leaf = 127, price_shade = 443, price_attempt = 51, price_outer = 90, price_topup = 251, price_retire = 120, price_skip = 25;
  const char* samples_out = nullptr;
};

struct Lane {
  bool active = false, midwalk = false;
  uint32_t g = 0;
  rt::PathState ps;
  rt::Ray32 q;
  uint32_t dir_neg = 0;
  float t_max32 = 0.f;
  int32_t cur = DONE;
  rt::Closest best;
  std::vector<int32_t> stack;
};

struct RingEntry { rt::Ray ray; rt::Rng rng; uint32_t g; };

struct Wave {
  Lane lane[64];
  std::vector<RingEntry> ring;  // a stack, as in trace_ring.inc
  uint32_t chunk_pos = 0, chunk_end = 0;
  bool queue_empty = false, finished = false, skipped = false;
};

struct Counters {
  uint64_t outer = 0, outer_lanes = 0, outer_skipped = 0, topups = 0, topup_lanes = 0;
  uint64_t node_steps = 0, node_lanes = 0, leaf_steps = 0, leaf_lanes = 0;
  uint64_t shade_rounds = 0, shade_lanes = 0, shade_hit_lanes = 0, attempts = 0;
  uint64_t retire_passes = 0, retire_lanes = 0, retire_skipped = 0;
  uint64_t rays = 0, node_visits = 0, below_root = 0, root_spares = 0, prim_tests = 0, paths = 0;
};

struct Model {
  const rtx::FlatScene& fs;
  rt::SceneView sv;
  rt::RenderParams rp;
  Options opt;
  rt::ItemOrder order;
  uint32_t total, npix, work_counter = 0;
  int32_t root, entry[2];
  uint32_t first_ref;
  std::vector<double> samples;
  Counters c;
  uint64_t geo_state = 0x9E3779B97F4A7C15ull;

  Model(const rtx::FlatScene& f, const rt::RenderParams& r, const Options& o) : fs(f), sv(f.view()), rp(r), opt(o) {
    npix = (uint32_t)rp.image_width * (uint32_t)rp.image_height;
    total = npix * (uint32_t)rp.samples_per_pixel;
    order = rt::make_item_order(npix, (uint32_t)rp.samples_per_pixel, opt.group);
    const rt::FlatEntry& be = fs.entries[(size_t)fs.top_level[0]];
    root = be.a;
    first_ref = (uint32_t)be.b;
    // lds_entry_pair speaks in LDS items; the model keeps the flattener's codes, so it asks the same question of them
    int32_t items[2];
    rtx::lds_entry_pair(fs.nodes32.data(), root, items);
    const rt::FlatNode32& rn = fs.nodes32[(size_t)root];
    if (rn.axis == 3 && rn.child[0] < 0) { entry[0] = rn.child[0]; entry[1] = rn.child[1]; }
    else { entry[0] = root; entry[1] = DONE; }
    if ((items[1] == LDSK_DONE) != (entry[1] == DONE)) { fprintf(stderr, "entry pair: the model and lds_entry_pair disagree\n"); exit(3); }
    samples.assign((size_t)total * 3, 0.0);
  }

  uint32_t geometric() {  // attempts of one rejection loop: P(n) = (1 - p)^(n - 1) p, p = pi / 6 (splitmix64)
    uint32_t n = 1;
    for (;;) {
      geo_state += 0x9E3779B97F4A7C15ull;
      uint64_t z = geo_state;
      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
      if ((double)(z >> 11) * 0x1.0p-53 < 0.5235987755982988) return n;
      ++n;
    }
  }

  void store(uint32_t g, const rt::Color& v) {
    double* o = &samples[(size_t)g * 3];
    o[0] = v.x; o[1] = v.y; o[2] = v.z;
    ++c.paths;
  }

  // trace_ring.inc: top up at most twice, then the lanes without a path take from the ring's top in rank order
  void refill(Wave& w) {
    uint32_t n_need = 0;
    for (const Lane& l : w.lane) n_need += l.active ? 0u : 1u;
    if (n_need == 0) return;
    for (int rep = 0; rep < 2 && w.ring.size() < n_need && !w.queue_empty; ++rep) {
      if (w.chunk_pos >= w.chunk_end) {
        const uint32_t base = work_counter;
        work_counter += opt.chunk;
        if (base >= total) { w.queue_empty = true; break; }
        w.chunk_pos = base;
        w.chunk_end = (total - base < opt.chunk) ? total : base + opt.chunk;
      }
      const uint32_t room = opt.ring - (uint32_t)w.ring.size(), avail = w.chunk_end - w.chunk_pos;
      const uint32_t m = room < avail ? room : avail;
      for (uint32_t k = 0; k < m; ++k) {
        uint32_t lp, s_local;
        RingEntry e;
        e.g = rt::item_order_map(order, w.chunk_pos + k, &lp, &s_local);
        rt::PathState fresh;
        rt::path_begin(rp, lp % (uint32_t)rp.image_width, lp / (uint32_t)rp.image_width, s_local, &fresh);
        e.ray = fresh.ray; e.rng = fresh.rng;
        w.ring.push_back(e);
      }
      w.chunk_pos += m;
      ++c.topups; c.topup_lanes += m;
    }
    const uint32_t take = n_need < (uint32_t)w.ring.size() ? n_need : (uint32_t)w.ring.size();
    uint32_t rank = 0;
    for (Lane& l : w.lane) {
      if (l.active) continue;
      if (rank < take) {
        const RingEntry& e = w.ring[w.ring.size() - 1u - rank];
        l.ps.ray = e.ray; l.ps.rng = e.rng;
        l.ps.product = rt::v3(1, 1, 1); l.ps.output = rt::v3(0, 0, 0); l.ps.depth = rp.max_depth;
        l.g = e.g;
        l.active = true;
      }
      ++rank;
    }
    w.ring.resize(w.ring.size() - take);
  }

  void bounce_begin(Lane& l) {
    if (rt::path_bounce_begin(&l.ps)) { store(l.g, l.ps.output); l.active = false; return; }
    ++c.rays;
    l.q = rt::make_ray32(l.ps.ray, rt::ray_t_min(l.ps.ray));
    l.dir_neg = rt::ray32_dir_neg(l.q);
    l.t_max32 = __builtin_huge_valf();
    l.best.t = RT_INFINITY; l.best.ref = 0; l.best.order = 0; l.best.hit = false;
    l.stack.clear();
    const float fin = __builtin_fmaf((l.q.oix + l.q.oiy) + l.q.oiz, 0.f, (l.q.ix * l.q.iy) * l.q.iz);
    if (std::isfinite(fin) && fin != 0.f) {
      l.cur = entry[0];
      if (entry[1] != DONE) {
        l.stack.push_back(entry[1]);
        ++c.below_root;
        // (a diagnostic, not a step: would the root have spared this walk child 1's node?  The walk then visits it for nothing.)
        const rt::FlatNode32& rn = fs.nodes32[(size_t)root];
        if (entry[1] >= 0 && !rt::cull32_may_hit(rn.lo[1], rn.hi[1], l.q, l.t_max32)) ++c.root_spares;
      }
    } else {
      l.cur = root;
    }
    l.midwalk = true;
  }

  void node_step(Lane& l) {
    ++c.node_visits;
    const rt::FlatNode32& nd = fs.nodes32[(size_t)l.cur];
    const int first = (int)((l.dir_neg >> (uint32_t)nd.axis) & 1u);
    const bool hf = rt::cull32_may_hit(nd.lo[first], nd.hi[first], l.q, l.t_max32);
    const bool hs = rt::cull32_may_hit(nd.lo[1 - first], nd.hi[1 - first], l.q, l.t_max32);
    const int32_t cf = nd.child[first], cs = nd.child[1 - first];
    if (hf) { l.cur = cf; if (hs) l.stack.push_back(cs); }
    else if (hs) l.cur = cs;
    else pop(l);
  }
  void pop(Lane& l) {
    if (l.stack.empty()) l.cur = DONE;
    else { l.cur = l.stack.back(); l.stack.pop_back(); }
  }
  void leaf_step(Lane& l) {
    const uint32_t f = rt::leaf_first(l.cur), k = rt::leaf_count(l.cur);
    for (uint32_t x = 0; x < k; ++x) {
      ++c.prim_tests;
      rt::offer_prim<rt::F_ALL, false>(sv, fs.refs[(size_t)first_ref + f + x], f + x, l.ps.ray, rt::ray_t_min(l.ps.ray), &l.best, nullptr);
    }
    l.t_max32 = rt::cull_round_up(l.best.t);
    pop(l);
  }

  // one iteration of the kernel's outer loop; false when the wave has left it
  bool outer(Wave& w) {
    refill(w);
    uint32_t n_active = 0;
    for (const Lane& l : w.lane) n_active += l.active ? 1u : 0u;
    if (n_active == 0) return false;
    if (w.skipped) ++c.outer_skipped; else { ++c.outer; c.outer_lanes += n_active; }
    for (Lane& l : w.lane) if (l.active && !l.midwalk) bounce_begin(l);
    const bool no_refill = w.queue_empty && w.ring.empty();
    const uint32_t threshold = no_refill ? 1u : opt.walk_threshold;
    auto count = [&](uint32_t* n_node, uint32_t* n_leaf) {
      *n_node = *n_leaf = 0;
      for (const Lane& l : w.lane) { if (l.cur >= 0) ++*n_node; else if (l.cur < -1) ++*n_leaf; }
    };
    uint32_t n_node, n_leaf;
    count(&n_node, &n_leaf);
    const bool retire_on = opt.retire_done != 0 && opt.ring != 0 && !no_refill;
    int32_t exit_at = (int32_t)threshold;
    const int32_t further = (int32_t)(w.skipped && opt.retire_step ? opt.retire_step : opt.retire_done);
    w.skipped = false;
    if (retire_on && (int32_t)(n_node + n_leaf) - further > exit_at) exit_at = (int32_t)(n_node + n_leaf) - further;
    while (n_node + n_leaf >= (uint32_t)exit_at) {
      if (n_node * opt.leaf_weight >= n_leaf) {
        ++c.node_steps; c.node_lanes += n_node;
        for (Lane& l : w.lane) if (l.cur >= 0) node_step(l);
      } else {
        ++c.leaf_steps; c.leaf_lanes += n_leaf;
        for (Lane& l : w.lane) if (l.cur < -1) leaf_step(l);
      }
      count(&n_node, &n_leaf);
    }
    const bool round_over = !retire_on || n_node + n_leaf < threshold;
    bool shade[64];
    uint32_t n_shade = 0;
    for (int k = 0; k < 64; ++k) {
      const Lane& l = w.lane[k];
      shade[k] = l.midwalk && l.cur == DONE && (round_over || !l.best.hit);
      n_shade += shade[k] ? 1u : 0u;
    }
    if (!round_over && n_shade < opt.retire_min) { ++c.retire_skipped; w.skipped = true; return true; }
    uint32_t n_hit = 0, slowest = 0;
    for (int k = 0; k < 64; ++k) {
      if (!shade[k]) continue;
      Lane& l = w.lane[k];
      l.midwalk = false;
      rt::HitRecord rec;
      const bool hit = l.best.hit;
      if (hit) {
        ++n_hit;
        rt::prim_finalize<rt::F_ALL>(sv, l.best.ref, l.ps.ray, l.best.t, &rec);
        const int32_t kind = fs.materials[(size_t)rec.mat].kind;
        if (kind == rt::MAT_LAMBERTIAN || kind == rt::MAT_METAL) { const uint32_t a = geometric(); if (a > slowest) slowest = a; }
      }
      if (rt::path_bounce_end<rt::F_ALL, false>(sv, rp, &l.ps, hit, rec, nullptr)) { store(l.g, l.ps.output); l.active = false; }
    }
    if (n_shade != 0 && round_over) { ++c.shade_rounds; c.shade_lanes += n_shade; c.shade_hit_lanes += n_hit; c.attempts += slowest; }
    else if (n_shade != 0) { ++c.retire_passes; c.retire_lanes += n_shade; }
    return true;
  }

  void run() {
    std::vector<Wave> waves(opt.waves);
    for (bool any = true; any;) {
      any = false;
      for (Wave& w : waves) {
        if (w.finished) continue;
        if (outer(w)) any = true; else w.finished = true;
      }
    }
  }
};

double mean(uint64_t lanes, uint64_t n) { return n ? (double)lanes / (double)n : 0.0; }

}  // namespace

int main(int argc, char** argv) {
  if (argc < 7) { fprintf(stderr, "usage: wave_model <scene id> <width> <aspect> <spp> <depth> <seed> [options: see the head of the file]\n"); return 2; }
  const int32_t sid = atoi(argv[1]), width = atoi(argv[2]), spp = atoi(argv[4]), depth = atoi(argv[5]);
  const double aspect = atof(argv[3]);
  const uint64_t seed = strtoull(argv[6], nullptr, 0);
  Options opt;
  for (int k = 7; k + 1 < argc; k += 2) {
    const std::string o = argv[k];
    const char* v = argv[k + 1];
    if (o == "--group") opt.group = (uint32_t)strtoul(v, nullptr, 0);
    else if (o == "--chunk") opt.chunk = (uint32_t)atoi(v);
    else if (o == "--ring") opt.ring = (uint32_t)atoi(v);
    else if (o == "--waves") opt.waves = (uint32_t)atoi(v);
    else if (o == "--walk-threshold") opt.walk_threshold = (uint32_t)atoi(v);
    else if (o == "--leaf-weight") opt.leaf_weight = (uint32_t)atoi(v);
    else if (o == "--retire-done") opt.retire_done = (uint32_t)atoi(v);
    else if (o == "--retire-min") opt.retire_min = (uint32_t)atoi(v);
    else if (o == "--price-node") opt.price_node = atof(v);
    else if (o == "--price-leaf") opt.price_leaf = atof(v);
    else if (o == "--price-shade") opt.price_shade = atof(v);
    else if (o == "--price-attempt") opt.price_attempt = atof(v);
    else if (o == "--price-outer") opt.price_outer = atof(v);
    else if (o == "--price-topup") opt.price_topup = atof(v);
    else if (o == "--price-retire") opt.price_retire = atof(v);
    else if (o == "--price-skip") opt.price_skip = atof(v);
    else if (o == "--retire-step") opt.retire_step = (uint32_t)atoi(v);
    else if (o == "--samples-out") opt.samples_out = v;
    else { fprintf(stderr, "unknown option %s\n", o.c_str()); return 2; }
  }
  if (width <= 0 || spp <= 0 || depth <= 0 || !(aspect > 0.0) || opt.group < 1 || opt.group > rt::ITEM_GROUP_MAX || opt.chunk < 64 ||
      opt.ring < 1 || opt.ring > 64 || opt.waves < 1 || opt.walk_threshold < 1 || opt.walk_threshold > 64 || opt.leaf_weight < 1 ||
      opt.retire_done > 64 || opt.retire_min > 64 || opt.retire_step > 64) { fprintf(stderr, "an argument is out of range\n"); return 2; }
  rtx::SceneGraph g(1);
  rtx::SceneOptions so;
  rtx::WorldCam wc;
  std::string err;
  if (!rtx::get_world_cam(g, sid, so, &wc, &err)) { fprintf(stderr, "scene %d: %s\n", sid, err.c_str()); return 1; }
  rtx::BuildOptions bo;
  rtx::FlatScene fs;
  if (!rtx::flatten_scene(g, wc.world, bo, &fs, &err)) { fprintf(stderr, "scene %d: flatten: %s\n", sid, err.c_str()); return 1; }
  if (fs.top_level.size() != 1 || fs.entries[(size_t)fs.top_level[0]].kind != rt::ENTRY_BVH || fs.entries[(size_t)fs.top_level[0]].a < 0) {
    fprintf(stderr, "scene %d is not one BVH of spheres: k_trace_lds does not run it\n", sid);
    return 1;
  }
  rt::RenderParams rp;
  rp.cam = wc.cam;
  rp.background = rt::v3(wc.background[0], wc.background[1], wc.background[2]);
  rp.image_width = width;
  rp.image_height = rt::rt_f64_as_i32((double)width / aspect);
  rp.samples_per_pixel = spp;
  rp.max_depth = depth;
  rp.seed = seed;
  if (rp.image_height <= 0 || (uint64_t)width * (uint64_t)rp.image_height * (uint64_t)spp >= (1ull << 32)) { fprintf(stderr, "frame out of range\n"); return 2; }
  Model m(fs, rp, opt);
  m.run();
  const Counters& c = m.c;
  if (c.paths != m.total) { fprintf(stderr, "%llu paths stored, %u items\n", (unsigned long long)c.paths, m.total); return 4; }
  if (opt.samples_out) {
    FILE* f = fopen(opt.samples_out, "wb");
    if (!f || fwrite(m.samples.data(), sizeof(double), m.samples.size(), f) != m.samples.size()) { fprintf(stderr, "cannot write %s\n", opt.samples_out); return 1; }
    fclose(f);
  }
  const double priced = (double)c.node_steps * opt.price_node + (double)c.leaf_steps * opt.price_leaf + (double)c.shade_rounds * opt.price_shade +
                        (double)c.attempts * opt.price_attempt + (double)c.outer * opt.price_outer + (double)c.topups * opt.price_topup +
                        (double)c.retire_passes * opt.price_retire + (double)c.outer_skipped * opt.price_skip;
  printf("frame %d x %d x %d spp, depth %d, seed %llu; group %u chunk %u ring %u waves %u; walk_threshold %u leaf_weight %u retire %u / %u\n",
         width, rp.image_height, spp, depth, (unsigned long long)seed, opt.group, opt.chunk, opt.ring, opt.waves, opt.walk_threshold,
         opt.leaf_weight, opt.retire_done, opt.retire_min);
  printf("paths %llu\nrays %llu\nnode_visits %llu\nwalks_below_root %llu\nroot_would_spare_child1 %llu\nprim_tests %llu\n", (unsigned long long)c.paths,
         (unsigned long long)c.rays, (unsigned long long)c.node_visits, (unsigned long long)c.below_root, (unsigned long long)c.root_spares,
         (unsigned long long)c.prim_tests);
  printf("node_steps %llu mean_lanes %.2f\nleaf_steps %llu mean_lanes %.2f\n", (unsigned long long)c.node_steps, mean(c.node_lanes, c.node_steps),
         (unsigned long long)c.leaf_steps, mean(c.leaf_lanes, c.leaf_steps));
  printf("shade_rounds %llu mean_lanes %.2f mean_hit_lanes %.2f attempts %llu\n", (unsigned long long)c.shade_rounds, mean(c.shade_lanes, c.shade_rounds),
         mean(c.shade_hit_lanes, c.shade_rounds), (unsigned long long)c.attempts);
  printf("outer_iterations_after_a_skip %llu\n", (unsigned long long)c.outer_skipped);
  printf("outer_iterations %llu mean_lanes %.2f\nring_topups %llu mean_lanes %.2f\n", (unsigned long long)c.outer, mean(c.outer_lanes, c.outer),
         (unsigned long long)c.topups, mean(c.topup_lanes, c.topups));
  printf("retire_passes %llu mean_lanes %.2f skipped %llu\n", (unsigned long long)c.retire_passes, mean(c.retire_lanes, c.retire_passes),
         (unsigned long long)c.retire_skipped);
  printf("rays_per_path %.4f\nnode_visits_per_ray %.4f\n", (double)c.rays / (double)c.paths, (double)c.node_visits / (double)c.rays);
  printf("priced_instructions %.0f\npriced_per_path %.3f\n", priced, priced / (double)c.paths);
  return 0;
}
