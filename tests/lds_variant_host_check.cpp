// csrc/hip/lds_variant.inc on the host: the launcher's choice of k_trace_lds instantiation, asked row by row.
//   lds_variant_host_check variant <time_boxes> <bvh_t0> <bvh_t1> <shutter1> <shutter2> <motion_axis> <mv_common>  -> the variant word
//   lds_variant_host_check common <time0> <time1> [<time0> <time1> ...]  -> "1 t0 t1" or "0"
//   lds_variant_host_check records <features> <static_preset> <n_static> <max_end>  -> "moving n_spheres n_moving n_uni"
// Stand-alone: g++ tests/lds_variant_host_check.cpp && ./a.out variant 1 0 1 0 1 -1 1
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace rtx {
#include "../ray-tracing-series-rust_amd/csrc/hip/lds_variant.inc"
}

struct Interval { double time0, time1; };
struct IntervalF { float time0, time1; };  // the f32 compilation's records

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "variant") && argc == 9) {
    std::printf("%d\n", (int)rtx::lds_trace_variant(atoi(argv[2]) != 0, strtod(argv[3], nullptr), strtod(argv[4], nullptr), strtod(argv[5], nullptr),
                                                    strtod(argv[6], nullptr), atoi(argv[7]), atoi(argv[8]) != 0));
    return 0;
  }
  if (argc >= 2 && !strcmp(argv[1], "common") && argc % 2 == 0) {
    std::vector<Interval> v;
    std::vector<IntervalF> vf;
    for (int k = 2; k + 1 < argc; k += 2) {
      v.push_back({strtod(argv[k], nullptr), strtod(argv[k + 1], nullptr)});
      vf.push_back({(float)v.back().time0, (float)v.back().time1});
    }
    double t0 = 0.0, t1 = 0.0, f0 = 0.0, f1 = 0.0;
    const bool same = rtx::lds_common_interval(v.data(), v.size(), &t0, &t1);
    const bool same_f = rtx::lds_common_interval(vf.data(), vf.size(), &f0, &f1);
    if (same != same_f) { std::printf("the f64 and f32 records disagree\n"); return 1; }
    if (same) std::printf("1 %.17g %.17g\n", t0, t1);
    else std::printf("0\n");
    return 0;
  }
  if (argc == 6 && !strcmp(argv[1], "records")) {
    uint32_t out[3];
    const uint32_t f = (uint32_t)strtoul(argv[2], nullptr, 0), preset = (uint32_t)strtoul(argv[3], nullptr, 0);
    rtx::lds_record_counts(f, preset, (uint32_t)strtoul(argv[4], nullptr, 0), (uint32_t)strtoul(argv[5], nullptr, 0), out);
    std::printf("%d %u %u %u\n", rtx::lds_records_are_moving(f, preset) ? 1 : 0, out[0], out[1], out[2]);
    return 0;
  }
  std::fprintf(stderr, "usage: see the head of tests/lds_variant_host_check.cpp\n");
  return 2;
}
