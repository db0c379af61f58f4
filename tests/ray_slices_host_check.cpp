// csrc/host/ray_slices.hpp swept on the host: the one rule by which the ray queries cut a batch, into staging slices by the host
// entries and into launch slices by the launchers.  Columns are address arithmetic on fake non-NULL bases -- nothing is
// dereferenced, so 2^31 rays need no memory.  Checked for slice lengths S in {1, 4, 5} and n in {0, 1, S-1, S, S+1, 2S, 2S+1}:
//   * the slices tile [0, n) in order, none empty; n = 0 makes no call; a status other than RTX_OK stops the loop and is returned;
//   * every non-NULL column of a slice is base + width * first (3, 3, 1, 1 for a batch, 1, 3, 3, 2, 4 for the hits), NULL stays NULL,
//     seed is seed0 + first * stream_step in wrapping 64-bit arithmetic, first_ray is first_ray0 + first, n is the count, and every
//     other field keeps its bits;
//   * nesting: cutting with S_host and then with S_launch inside gives every ray the address and stream that cutting [0, n)
//     directly gives -- what makes a host entry and a device entry agree;
//   * 2^31 + 3 rays in launch slices of 2^30 start at 0, 2^30 and 2^31, the last of 3 rays.
// Stand-alone: g++ -std=c++17 tests/ray_slices_host_check.cpp && ./a.out
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../ray-tracing-series-rust_amd/csrc/host/ray_slices.hpp"

static long long failures = 0, checks = 0;
#define CHECK(cond)                                                                                   \
  do {                                                                                                \
    ++checks;                                                                                         \
    if (!(cond) && failures++ < 20) std::printf("FAILED line %d: %s (%s)\n", __LINE__, #cond, what); \
  } while (0)

struct Slice { int64_t first, count; };

template <class T>
static T* fake(uintptr_t address) { return (T*)address; }
static uintptr_t at(const void* p) { return (uintptr_t)p; }
// where row `first` of a [n][width] column of T lies, by plain integer arithmetic
template <class T>
static uintptr_t row(const T* base, int64_t width, int64_t first) {
  return base ? at(base) + (uintptr_t)sizeof(T) * (uintptr_t)width * (uintptr_t)first : 0;
}

static RtxRayBatch make_batch(int64_t n, bool optional, uint64_t stream_step) {
  RtxRayBatch b;
  std::memset(&b, 0x5a, sizeof(b));
  b.n = n;
  b.origin = fake<const double>(0x10000000);
  b.direction = fake<const double>(0x20000008);
  b.time = optional ? fake<const double>(0x30000010) : nullptr;
  b.t_max = optional ? fake<const double>(0x40000018) : nullptr;
  b.t_min = 0.001;
  b.t_max_all = 1e30;
  b.seed = 0xfffffffffffffff0ull;  // first * stream_step wraps past 2^64 at once
  b.stream_step = stream_step;
  return b;
}
static RtxRayHits make_hits(bool optional) {
  if (!optional) return {nullptr, nullptr, nullptr, nullptr, nullptr};
  return {fake<double>(0x50000000), fake<double>(0x60000008), fake<double>(0x70000010), fake<double>(0x80000020), fake<int32_t>(0x90000030)};
}
static RtxRadianceRays make_radiance(int64_t n, bool optional) {
  RtxRadianceRays q;
  std::memset(&q, 0xa5, sizeof(q));
  q.n = n;
  q.origin = fake<const double>(0x10000000);
  q.direction = fake<const double>(0x20000008);
  q.time = optional ? fake<const double>(0x30000010) : nullptr;
  q.first_ray = 0xffffffffffffff00ull;
  return q;
}

static void check_batch_slice(const char* what, const RtxRayBatch& b, const RtxRayBatch& s, int64_t first, int64_t count) {
  CHECK(s.n == count);
  CHECK(at(s.origin) == row(b.origin, 3, first) && at(s.direction) == row(b.direction, 3, first));
  CHECK(at(s.time) == row(b.time, 1, first) && at(s.t_max) == row(b.t_max, 1, first));
  CHECK(s.seed == b.seed + (uint64_t)first * b.stream_step);
  RtxRayBatch rest = s;  // every other field: the original's bits
  rest.n = b.n; rest.origin = b.origin; rest.direction = b.direction; rest.time = b.time; rest.t_max = b.t_max; rest.seed = b.seed;
  CHECK(std::memcmp(&rest, &b, sizeof(b)) == 0);
}
static void check_hits_slice(const char* what, const RtxRayHits& h, const RtxRayHits& s, int64_t first) {
  CHECK(at(s.t) == row(h.t, 1, first) && at(s.p) == row(h.p, 3, first) && at(s.normal) == row(h.normal, 3, first));
  CHECK(at(s.uv) == row(h.uv, 2, first) && at(s.ids) == row(h.ids, 4, first));
}
static void check_radiance_slice(const char* what, const RtxRadianceRays& q, const RtxRadianceRays& s, int64_t first, int64_t count) {
  CHECK(s.n == count);
  CHECK(at(s.origin) == row(q.origin, 3, first) && at(s.direction) == row(q.direction, 3, first) && at(s.time) == row(q.time, 1, first));
  CHECK(s.first_ray == q.first_ray + (uint64_t)first);
  RtxRadianceRays rest = s;
  rest.n = q.n; rest.origin = q.origin; rest.direction = q.direction; rest.time = q.time; rest.first_ray = q.first_ray;
  CHECK(std::memcmp(&rest, &q, sizeof(q)) == 0);
}

static std::vector<Slice> slices_of(int64_t n, int64_t per_slice) {
  std::vector<Slice> v;
  const rtx_status st = rtx::for_ray_slices(n, per_slice, [&](int64_t first, int64_t count) {
    v.push_back({first, count});
    return (rtx_status)RTX_OK;
  });
  const char* what = "for_ray_slices";
  CHECK(st == RTX_OK);
  return v;
}

static const uint64_t STEPS[] = {0ull, 1ull, (1ull << 63) + 1ull};

int main() {
  const int64_t lengths[] = {1, 4, 5};
  for (int64_t S : lengths) {
    const int64_t ns[] = {0, 1, S - 1, S, S + 1, 2 * S, 2 * S + 1};
    for (int64_t n : ns) {
      char what[96];
      std::snprintf(what, sizeof(what), "S %lld n %lld", (long long)S, (long long)n);
      // ---- tiling
      const std::vector<Slice> v = slices_of(n, S);
      CHECK((int64_t)v.size() == (n + S - 1) / S);
      int64_t next = 0;
      for (const Slice& s : v) {
        CHECK(s.first == next && s.count >= 1 && s.count <= S);
        next = s.first + s.count;
      }
      CHECK(next == n);
      // ---- a refusing callback: call k answers RTX_EINVAL, nothing is called after it
      for (size_t k = 0; k < v.size(); ++k) {
        size_t calls = 0;
        const rtx_status st = rtx::for_ray_slices(n, S, [&](int64_t, int64_t) { return calls++ == k ? (rtx_status)RTX_EINVAL : (rtx_status)RTX_OK; });
        CHECK(st == RTX_EINVAL && calls == k + 1);
      }
      // ---- the three structs and the bare column, optional columns all NULL / all set
      for (int optional = 0; optional < 2; ++optional) {
        const RtxRayHits h = make_hits(optional != 0);
        const RtxRadianceRays q = make_radiance(n, optional != 0);
        for (const Slice& s : v) {
          for (uint64_t step : STEPS) {
            const RtxRayBatch b = make_batch(n, optional != 0, step);
            check_batch_slice(what, b, rtx::slice_of(b, s.first, s.count), s.first, s.count);
          }
          check_hits_slice(what, h, rtx::slice_of(h, s.first), s.first);
          check_radiance_slice(what, q, rtx::slice_of(q, s.first, s.count), s.first, s.count);
          CHECK(at(rtx::slice_of(h.p, 3, s.first)) == row(h.p, 3, s.first));
          CHECK(at(rtx::slice_of(h.ids, 4, s.first)) == row(h.ids, 4, s.first));
        }
      }
      // ---- nesting: staging slices of S, launch slices of L inside them, against the direct rule ray by ray
      for (int64_t L : lengths)
        for (uint64_t step : STEPS) {
          const RtxRayBatch b = make_batch(n, true, step);
          const RtxRayHits h = make_hits(true);
          const RtxRadianceRays q = make_radiance(n, true);
          int64_t rays = 0;
          for (const Slice& hs : v) {
            const RtxRayBatch b1 = rtx::slice_of(b, hs.first, hs.count);
            const RtxRayHits h1 = rtx::slice_of(h, hs.first);
            const RtxRadianceRays q1 = rtx::slice_of(q, hs.first, hs.count);
            for (const Slice& ls : slices_of(hs.count, L)) {
              const RtxRayBatch b2 = rtx::slice_of(b1, ls.first, ls.count);
              const RtxRayHits h2 = rtx::slice_of(h1, ls.first);
              const RtxRadianceRays q2 = rtx::slice_of(q1, ls.first, ls.count);
              for (int64_t r = 0; r < ls.count; ++r, ++rays) {  // ray r of the launch is ray g of the caller's batch
                const int64_t g = hs.first + ls.first + r;
                CHECK(row(b2.origin, 3, r) == row(b.origin, 3, g) && row(b2.direction, 3, r) == row(b.direction, 3, g));
                CHECK(row(b2.time, 1, r) == row(b.time, 1, g) && row(b2.t_max, 1, r) == row(b.t_max, 1, g));
                CHECK(b2.seed + (uint64_t)r * b2.stream_step == b.seed + (uint64_t)g * b.stream_step);
                CHECK(row(h2.t, 1, r) == row(h.t, 1, g) && row(h2.p, 3, r) == row(h.p, 3, g) && row(h2.normal, 3, r) == row(h.normal, 3, g));
                CHECK(row(h2.uv, 2, r) == row(h.uv, 2, g) && row(h2.ids, 4, r) == row(h.ids, 4, g));
                CHECK(row(q2.origin, 3, r) == row(q.origin, 3, g) && row(q2.direction, 3, r) == row(q.direction, 3, g) &&
                      row(q2.time, 1, r) == row(q.time, 1, g));
                CHECK(q2.first_ray + (uint64_t)r == q.first_ray + (uint64_t)g);
              }
            }
          }
          CHECK(rays == n);
        }
    }
  }
  // ---- past 2^31 rays: the launch slices of the largest batch a caller can address in 32 bits and a little more
  {
    const char* what = "2^31 + 3 rays";
    const int64_t n = ((int64_t)1 << 31) + 3, per = (int64_t)1 << 30;
    const std::vector<Slice> v = slices_of(n, per);
    CHECK(v.size() == 3);
    if (v.size() == 3) {
      CHECK(v[0].first == 0 && v[1].first == per && v[2].first == 2 * per);
      CHECK(v[0].count == per && v[1].count == per && v[2].count == 3);
      const RtxRayBatch b = make_batch(n, true, (1ull << 63) + 1ull);
      const RtxRayHits h = make_hits(true);
      const RtxRadianceRays q = make_radiance(n, true);
      for (const Slice& s : v) {
        check_batch_slice(what, b, rtx::slice_of(b, s.first, s.count), s.first, s.count);
        check_hits_slice(what, h, rtx::slice_of(h, s.first), s.first);
        check_radiance_slice(what, q, rtx::slice_of(q, s.first, s.count), s.first, s.count);
      }
    }
  }
  if (failures) {
    std::printf("ray slices host check: %lld of %lld checks FAILED\n", failures, checks);
    return 1;
  }
  std::printf("ray slices host check clean: %lld checks\n", checks);
  return 0;
}
