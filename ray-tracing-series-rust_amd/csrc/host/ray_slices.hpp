// The one rule by which a batch of query rays is cut into slices.  Two loops cut a batch: the host
// entries stage RTX_*_HOST_SLICE rays at a time (hip/query_entries.inc) and the launchers send at most 2^30 rays per launch
// (hip/queries.inc).  Both go through here, so a ray of the caller's batch keeps its column rows and its stream however the batch
// was cut, and a slice of a slice is a slice of the batch: slice_of(slice_of(b, f1, c1), f2, c2) is slice_of(b, f1 + f2, c2).
// No HIP, no other header of the project: tests/ray_slices_host_check.cpp compiles it alone.
#pragma once
#include "../../../include/rtx_abi.h"

namespace rtx {

// f(first, count) over [0, n) in order, `per_slice` rays at a time (the last slice takes what is left; n <= 0: no call).
// Stops at the first status that is not RTX_OK and returns it.
template <class F>
inline rtx_status for_ray_slices(int64_t n, int64_t per_slice, F f) {
  for (int64_t first = 0; first < n; first += per_slice) {
    const rtx_status st = f(first, n - first < per_slice ? n - first : per_slice);
    if (st != RTX_OK) return st;
  }
  return RTX_OK;
}

// Row `first` of a [n][width] column; a NULL column (one the caller left out) stays NULL.
template <class T>
inline T* slice_of(T* column, int64_t width, int64_t first) { return column ? column + width * first : nullptr; }

// Rays [first, first + count) of a batch: ray r of the slice keeps the stream seed + (first + r) * stream_step (wrapping).
inline RtxRayBatch slice_of(const RtxRayBatch& b, int64_t first, int64_t count) {
  RtxRayBatch s = b;
  s.n = count;
  s.origin = slice_of(b.origin, 3, first);
  s.direction = slice_of(b.direction, 3, first);
  s.time = slice_of(b.time, 1, first);
  s.t_max = slice_of(b.t_max, 1, first);
  s.seed = b.seed + (uint64_t)first * b.stream_step;
  return s;
}

// The result columns of the rays from `first` on.
inline RtxRayHits slice_of(const RtxRayHits& h, int64_t first) {
  return {slice_of(h.t, 1, first), slice_of(h.p, 3, first), slice_of(h.normal, 3, first), slice_of(h.uv, 2, first),
          slice_of(h.ids, 4, first)};
}

// Rays [first, first + count) of a radiance batch: ray r of the slice keeps the stream key first_ray + first + r.
inline RtxRadianceRays slice_of(const RtxRadianceRays& q, int64_t first, int64_t count) {
  RtxRadianceRays s = q;
  s.n = count;
  s.origin = slice_of(q.origin, 3, first);
  s.direction = slice_of(q.direction, 3, first);
  s.time = slice_of(q.time, 1, first);
  s.first_ray = q.first_ray + (uint64_t)first;
  return s;
}

// Points [first, first + count) of a gather batch: point r of the slice keeps the stream key first_point + first + r.
inline RtxGatherPoints slice_of(const RtxGatherPoints& q, int64_t first, int64_t count) {
  RtxGatherPoints s = q;
  s.n = count;
  s.position = slice_of(q.position, 3, first);
  s.normal = slice_of(q.normal, 3, first);
  s.time = slice_of(q.time, 1, first);
  s.first_point = q.first_point + (uint64_t)first;
  return s;
}

// Points [first, first + count) of a nearest-point batch, and the result columns of the points from `first` on.
inline RtxPointBatch slice_of(const RtxPointBatch& b, int64_t first, int64_t count) {
  RtxPointBatch s = b;
  s.n = count;
  s.points = slice_of(b.points, 3, first);
  s.time = slice_of(b.time, 1, first);
  s.r_max = slice_of(b.r_max, 1, first);
  return s;
}
inline RtxNearest slice_of(const RtxNearest& o, int64_t first) {
  return {slice_of(o.d, 1, first), slice_of(o.q, 3, first), slice_of(o.ids, 4, first)};
}

}  // namespace rtx
