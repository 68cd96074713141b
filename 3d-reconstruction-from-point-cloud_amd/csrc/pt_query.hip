// pt_query.hip -- the small kernels around the k-NN search, for gfx950 (MI355X): merge of candidate lists (slab exchange, streamed
// chunks), the streamed-chunk sweep, slab-need / request packing, compaction of the group kernel's marks, bound capping.  The search
// kernels themselves are in pt_knn_group.hip, pt_knn_wave.hip and pt_knn_tile.hip.
#include "pt_knn_common.h"

using namespace pt_knn;

namespace {

// ---- G-way merge of candidate lists under (d2, idx): one thread per (target, list slot) --------------
__global__ __launch_bounds__(WG) void merge_kernel(const uint32_t* __restrict__ idx_lists, const double* __restrict__ d2_lists, int g,
                                                   uint32_t m, int k, uint32_t* __restrict__ idx_out, double* __restrict__ d2_out) {
  const int per = g * k;
  const uint64_t gt = (uint64_t)blockIdx.x * WG + threadIdx.x;
  const uint32_t t = (uint32_t)(gt / (uint64_t)per);
  if (t >= m) return;
  const int slot = (int)(gt % (uint64_t)per);
  const int mg = slot / k, mj = slot % k;
  const size_t mo = ((size_t)mg * m + t) * (size_t)k + (size_t)mj;
  const uint32_t myi = idx_lists[mo];
  const double myd = d2_lists[mo];
  int rank = 0, cnt = 0;
  for (int r = 0; r < g; ++r)
    for (int j = 0; j < k; ++j) {
      const size_t o = ((size_t)r * m + t) * (size_t)k + (size_t)j;
      const uint32_t oi = idx_lists[o];
      if (oi == PT_NOIDX_U) continue;
      ++cnt;
      const double od = d2_lists[o];
      if (key_lt(od, oi, myd, myi) || (od == myd && oi == myi && (r * k + j) < slot)) ++rank;
    }
  if (myi != PT_NOIDX_U && rank < k) { idx_out[(size_t)t * k + rank] = myi; d2_out[(size_t)t * k + rank] = myd; }
  if (slot < k && slot >= cnt) { idx_out[(size_t)t * k + slot] = PT_NOIDX_U; d2_out[(size_t)t * k + slot] = INFINITY; }
}

// ---- running merge of a streamed source (pt_stream_query): the k best so far (64-bit ids) with the k of the chunk just searched
// (32-bit chunk-local ids + the chunk's first id), both ascending under (d2, id); one thread per target, out-of-place
__global__ __launch_bounds__(WG) void merge_stream_kernel(const unsigned long long* __restrict__ bi, const double* __restrict__ bd,
                                                          const uint32_t* __restrict__ ci, const double* __restrict__ cd, unsigned long long base,
                                                          uint32_t m, int k, unsigned long long* __restrict__ oi, double* __restrict__ od) {
  const uint32_t t = blockIdx.x * WG + threadIdx.x;
  if (t >= m) return;
  const size_t row = (size_t)t * (size_t)k;
  int a = 0, b = 0;
  for (int o = 0; o < k; ++o) {
    const bool ha = a < k && bi[row + a] != ~0ull, hb = b < k && ci[row + b] != PT_NOIDX_U;
    unsigned long long ia = ~0ull, ib = ~0ull;
    double da = INFINITY, db = INFINITY;
    if (ha) { ia = bi[row + a]; da = bd[row + a]; }
    if (hb) { ib = base + (unsigned long long)ci[row + b]; db = cd[row + b]; }
    const bool take_a = ha && (!hb || da < db || (da == db && ia < ib));
    if (take_a) { oi[row + o] = ia; od[row + o] = da; ++a; }
    else if (hb) { oi[row + o] = ib; od[row + o] = db; ++b; }
    else { oi[row + o] = ~0ull; od[row + o] = INFINITY; }
  }
}

// ---- which other slabs can still hold one of a target's k nearest (reference Distance.h:27-57 on slab boxes)
template <class T>
__global__ __launch_bounds__(WG) void slab_need_kernel(const T* __restrict__ x, const T* __restrict__ y, const T* __restrict__ z,
                                                       const double* __restrict__ d2, uint32_t m, int k, int axis,
                                                       const double* __restrict__ bounds, int g, int my_slab, double cap2, uint8_t* __restrict__ need) {
  const uint32_t t = blockIdx.x * WG + threadIdx.x;
  if (t >= m) return;
  const double c = (double)(axis == 0 ? x[t] : (axis == 1 ? y[t] : z[t]));
  const double kth = pt_reach2(d2[(size_t)t * k + (k - 1)], cap2);
  for (int s = 0; s < g; ++s) {
    uint8_t v = 0;
    if (s != my_slab) {
      const double lo = bounds[s], hi = bounds[s + 1];
      const double gapd = c < lo ? lo - c : (c >= hi ? c - hi : 0.0);
      v = (gapd * gapd * (1.0 - 1e-12) <= kth) ? 1 : 0;     // `<=`: an equal-distance lower-index point would win the tie
    }
    need[(size_t)s * m + t] = v;
  }
}

// slab_need + compaction in one pass: the targets that need another slab leave as request packets
// {x, y, z, current k-th d2, bitmask of the slabs asked} (5 doubles) with their row in `sel`; *count is the number written
// (order unspecified: whoever reserves a slot first).  The bitmask is exact in a double for g <= 52.
template <class T>
__global__ __launch_bounds__(WG) void request_pack_kernel(const T* __restrict__ x, const T* __restrict__ y, const T* __restrict__ z,
                                                          const double* __restrict__ d2, uint32_t m, int k, int axis,
                                                          const double* __restrict__ bounds, int g, int my_slab, double cap2, uint32_t* __restrict__ count,
                                                          uint32_t* __restrict__ sel, double* __restrict__ pkt) {
  const uint32_t t = blockIdx.x * WG + threadIdx.x;
  if (t >= m) return;
  const double c = (double)(axis == 0 ? x[t] : (axis == 1 ? y[t] : z[t]));
  const double kth = pt_reach2(d2[(size_t)t * k + (k - 1)], cap2);
  uint64_t mask = 0;
  for (int s = 0; s < g; ++s) {
    if (s == my_slab) continue;
    const double lo = bounds[s], hi = bounds[s + 1];
    const double gapd = c < lo ? lo - c : (c >= hi ? c - hi : 0.0);
    if (gapd * gapd * (1.0 - 1e-12) <= kth) mask |= 1ull << s;       // same test as slab_need_kernel
  }
  if (!mask) return;
  const uint32_t pos = atomicAdd(count, 1u);                         // (folded into one atomic per wave)
  sel[pos] = t;
  double* o = pkt + (size_t)pos * 5;
  o[0] = (double)x[t]; o[1] = (double)y[t]; o[2] = (double)z[t]; o[3] = kth; o[4] = (double)mask;
}

}  // namespace

template <class T>
void pt_launch_request_pack(const T* x, const T* y, const T* z, const double* d2, uint32_t m, int k, int axis, const double* bounds_dev, int g,
                            int my_slab, double cap2, uint32_t* count, uint32_t* sel, double* pkt, hipStream_t s) {
  if (!m) return;
  hipLaunchKernelGGL(request_pack_kernel<T>, dim3((m + WG - 1) / WG), dim3(WG), 0, s, x, y, z, d2, m, k, axis, bounds_dev, g, my_slab, cap2, count, sel, pkt);
}
template void pt_launch_request_pack<float>(const float*, const float*, const float*, const double*, uint32_t, int, int, const double*, int, int, double,
                                            uint32_t*, uint32_t*, double*, hipStream_t);
template void pt_launch_request_pack<double>(const double*, const double*, const double*, const double*, uint32_t, int, int, const double*, int, int,
                                             double, uint32_t*, uint32_t*, double*, hipStream_t);

// ---- the marks of the group kernel, compacted in order: positions with mark 1 to list1, with mark 2 to list2 ----------------------
constexpr int CP_ITEMS = 8, CP_TILE = WG * CP_ITEMS;
__global__ __launch_bounds__(WG) void mark_count_kernel(const uint8_t* __restrict__ mark, uint32_t m, uint32_t* __restrict__ c1, uint32_t* __restrict__ c2) {
  __shared__ uint32_t wsum[4];
  uint32_t a = 0, b = 0;
#pragma unroll
  for (int i = 0; i < CP_ITEMS; ++i) {
    const uint32_t t = blockIdx.x * CP_TILE + threadIdx.x * CP_ITEMS + i;
    const uint32_t v = t < m ? mark[t] : 0u;
    a += v == 1u; b += v == 2u;
  }
  uint32_t ta, tb;
  block_excl_scan(a, wsum, ta);
  __syncthreads();
  block_excl_scan(b, wsum, tb);
  if (threadIdx.x == 0) { c1[blockIdx.x] = ta; c2[blockIdx.x] = tb; }
}
__global__ __launch_bounds__(WG) void mark_write_kernel(const uint8_t* __restrict__ mark, uint32_t m, const uint32_t* __restrict__ o1, const uint32_t* __restrict__ o2,
                                                        uint32_t* __restrict__ list1, uint32_t* __restrict__ list2) {
  __shared__ uint32_t wsum[4];
  uint32_t v[CP_ITEMS], a = 0, b = 0;
#pragma unroll
  for (int i = 0; i < CP_ITEMS; ++i) {
    const uint32_t t = blockIdx.x * CP_TILE + threadIdx.x * CP_ITEMS + i;
    v[i] = t < m ? mark[t] : 0u;
    a += v[i] == 1u; b += v[i] == 2u;
  }
  uint32_t ta, tb;
  uint32_t ea = o1[blockIdx.x] + block_excl_scan(a, wsum, ta);
  __syncthreads();
  uint32_t eb = o2[blockIdx.x] + block_excl_scan(b, wsum, tb);
#pragma unroll
  for (int i = 0; i < CP_ITEMS; ++i) {
    const uint32_t t = blockIdx.x * CP_TILE + threadIdx.x * CP_ITEMS + i;
    if (v[i] == 1u) list1[ea++] = t;
    else if (v[i] == 2u) list2[eb++] = t;
  }
}
template <class Rec>
__global__ __launch_bounds__(WG) void mark_near_kernel(GridParams gp, const Rec* __restrict__ tgt, const uint32_t* __restrict__ list, const uint32_t* __restrict__ list_n,
                                                       uint32_t m, const uint8_t* __restrict__ near, uint8_t* __restrict__ mark) {
  const uint32_t i = blockIdx.x * WG + threadIdx.x;
  if (i >= (list ? *list_n : m)) return;
  const uint32_t pos = list ? list[i] : i;
  const Rec r = tgt[pos];
  const double q[3] = {(double)r.x, (double)r.y, (double)r.z};
  int c[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) c[a] = (int)fmin(fmax((q[a] - gp.bbmin[a]) * gp.inv_h, 0.0), (double)(gp.dim[a] - 1));     // as the search kernels place the target
  mark[pos] = near[cell_key(gp, c[0], c[1], c[2])] ? 2u : 1u;
}
template <class Rec>
void pt_launch_mark_near(const GridParams& gp, const Rec* tgt, const uint32_t* list, const uint32_t* list_n, uint32_t m, const uint8_t* near, uint8_t* mark, hipStream_t s) {
  if (m) hipLaunchKernelGGL(mark_near_kernel<Rec>, dim3((m + WG - 1) / WG), dim3(WG), 0, s, gp, tgt, list, list_n, m, near, mark);
}
template void pt_launch_mark_near<RecF>(const GridParams&, const RecF*, const uint32_t*, const uint32_t*, uint32_t, const uint8_t*, uint8_t*, hipStream_t);
template void pt_launch_mark_near<RecD>(const GridParams&, const RecD*, const uint32_t*, const uint32_t*, uint32_t, const uint8_t*, uint8_t*, hipStream_t);
// counts -> cnt[nt + 1] each (exclusive offsets, the totals in the last entry); scratch: 2 * (nt + 1) + scan scratch words
void pt_launch_mark_count(const uint8_t* mark, uint32_t m, uint32_t* off1, uint32_t* off2, uint32_t* scan_tmp, hipStream_t s) {
  const uint32_t nt = (m + CP_TILE - 1) / CP_TILE;
  (void)hipMemsetAsync(off1 + nt, 0, 4, s); (void)hipMemsetAsync(off2 + nt, 0, 4, s);
  if (nt) hipLaunchKernelGGL(mark_count_kernel, dim3(nt), dim3(WG), 0, s, mark, m, off1, off2);
  pt_launch_scan_u32(off1, off1, nt + 1, scan_tmp, s);
  pt_launch_scan_u32(off2, off2, nt + 1, scan_tmp, s);
}
void pt_launch_mark_write(const uint8_t* mark, uint32_t m, const uint32_t* off1, const uint32_t* off2, uint32_t* list1, uint32_t* list2, hipStream_t s) {
  const uint32_t nt = (m + CP_TILE - 1) / CP_TILE;
  if (nt) hipLaunchKernelGGL(mark_write_kernel, dim3(nt), dim3(WG), 0, s, mark, m, off1, off2, list1, list2);
}
uint32_t pt_mark_tiles(uint32_t m) { return (m + CP_TILE - 1) / CP_TILE; }

// pt_stream_query, once per chunk and sweep: the bound every target brings to this chunk's search, and how many targets bring one that
// reaches the chunk's bounding box at all (box distance: Distance::min_distance_to_rectangle of the reference, src/Distance.h:27-57;
// `<=` because an equal distance could still enter the list).
//   forward sweep, chunk c:   a target searched in an earlier chunk (first[t] < c) brings its current k-th squared distance (+inf while
//                             its list is short); one that has not been searched yet and lies INSIDE the chunk's box -- or within
//                             `margin` of it, a few point spacings: the distance over which its neighbours may well be in this chunk and
//                             an unbounded search from outside costs a ring or two -- is searched unbounded from now on (first[t] = c);
//                             one that lies farther outside and has no list yet is DEFERRED (-1: the
//                             kernels return an empty list for it) -- searching it from outside, unbounded, is the slow path of every
//                             kernel, and the chunk that holds its neighbourhood is still to come;
//   backward sweep, chunk c:  exactly the deferred pairs, first[t] > c, now with a bound.  Every (target, chunk) pair is searched once,
//                             under a bound that is an upper bound of the target's final k-th distance, so the merged lists are the
//                             resident search's.
// With a max_dist cap (cap2 < +inf) nothing is deferred: a target without a list brings cap2 -- it is searched from now on, within the
// cap, wherever it lies -- and one with a list brings min(k-th, cap2); the backward sweep then finds no pair left.
template <class T>
__global__ __launch_bounds__(WG) void stream_sweep_kernel(const T* __restrict__ x, const T* __restrict__ y, const T* __restrict__ z,
                                                          const unsigned long long* __restrict__ bi, const double* __restrict__ bd, uint32_t m, int k,
                                                          uint32_t c, int backward, uint32_t* __restrict__ first, double lx, double ly, double lz, double hx,
                                                          double hy, double hz, double margin2, double cap2, double* __restrict__ bound, uint32_t* count) {
  const uint32_t t = blockIdx.x * WG + threadIdx.x;
  bool reach = false;
  if (t < m) {
    const double q[3] = {(double)x[t], (double)y[t], (double)z[t]}, lo[3] = {lx, ly, lz}, hi[3] = {hx, hy, hz};
    double d = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) { const double g = q[a] < lo[a] ? lo[a] - q[a] : (q[a] > hi[a] ? q[a] - hi[a] : 0.0); d += g * g; }
    const size_t last = (size_t)t * (size_t)k + (size_t)(k - 1);
    const double kth = fmin(bi[last] != ~0ull ? bd[last] : INFINITY, cap2);
    const uint32_t f = first[t];
    double b;
    if (d != d) b = -1.0;                                       // a NaN coordinate: no neighbours anywhere, the row stays empty
    else if (backward) b = f > c ? kth : -1.0;
    else if (f < c) b = kth;
    else if (d <= margin2 || cap2 < INFINITY) { b = cap2; first[t] = c; }      // inside the box, or within a few point spacings of it (capped: anywhere)
    else b = -1.0;
    bound[t] = b;
    reach = b >= 0.0 && !(d > b);
  }
  const uint32_t n = (uint32_t)__popcll(__ballot(reach));
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(count, n);
}
template <class T>
void pt_launch_stream_sweep(const T* xyz_planar, const unsigned long long* best_idx, const double* best_d2, uint32_t m, int k, uint32_t chunk, int backward,
                            uint32_t* first, const double lo[3], const double hi[3], double margin, double cap2, double* bound, uint32_t* count, hipStream_t s) {
  if (m) hipLaunchKernelGGL(stream_sweep_kernel<T>, dim3((m + WG - 1) / WG), dim3(WG), 0, s, xyz_planar, xyz_planar + m, xyz_planar + 2 * (size_t)m, best_idx, best_d2,
                            m, k, chunk, backward, first, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], margin * margin, cap2, bound, count);
}
template void pt_launch_stream_sweep<float>(const float*, const unsigned long long*, const double*, uint32_t, int, uint32_t, int, uint32_t*, const double*, const double*,
                                            double, double, double*, uint32_t*, hipStream_t);
template void pt_launch_stream_sweep<double>(const double*, const unsigned long long*, const double*, uint32_t, int, uint32_t, int, uint32_t*, const double*, const double*,
                                             double, double, double*, uint32_t*, hipStream_t);
void pt_launch_merge_stream(const unsigned long long* best_idx, const double* best_d2, const uint32_t* chunk_idx, const double* chunk_d2,
                           unsigned long long base, uint32_t m, int k, unsigned long long* out_idx, double* out_d2, hipStream_t s) {
  if (!m) return;
  hipLaunchKernelGGL(merge_stream_kernel, dim3((m + WG - 1) / WG), dim3(WG), 0, s, best_idx, best_d2, chunk_idx, chunk_d2, base, m, k, out_idx, out_d2);
}

void pt_launch_merge(const uint32_t* idx_lists, const double* d2_lists, int g, uint32_t m, int k, uint32_t* idx_out, double* d2_out,
                     hipStream_t s) {
  if (!m) return;
  const uint64_t threads = (uint64_t)m * (uint64_t)(g * k);
  hipLaunchKernelGGL(merge_kernel, dim3((uint32_t)((threads + WG - 1) / WG)), dim3(WG), 0, s, idx_lists, d2_lists, g, m, k, idx_out, d2_out);
}

template <class T>
void pt_launch_slab_need(const T* x, const T* y, const T* z, const double* d2, uint32_t m, int k, int axis, const double* bounds_dev, int g,
                         int my_slab, double cap2, uint8_t* need, hipStream_t s) {
  if (!m) return;
  hipLaunchKernelGGL(slab_need_kernel<T>, dim3((m + WG - 1) / WG), dim3(WG), 0, s, x, y, z, d2, m, k, axis, bounds_dev, g, my_slab, cap2, need);
}
template void pt_launch_slab_need<float>(const float*, const float*, const float*, const double*, uint32_t, int, int, const double*, int, int,
                                         double, uint8_t*, hipStream_t);
template void pt_launch_slab_need<double>(const double*, const double*, const double*, const double*, uint32_t, int, int, const double*, int,
                                          int, double, uint8_t*, hipStream_t);

// the per-target bounds of a capped query (the group, hier and wave kernels read theirs by target id): min(bound2[t], cap2), or cap2
__global__ __launch_bounds__(WG) static void cap_bounds_kernel(const double* __restrict__ bound2, uint32_t m, double cap2, double* __restrict__ out) {
  const uint32_t t = blockIdx.x * WG + threadIdx.x;
  if (t < m) out[t] = bound2 ? fmin(bound2[t], cap2) : cap2;
}
void pt_launch_cap_bounds(const double* bound2, uint32_t m, double cap2, double* out, hipStream_t s) {
  if (m) hipLaunchKernelGGL(cap_bounds_kernel, dim3((m + WG - 1) / WG), dim3(WG), 0, s, bound2, m, cap2, out);
}
