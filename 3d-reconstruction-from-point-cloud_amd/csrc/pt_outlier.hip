// pt_outlier.hip -- outlier removal on the resident cloud (pt_remove_outliers, include/pt_api.h): the consumer of
// the self-query's lists (one score per point), the two reductions behind the statistical threshold, the keep mask, and the gathers
// that compact the cloud in place.  The search itself is run_query's (pt_api.hip), chunk by chunk, as for pt_estimate_normals.
//
// Determinism: a row's score is summed by ONE thread from left to right, the reductions add per-thread runs, then LDS trees, then the
// per-workgroup partials in index order -- every order is a function of n alone (never of the chunk size, the route or the device), and
// no floating-point atomic is used anywhere.
#include "../../include/pt_api.h"
#include "pt_internal.h"

namespace {

constexpr int WG = 256;
constexpr int OS_ROWS = 128;                     // rows (= threads) per workgroup of the score kernel: 128 * 33 * 8 = 33 KB of LDS
constexpr int OS_STRIDE_MAX = PT_MAX_K | 1, OS_BATCH = 4;
constexpr int OR_ITEMS = 16, OR_TILE = WG * OR_ITEMS;      // scores per workgroup of the reductions: the grid is ceil(n / 4096), whatever the device

// One score per row of the chunk's lists.  Phase 1, coalesced: the workgroup's rows * k entries of d2 and idx are read as they lie in
// memory and sqrt(d2) -- or -1 for an entry that names no point -- goes to LDS, rows padded to an odd stride (a column read then touches
// 32 distinct bank pairs per half wave).  Phase 2: thread r walks row r from left to right; the first entry that names a point is the
// point itself (or its lower-indexed duplicate, d2 = 0) and is counted, not added.
//   statistical: score = (sum of the other entries' distances) / (c - 1), +inf when c <= 1;   radius: score = c - 1 (0 when c = 0)
template <class Rec>
__global__ __launch_bounds__(OS_ROWS) void outlier_score_kernel(const double* __restrict__ d2, const uint32_t* __restrict__ idx, uint32_t m, int k,
                                                                const Rec* __restrict__ rec, int radius_mode, double* __restrict__ score) {
  __shared__ double sh[OS_ROWS * OS_STRIDE_MAX];
  const uint32_t stride = (uint32_t)k | 1u;
  const uint32_t row0 = blockIdx.x * OS_ROWS;
  const uint32_t rows = min((uint32_t)OS_ROWS, m - row0);
  const uint32_t total = rows * (uint32_t)k;
  const size_t base = (size_t)row0 * (size_t)k;
  const uint32_t my_id = threadIdx.x < rows ? rec[row0 + threadIdx.x].id : 0u;      // (asked for first: it is needed last)
  for (uint32_t e0 = threadIdx.x; e0 < total; e0 += OS_ROWS * OS_BATCH) {      // OS_BATCH pairs of loads in flight per thread before the first wait
    double v[OS_BATCH];
    uint32_t id[OS_BATCH];
#pragma unroll
    for (int i = 0; i < OS_BATCH; ++i) {
      const uint32_t e = min(e0 + (uint32_t)i * OS_ROWS, total - 1u);           // (clamped, not branched: the loads stay unconditional)
      v[i] = d2[base + e];
      id[i] = idx[base + e];
    }
#pragma unroll
    for (int i = 0; i < OS_BATCH; ++i) {
      const uint32_t e = e0 + (uint32_t)i * OS_ROWS;
      const uint32_t r = e / (uint32_t)k, j = e - r * (uint32_t)k;
      const double d = sqrt(v[i]);
      if (e < total) sh[r * stride + j] = id[i] != PT_NOIDX_U ? d : -1.0;
    }
  }
  __syncthreads();
  if (threadIdx.x >= rows) return;
  const double* p = sh + threadIdx.x * stride;
  int c = 0;
  double sum = 0.0;
  for (int j = 0; j < k; ++j) {
    const double v = p[j];
    if (v >= 0.0) {
      if (c) sum += v;
      ++c;
    }
  }
  double s;
  if (radius_mode) s = c ? (double)(c - 1) : 0.0;
  else s = c >= 2 ? sum / (double)(c - 1) : INFINITY;
  score[my_id] = s;
}

// workgroup sums of a double and a count, in a fixed order: a tree over the 256 slots, stride halving
__device__ inline void block_tree_sum(double& v, uint32_t& cnt, double* sv, uint32_t* sc) {
  sv[threadIdx.x] = v; sc[threadIdx.x] = cnt;
  __syncthreads();
#pragma unroll
  for (int o = WG / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) { sv[threadIdx.x] += sv[threadIdx.x + o]; sc[threadIdx.x] += sc[threadIdx.x + o]; }
    __syncthreads();
  }
  v = sv[0]; cnt = sc[0];
}

// pass 0 (res == null): per workgroup the number of finite scores of its tile and their sum;  pass 1: the sum of (s - mean)^2 over them,
// mean = res[1].  Thread t takes the scores t, t + 256, ... of the tile (coalesced) in that order.
__global__ __launch_bounds__(WG) void outlier_partial_kernel(const double* __restrict__ score, uint32_t n, const double* __restrict__ res,
                                                             double* __restrict__ part_sum, uint32_t* __restrict__ part_cnt) {
  __shared__ double sv[WG];
  __shared__ uint32_t sc[WG];
  const double mean = res ? res[1] : 0.0;
  const size_t first = (size_t)blockIdx.x * OR_TILE;
  double v = 0.0;
  uint32_t cnt = 0;
#pragma unroll
  for (int i = 0; i < OR_ITEMS; ++i) {
    const size_t t = first + (size_t)i * WG + threadIdx.x;
    const double s = t < n ? score[t] : INFINITY;
    if (s < INFINITY) {
      const double d = s - mean;
      v += res ? d * d : s;
      ++cnt;
    }
  }
  block_tree_sum(v, cnt, sv, sc);
  if (threadIdx.x == 0) { part_sum[blockIdx.x] = v; part_cnt[blockIdx.x] = cnt; }
}

// ONE workgroup: the partials in index order (thread t: t, t + 256, ...), the same tree, and the result words
//   res[0] = n_f (finite scores), res[1] = mean, res[2] = stddev (population), res[3] = threshold = mean + alpha * stddev
__global__ __launch_bounds__(WG) void outlier_final_kernel(const double* __restrict__ part_sum, const uint32_t* __restrict__ part_cnt, uint32_t nparts,
                                                           int pass, double alpha, double* __restrict__ res) {
  __shared__ double sv[WG];
  __shared__ unsigned long long sc[WG];
  double v = 0.0;
  unsigned long long cnt = 0;
  for (uint32_t i = threadIdx.x; i < nparts; i += WG) { v += part_sum[i]; cnt += part_cnt[i]; }
  sv[threadIdx.x] = v; sc[threadIdx.x] = cnt;
  __syncthreads();
#pragma unroll
  for (int o = WG / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) { sv[threadIdx.x] += sv[threadIdx.x + o]; sc[threadIdx.x] += sc[threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x) return;
  const double nf = (double)sc[0];
  if (pass == 0) {
    res[0] = nf;
    res[1] = sc[0] ? sv[0] / nf : 0.0;
  } else {
    const double sd = sc[0] ? sqrt(sv[0] / nf) : 0.0;
    res[2] = sd;
    res[3] = res[1] + alpha * sd;
  }
}

// keep[i] = score[i] <= threshold (statistical: thr = res[3] on the device), or score[i] == full (radius: full = k - 1); four points per
// thread, one 32-bit store.  The mask buffer is padded to a multiple of four bytes; the padding reads 0.
__global__ __launch_bounds__(WG) void outlier_mask_kernel(const double* __restrict__ score, uint32_t n, const double* __restrict__ res, int radius_mode,
                                                          double full, uint32_t* __restrict__ keep4) {
  const size_t q = (size_t)blockIdx.x * WG + threadIdx.x;
  if (q * 4 >= n) return;
  const double thr = radius_mode ? full : res[3];
  uint32_t w = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const size_t t = q * 4 + i;
    if (t < n) {
      const double s = score[t];
      w |= (radius_mode ? s == thr : s <= thr) ? 1u << (8 * i) : 0u;
    }
  }
  keep4[q] = w;
}

// compaction: out[p][j] = in[p][map[j]] for `planes` planes of in_stride / nk elements -- writes coalesced, reads ascending (map ascends)
template <class T>
__global__ __launch_bounds__(WG) void outlier_gather_kernel(const T* __restrict__ in, size_t in_stride, const uint32_t* __restrict__ map, uint32_t nk,
                                                            int planes, T* __restrict__ out) {
  const size_t j = (size_t)blockIdx.x * WG + threadIdx.x;
  if (j >= nk) return;
  const uint32_t src = map[j];
  for (int p = 0; p < planes; ++p) out[(size_t)p * nk + j] = in[(size_t)p * in_stride + src];
}

inline dim3 grid_for(size_t items) { return dim3((unsigned)((items + WG - 1) / WG)); }

}  // namespace

template <class Rec>
void pt_launch_outlier_score(const double* d2, const uint32_t* idx, uint32_t m, int k, const Rec* rec, int radius_mode, double* score, hipStream_t s) {
  if (!m) return;
  hipLaunchKernelGGL(outlier_score_kernel<Rec>, dim3((m + OS_ROWS - 1) / OS_ROWS), dim3(OS_ROWS), 0, s, d2, idx, m, k, rec, radius_mode, score);
}
template void pt_launch_outlier_score<RecF>(const double*, const uint32_t*, uint32_t, int, const RecF*, int, double*, hipStream_t);
template void pt_launch_outlier_score<RecD>(const double*, const uint32_t*, uint32_t, int, const RecD*, int, double*, hipStream_t);

uint32_t pt_outlier_parts(uint32_t n) { return (uint32_t)(((size_t)n + OR_TILE - 1) / OR_TILE); }

void pt_launch_outlier_stats(const double* score, uint32_t n, double alpha, double* part_sum, uint32_t* part_cnt, double* res, hipStream_t s) {
  const uint32_t np = pt_outlier_parts(n);
  for (int pass = 0; pass < 2; ++pass) {
    if (np) hipLaunchKernelGGL(outlier_partial_kernel, dim3(np), dim3(WG), 0, s, score, n, pass ? res : nullptr, part_sum, part_cnt);
    hipLaunchKernelGGL(outlier_final_kernel, dim3(1), dim3(WG), 0, s, part_sum, part_cnt, np, pass, alpha, res);
  }
}

void pt_launch_outlier_mask(const double* score, uint32_t n, const double* res, int radius_mode, double full, uint8_t* keep, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(outlier_mask_kernel, grid_for(((size_t)n + 3) / 4), dim3(WG), 0, s, score, n, res, radius_mode, full, (uint32_t*)keep);
}

void pt_launch_gather(const void* in, size_t in_stride, size_t elem_bytes, const uint32_t* map, uint32_t nk, int planes, void* out, hipStream_t s) {
  if (!nk) return;
  switch (elem_bytes) {
    case 2: hipLaunchKernelGGL(outlier_gather_kernel<uint16_t>, grid_for(nk), dim3(WG), 0, s, (const uint16_t*)in, in_stride, map, nk, planes, (uint16_t*)out); break;
    case 4: hipLaunchKernelGGL(outlier_gather_kernel<uint32_t>, grid_for(nk), dim3(WG), 0, s, (const uint32_t*)in, in_stride, map, nk, planes, (uint32_t*)out); break;
    case 8: hipLaunchKernelGGL(outlier_gather_kernel<uint64_t>, grid_for(nk), dim3(WG), 0, s, (const uint64_t*)in, in_stride, map, nk, planes, (uint64_t*)out); break;
    default: hipLaunchKernelGGL(outlier_gather_kernel<uint4>, grid_for(nk), dim3(WG), 0, s, (const uint4*)in, in_stride, map, nk, planes, (uint4*)out); break;      // 16: attribute records
  }
}
