// pt_voxel.hip -- voxel-grid downsampling of the resident cloud (pt_voxel_downsample, include/pt_api.h): the voxel
// keys, a stable LSD radix sort of (key, original index) pairs, the segment heads, and the segmented reduction that turns every voxel's
// members into one point.
//
// Determinism: the sort is stable and ranks by position only (no global cursor, no atomics that decide an order), so the members of a
// voxel arrive in ascending original index; a voxel's sums run over ranks 0 .. c - 1 in blocks of 256 -- one thread per block from left to
// right, then the block sums from left to right -- an order that is a function of c alone.  No floating-point atomic is used anywhere, and
// nothing depends on the number of compute units.
#include <hip/hip_fp16.h>

#include <utility>

#include "../../include/pt_api.h"
#include "pt_internal.h"

namespace {

constexpr int WG = 256;
constexpr int RS_ITEMS = 16, RS_TILE = WG * RS_ITEMS;      // keys per thread and per tile of the sort
constexpr uint32_t VB = PT_VOXEL_BLOCK;                    // members per block of the blocked sum: part of the DEFINITION, not a tunable
constexpr uint32_t NO_OWNER = 0xFFFFFFFFu;

__device__ inline double vx_widen(double v) { return v; }
__device__ inline double vx_widen(float v) { return (double)v; }
__device__ inline double vx_widen(__half v) { return (double)__half2float(v); }
// the quotient in the width the cloud is held in: fp32 by round-to-nearest-even, fp16 through fp32 (two roundings, as the header states)
template <class T> __device__ inline T vx_narrow(double q);
template <> __device__ inline double vx_narrow<double>(double q) { return q; }
template <> __device__ inline float vx_narrow<float>(double q) { return (float)q; }
template <> __device__ inline __half vx_narrow<__half>(double q) { return __float2half((float)q); }

// ---- keys ----------------------------------------------------------------------------------------------------------------------------
// i = floor((p - o) / v) per axis, the subtraction and the division rounded once each (a true division: -ffp-contract=off, no reciprocal);
// key = iz | iy | ix packed into bits[2] + bits[1] + bits[0] bits, z highest.  The host has checked the range from the bounding box.
template <class T, class Key>
__global__ __launch_bounds__(WG) void voxel_key_kernel(const T* __restrict__ x, const T* __restrict__ y, const T* __restrict__ z, uint32_t n, double ox,
                                                       double oy, double oz, double v, int bx, int by, Key* __restrict__ key, uint32_t* __restrict__ idx) {
  const uint32_t i = blockIdx.x * WG + threadIdx.x;
  if (i >= n) return;
  const double px = vx_widen(x[i]), py = vx_widen(y[i]), pz = vx_widen(z[i]);
  const unsigned long long ix = (unsigned long long)floor((px - ox) / v), iy = (unsigned long long)floor((py - oy) / v),
                           iz = (unsigned long long)floor((pz - oz) / v);
  key[i] = (Key)((iz << (bx + by)) | (iy << bx) | ix);
  idx[i] = i;
}

// ---- one pass of the radix sort ------------------------------------------------------------------------------------------------------
// the tile's digit histogram, written digit-major (H[d * ntiles + tile]): ONE flat exclusive scan of H then holds, for every (digit, tile),
// where that tile's run of that digit starts in the output
template <class Key>
__global__ __launch_bounds__(WG) void radix_hist_kernel(const Key* __restrict__ key, uint32_t n, int shift, uint32_t ntiles, uint32_t* __restrict__ H) {
  __shared__ uint32_t cnt[256];
  cnt[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t base = blockIdx.x * RS_TILE;
  Key k[RS_ITEMS];
#pragma unroll
  for (int i = 0; i < RS_ITEMS; ++i) k[i] = key[min(base + (uint32_t)i * WG + threadIdx.x, n - 1u)];      // (clamped, not branched: all loads in flight)
#pragma unroll
  for (int i = 0; i < RS_ITEMS; ++i)
    if (base + (uint32_t)i * WG + threadIdx.x < n) atomicAdd(&cnt[(uint32_t)(k[i] >> shift) & 255u], 1u);
  __syncthreads();
  H[(size_t)threadIdx.x * ntiles + blockIdx.x] = cnt[threadIdx.x];
}

// The scatter.  Wave w holds the tile's elements (w * RS_ITEMS + i) * 64 + lane, so (w, i, lane) is the input order.  Stable rank inside
// the tile, without a cursor: for every i the lanes of a wave that share a digit find each other with eight ballots; the lowest of them
// advances the wave's LDS counter of that digit by the size of the group and hands the old value to the others, whose rank is that value
// plus the number of group members in lower lanes.  The four waves' counters are then prefixed per digit, the tile's digit counts scanned,
// the pairs placed in tile order in LDS, and written out in runs: position q of the tile goes to Hscan[d][tile] + (q - first q of digit d).
// Elements past n (last tile) take digit 255 and the highest indices: they rank behind every real element and are never written.
template <class Key>
__global__ __launch_bounds__(WG) void radix_scatter_kernel(const Key* __restrict__ key, const uint32_t* __restrict__ idx, uint32_t n, int shift, uint32_t ntiles,
                                                           const uint32_t* __restrict__ Hscan, Key* __restrict__ okey, uint32_t* __restrict__ oidx) {
  __shared__ Key lk[RS_TILE];
  __shared__ uint32_t li[RS_TILE];
  __shared__ uint32_t wcnt[4 * 256];
  __shared__ uint32_t tile_ex[256], gb[256], wsum[4];
  volatile uint32_t* vcnt = wcnt;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long lower = (1ull << lane) - 1ull;
  const uint32_t base = blockIdx.x * RS_TILE;
#pragma unroll
  for (int q = 0; q < 4; ++q) wcnt[q * 256 + threadIdx.x] = 0;
  Key k[RS_ITEMS];
  uint32_t id[RS_ITEMS], rk[RS_ITEMS];
#pragma unroll
  for (int i = 0; i < RS_ITEMS; ++i) {
    const uint32_t e = min(base + (uint32_t)(w * RS_ITEMS + i) * 64u + (uint32_t)lane, n - 1u);
    k[i] = key[e];
    id[i] = idx[e];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < RS_ITEMS; ++i) {
    const uint32_t e = base + (uint32_t)(w * RS_ITEMS + i) * 64u + (uint32_t)lane;
    const uint32_t d = e < n ? (uint32_t)(k[i] >> shift) & 255u : 255u;
    unsigned long long peers = ~0ull;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long m = __ballot(bit);
      peers &= bit ? m : ~m;
    }
    const int leader = __ffsll((long long)peers) - 1;
    uint32_t old = 0;
    if (lane == leader) { old = vcnt[w * 256 + d]; vcnt[w * 256 + d] = old + (uint32_t)__popcll(peers); }
    old = (uint32_t)__shfl((int)old, leader);
    rk[i] = old + (uint32_t)__popcll(peers & lower);
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  {
    uint32_t tot = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) { const uint32_t c = wcnt[q * 256 + threadIdx.x]; wcnt[q * 256 + threadIdx.x] = tot; tot += c; }
    uint32_t total;
    tile_ex[threadIdx.x] = block_excl_scan(tot, wsum, total);
    gb[threadIdx.x] = Hscan[(size_t)threadIdx.x * ntiles + blockIdx.x];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < RS_ITEMS; ++i) {
    const uint32_t e = base + (uint32_t)(w * RS_ITEMS + i) * 64u + (uint32_t)lane;
    const uint32_t d = e < n ? (uint32_t)(k[i] >> shift) & 255u : 255u;
    const uint32_t r = tile_ex[d] + wcnt[w * 256 + d] + rk[i];
    if (r < (uint32_t)RS_TILE) { lk[r] = k[i]; li[r] = id[i]; }
  }
  __syncthreads();
  const uint32_t nvalid = min((uint32_t)RS_TILE, n - base);
#pragma unroll
  for (int i = 0; i < RS_ITEMS; ++i) {
    const uint32_t q = (uint32_t)i * WG + threadIdx.x;
    if (q < nvalid) {
      const Key kk = lk[q];
      const uint32_t d = (uint32_t)(kk >> shift) & 255u;
      const uint32_t pos = gb[d] + (q - tile_ex[d]);
      if (pos < n) { okey[pos] = kk; oidx[pos] = li[q]; }
    }
  }
}

// ---- segments ------------------------------------------------------------------------------------------------------------------------
template <class Key>
__global__ __launch_bounds__(WG) void voxel_heads_kernel(const Key* __restrict__ key, uint32_t n, uint8_t* __restrict__ mark) {
  const uint32_t i = blockIdx.x * WG + threadIdx.x;
  if (i >= n) return;
  mark[i] = (i == 0 || key[i] != key[i - 1]) ? 1u : 0u;
}

// members of the fullest voxel: one integer atomicMax per workgroup (launched over n, the bound on the number of voxels, which stays on the device)
__global__ __launch_bounds__(WG) void voxel_max_count_kernel(const uint32_t* __restrict__ start, const uint32_t* __restrict__ nv_dev, uint32_t n, uint32_t* __restrict__ out) {
  __shared__ uint32_t mx;
  if (threadIdx.x == 0) mx = 0;
  __syncthreads();
  const uint32_t nv = *nv_dev, j = blockIdx.x * WG + threadIdx.x;
  if (j < nv) atomicMax(&mx, (j + 1 < nv ? start[j + 1] : n) - start[j]);
  __syncthreads();
  if (threadIdx.x == 0 && mx) atomicMax(out, mx);
}

// ---- reduction -----------------------------------------------------------------------------------------------------------------------
// One block's (or one small voxel's) sums: the members idx[p .. p + m) in order, every sum STARTING FROM ITS FIRST TERM (a lone -0.0 stays
// -0.0); voxel_of is written on the way.  Without `apply` only voxel_of is.
struct Sums { double s[6]; uint32_t c[4]; };
template <class T>
__device__ inline void sum_members(const VoxelReduce& r, const T* __restrict__ x, uint32_t p, uint32_t m, uint32_t j, Sums& o) {
  const T* __restrict__ y = x + r.n;
  const T* __restrict__ z = y + r.n;
#pragma unroll
  for (int a = 0; a < 6; ++a) o.s[a] = 0.0;
#pragma unroll
  for (int a = 0; a < 4; ++a) o.c[a] = 0;
  for (uint32_t q = 0; q < m; ++q) {
    const uint32_t id = r.idx[p + q];
    if (id >= r.n) continue;      // (the sort moves an iota: never taken)
    r.voxel_of[id] = j;
    if (!r.apply) continue;
    const double v[3] = {vx_widen(x[id]), vx_widen(y[id]), vx_widen(z[id])};
#pragma unroll
    for (int a = 0; a < 3; ++a) o.s[a] = q ? o.s[a] + v[a] : v[a];
    if (r.attr) {
      const Attr t = pt_gather_attr(r.attr, id);
      const double nn[3] = {(double)t.nx, (double)t.ny, (double)t.nz};
#pragma unroll
      for (int a = 0; a < 3; ++a) o.s[3 + a] = q ? o.s[3 + a] + nn[a] : nn[a];
#pragma unroll
      for (int a = 0; a < 4; ++a) o.c[a] += (t.rgba >> (8 * a)) & 255u;
    }
  }
}
// result point j from its sums: S / c per axis in the stored width; colour bytes (2 s + c) / (2 c), round half up; normals S / c as floats
template <class T>
__device__ inline void write_voxel(const VoxelReduce& r, uint32_t j, uint32_t c, const double (&s)[6], const unsigned long long (&cs)[4]) {
  T* out = (T*)r.xyz_out;
  const double dc = (double)c;
#pragma unroll
  for (int a = 0; a < 3; ++a) out[(size_t)a * r.nv + j] = vx_narrow<T>(s[a] / dc);
  if (r.attr) {
    uint32_t rgba = 0;
#pragma unroll
    for (int a = 0; a < 4; ++a) rgba |= (uint32_t)((2ull * cs[a] + c) / (2ull * c)) << (8 * a);
    Attr t;
    t.rgba = rgba; t.nx = (float)(s[3] / dc); t.ny = (float)(s[4] / dc); t.nz = (float)(s[5] / dc);
    r.attr_out[j] = t;
  }
}
// where block b of a voxel that starts at sorted position s keeps its partial sums: two slots per 256 positions, the second for a voxel's
// FIRST block.  Blocks of one voxel start 256 positions apart and a voxel of more than 256 members is longer than that, so no two blocks
// share a slot (include/pt_api.h, "Memory").
__device__ inline uint32_t block_slot(uint32_t s, uint32_t b) { return 2u * ((s + b * VB) >> 8) + (b == 0 ? 1u : 0u); }

// one thread per voxel: count; c <= 256: the whole voxel; larger: its blocks' slots are claimed for the block kernel
template <class T>
__global__ __launch_bounds__(WG) void voxel_small_kernel(VoxelReduce r) {
  const uint32_t j = blockIdx.x * WG + threadIdx.x;
  if (j >= r.nv) return;
  const uint32_t s = r.start[j], e = j + 1 < r.nv ? r.start[j + 1] : r.n, c = e - s;
  r.count[j] = c;
  if (c > VB) {
    for (uint32_t b = 0; s + b * VB < e; ++b) {
      const uint32_t sl = block_slot(s, b);
      if (sl < r.nslots) r.owner[sl] = j;
    }
    return;
  }
  Sums o;
  sum_members<T>(r, (const T*)r.xyz, s, c, j, o);
  if (!r.apply) return;
  const unsigned long long cs[4] = {o.c[0], o.c[1], o.c[2], o.c[3]};
  write_voxel<T>(r, j, c, o.s, cs);
}
// one thread per claimed slot: P_b of its 256 (or fewer) members
template <class T>
__global__ __launch_bounds__(WG) void voxel_block_kernel(VoxelReduce r) {
  const uint32_t sl = blockIdx.x * WG + threadIdx.x;
  if (sl >= r.nslots) return;
  const uint32_t j = r.owner[sl];
  if (j == NO_OWNER || j >= r.nv) return;
  const uint32_t s = r.start[j], e = j + 1 < r.nv ? r.start[j + 1] : r.n;
  const uint32_t p = (sl & 1u) ? s : (((sl >> 1) << 8) | (s & 255u));
  if (p < s || p >= e) return;
  Sums o;
  sum_members<T>(r, (const T*)r.xyz, p, min(VB, e - p), j, o);
  if (r.apply) ((Sums*)r.part)[sl] = o;
}
// one thread per voxel of more than 256 members: its partials in order
template <class T>
__global__ __launch_bounds__(WG) void voxel_big_kernel(VoxelReduce r) {
  const uint32_t j = blockIdx.x * WG + threadIdx.x;
  if (j >= r.nv) return;
  const uint32_t s = r.start[j], e = j + 1 < r.nv ? r.start[j + 1] : r.n, c = e - s;
  if (c <= VB) return;
  double sum[6] = {0, 0, 0, 0, 0, 0};
  unsigned long long cs[4] = {0, 0, 0, 0};
  for (uint32_t b = 0; s + b * VB < e; ++b) {
    const uint32_t sl = block_slot(s, b);
    if (sl >= r.nslots) break;
    const Sums o = ((const Sums*)r.part)[sl];
#pragma unroll
    for (int a = 0; a < 6; ++a) sum[a] = b ? sum[a] + o.s[a] : o.s[a];
#pragma unroll
    for (int a = 0; a < 4; ++a) cs[a] += o.c[a];
  }
  write_voxel<T>(r, j, c, sum, cs);
}

inline dim3 grid_for(size_t items) { return dim3((unsigned)((items + WG - 1) / WG)); }

template <class Key>
int radix_sort(Key* a, Key* b, uint32_t* ia, uint32_t* ib, uint32_t n, int bits, uint32_t* hist, uint32_t* scan_tmp, hipStream_t s) {
  const uint32_t ntiles = pt_radix_tiles(n);
  int passes = 0;
  for (int shift = 0; shift < bits; shift += 8, ++passes) {
    hipLaunchKernelGGL(radix_hist_kernel<Key>, dim3(ntiles), dim3(WG), 0, s, a, n, shift, ntiles, hist);
    pt_launch_scan_u32(hist, hist, 256u * ntiles, scan_tmp, s);
    hipLaunchKernelGGL(radix_scatter_kernel<Key>, dim3(ntiles), dim3(WG), 0, s, a, ia, n, shift, ntiles, hist, b, ib);
    std::swap(a, b);
    std::swap(ia, ib);
  }
  return passes;
}

}  // namespace

static_assert(sizeof(Sums) == PT_VOXEL_PART_BYTES, "pt_internal.h states the size of a partial");

uint32_t pt_radix_tiles(uint32_t n) { return (uint32_t)(((size_t)n + RS_TILE - 1) / RS_TILE); }
uint32_t pt_voxel_slots(uint32_t n) { return 2u * ((n >> 8) + 1u); }

template <class T>
void pt_launch_voxel_keys(const T* xyz, uint32_t n, const double o[3], double v, const int bits[3], bool key64, void* key, uint32_t* idx, hipStream_t s) {
  if (!n) return;
  if (key64) hipLaunchKernelGGL((voxel_key_kernel<T, unsigned long long>), grid_for(n), dim3(WG), 0, s, xyz, xyz + n, xyz + 2 * (size_t)n, n, o[0], o[1], o[2], v, bits[0], bits[1], (unsigned long long*)key, idx);
  else hipLaunchKernelGGL((voxel_key_kernel<T, uint32_t>), grid_for(n), dim3(WG), 0, s, xyz, xyz + n, xyz + 2 * (size_t)n, n, o[0], o[1], o[2], v, bits[0], bits[1], (uint32_t*)key, idx);
}
template void pt_launch_voxel_keys<__half>(const __half*, uint32_t, const double*, double, const int*, bool, void*, uint32_t*, hipStream_t);
template void pt_launch_voxel_keys<float>(const float*, uint32_t, const double*, double, const int*, bool, void*, uint32_t*, hipStream_t);
template void pt_launch_voxel_keys<double>(const double*, uint32_t, const double*, double, const int*, bool, void*, uint32_t*, hipStream_t);

int pt_launch_radix_sort(void* key_a, void* key_b, uint32_t* idx_a, uint32_t* idx_b, uint32_t n, int bits, bool key64, uint32_t* hist, uint32_t* scan_tmp, hipStream_t s) {
  if (!n) return 0;
  return key64 ? radix_sort((unsigned long long*)key_a, (unsigned long long*)key_b, idx_a, idx_b, n, bits, hist, scan_tmp, s)
               : radix_sort((uint32_t*)key_a, (uint32_t*)key_b, idx_a, idx_b, n, bits, hist, scan_tmp, s);
}

void pt_launch_voxel_heads(const void* key, bool key64, uint32_t n, uint8_t* mark, hipStream_t s) {
  if (!n) return;
  if (key64) hipLaunchKernelGGL(voxel_heads_kernel<unsigned long long>, grid_for(n), dim3(WG), 0, s, (const unsigned long long*)key, n, mark);
  else hipLaunchKernelGGL(voxel_heads_kernel<uint32_t>, grid_for(n), dim3(WG), 0, s, (const uint32_t*)key, n, mark);
}

void pt_launch_voxel_max_count(const uint32_t* start, const uint32_t* nv_dev, uint32_t n, uint32_t* max_out, hipStream_t s) {
  (void)hipMemsetAsync(max_out, 0, 4, s);
  if (n) hipLaunchKernelGGL(voxel_max_count_kernel, grid_for(n), dim3(WG), 0, s, start, nv_dev, n, max_out);
}

template <class T>
void pt_launch_voxel_reduce(const VoxelReduce& r, bool blocked, hipStream_t s) {
  if (!r.nv) return;
  if (blocked) (void)hipMemsetAsync(r.owner, 0xFF, (size_t)r.nslots * sizeof(uint32_t), s);
  hipLaunchKernelGGL(voxel_small_kernel<T>, grid_for(r.nv), dim3(WG), 0, s, r);
  if (!blocked) return;
  hipLaunchKernelGGL(voxel_block_kernel<T>, grid_for(r.nslots), dim3(WG), 0, s, r);
  if (r.apply) hipLaunchKernelGGL(voxel_big_kernel<T>, grid_for(r.nv), dim3(WG), 0, s, r);
}
template void pt_launch_voxel_reduce<__half>(const VoxelReduce&, bool, hipStream_t);
template void pt_launch_voxel_reduce<float>(const VoxelReduce&, bool, hipStream_t);
template void pt_launch_voxel_reduce<double>(const VoxelReduce&, bool, hipStream_t);
