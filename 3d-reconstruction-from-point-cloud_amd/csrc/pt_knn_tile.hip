// pt_knn_tile.hip -- the LDS tile kernel of the exact k-NN search (pt_knn_common.h), for gfx950 (MI355X), and its launcher.
#include "pt_knn_common.h"

using namespace pt_knn;

namespace {

// =====================================================================================================================
// Tile kernel: one 8x8x8-cell block per workgroup, candidates staged in LDS, FOUR LANES (a DPP quad) PER TARGET.
//
// Why a second kernel: the 8-lanes-per-target kernel (pt_knn_group.hip) is VALU-issue-bound -- every step pays fp64 ranking and
// cross-lane insertion with 1/8 of the wave doing useful work.  Targets of one block share their 3x3x3 neighbourhoods,
// so the 10x10x10-cell region around the block is staged ONCE into LDS and ranked from there:
//   stage   one thread per region ROW builds the cell table (a row's cells x = 1..8 are eight consecutive keys of one
//           block); rows go HBM -> LDS by LDS-DMA with wave-uniform addresses, the 200 halo cells through registers;
//   pass 1  the lanes of a quad walk the 2x2x2 cells nearest to the target interleaved (lane q: records q, q+4, ...)
//           in fp32 and keep the K smallest VALUES only (v_med3 chain, no payload); one bitonic DPP merge + a max of
//           mins gives the quad's k-th smallest -> a proven upper bound on the exact k-th squared distance (any set of
//           >= k candidates bounds it; see `kth_bound32`);
//   pass 2  ring 1 under that bound, rows and end cells pruned in fp32; what is within the bound is appended, branch-
//           free, to the lane's own queue segment (no atomics);
//   pass 3  exact fp64 metric on the queued candidates, ranked by all-pairs counting through DPP quad broadcasts
//           (distance only; ranks that do not add up reveal equal distances and the quad recounts under (d2, index));
//           each survivor is written straight to its final slot.
// Targets that ring 1 cannot settle (k-th neighbour farther than the region guarantees, more candidates under the bound
// than the queue holds, region larger than the LDS budget) are appended to `todo` and finished by the group kernel.
// fp32 records only (the fp32 pre-filter needs exact fp32 inputs).
constexpr int TILE_R = 10, TILE_CELLS = TILE_R * TILE_R * TILE_R;
// Geometries: LARGE = 768 threads, 8448 staged records (132 KB, one workgroup per CU) for rho ~ 6-8;
//             SMALL = 512 threads, 4400 / 3888 staged records (two 80-KB workgroups per CU: one stages while the other ranks);
//             WIDE  = 512 threads, 8960 staged records, 64-entry queue, one per CU: k in 25..32.
// queue entries per quad (CAP: room for the k survivors plus whatever else the fp32 bound lets through) and per lane
// (LCAP: every lane of the quad appends to its own segment, so no atomics and no counters in LDS)
// WIDE: k in (24, 32] -- a longer queue for pass 3 (512-thread workgroups: the registers of 12 waves would not hold it)
template <int K, bool WIDE> struct TileQ { static constexpr int CAP = K == 8 ? 24 : (K == 16 ? 40 : (WIDE ? 64 : 48)), LCAP = K == 8 ? 8 : 16; };

// LDS read of one staged record as ONE ds_read_b128 (4 LDS cycles per wave-instruction).  Without the empty asm the
// compiler drops the unused id and emits ds_read_b96, which costs 8 (MI355X_MICROARCH.md, LDS table).
__device__ inline RecF lds_rec(const RecF* p) {
  const float4 v = *reinterpret_cast<const float4*>(p);
  asm volatile("" ::"v"(v.w));
  RecF r;
  r.x = v.x; r.y = v.y; r.z = v.z; r.id = __float_as_uint(v.w);
  return r;
}
// two staged records, both reads issued before either is waited for
__device__ inline void lds_rec2(const RecF* p, const RecF* q, RecF& a, RecF& b) {
  const float4 u = *reinterpret_cast<const float4*>(p), v = *reinterpret_cast<const float4*>(q);
  asm volatile("" ::"v"(u.w), "v"(v.w));
  a.x = u.x; a.y = u.y; a.z = u.z; a.id = __float_as_uint(u.w);
  b.x = v.x; b.y = v.y; b.z = v.z; b.id = __float_as_uint(v.w);
}
// d32 is computed from exact fp32 inputs with 3 sub, 1 mul, 2 fma: relative error < 2^-21 (all terms >= 0).
// If b = k-th smallest d32 of a candidate set, then k candidates have exact d2 <= b*(1+2^-21), so the exact k-th d2
// D_k <= b*(1+2^-21), and every candidate with exact d2 <= D_k has d32 <= b*(1+2^-21)^2 < b*(1+2^-18).
__device__ inline float kth_bound32(float b) { return b * 1.0000038146972656f + 1e-30f; }   // 1 + 2^-18, + denormal slack

template <int CTRL>
__device__ inline float dpp_f32(float v) { return __uint_as_float(dpp_u32<CTRL>(__float_as_uint(v))); }
constexpr int DPP_QP_1032 = 0xB1;    // quad_perm [1,0,3,2]: partner lane ^ 1
constexpr int DPP_QP_2301 = 0x4E;    // quad_perm [2,3,0,1]: partner lane ^ 2
constexpr int DPP_QP_0000 = 0x00, DPP_QP_1111 = 0x55, DPP_QP_2222 = 0xAA, DPP_QP_3333 = 0xFF;

// merge my ascending list with the partner lane's: afterwards both lanes hold the K smallest of the 2K values, ascending
template <int K, int CTRL>
__device__ inline void quad_merge_sorted(float (&l)[K]) {
#pragma unroll
  for (int j = 0; j < K / 2; ++j) {                    // bitonic: lowest K of the union, in place (pairs j, K-1-j)
    const float a = l[j], b = l[K - 1 - j];
    const float pa = dpp_f32<CTRL>(b), pb = dpp_f32<CTRL>(a);
    l[j] = fminf(a, pa); l[K - 1 - j] = fminf(b, pb);
  }
#pragma unroll
  for (int d = K / 2; d >= 1; d >>= 1) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      if ((j & d) == 0) { const float lo = fminf(l[j], l[j + d]), hi = fmaxf(l[j], l[j + d]); l[j] = lo; l[j + d] = hi; }
    }
  }
}

// one LDS-DMA wave-instruction: active lane L copies 16 bytes from its own `g` to `lbase + L` (lbase wave-uniform)
__device__ inline void glds16(const uint4* g, uint4* lbase) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g, (__attribute__((address_space(3))) void*)lbase, 16, 0, 0);
}

// BLEND: the attribute blend fused into the kernel (TileBlend, pt_internal.h).
// Second chance for blocks whose region is over this geometry's LDS budget but within the large geometry's: their ids go
// to `retry` (retry != null), and a second launch (blocks != null: blockIdx.x indexes that list) takes them.
struct TileBlocks { const uint32_t* blocks; uint32_t* retry; uint32_t* retry_n; uint32_t retry_cap; const double* bound; double cap2; };
// BND: every target brings a radius bound, min(bound[id], cap2) -- bound[id] (may be null) the k-th squared distance it already has from
// another part of the cloud (the chunks of a streamed source, pt_stream_query), cap2 the context's uniform "max_dist" squared (+inf when
// off) -- and only points with d2 <= bound matter.  The bound joins pass 1's own (whichever is smaller prunes pass 2), settles targets
// whose k-th neighbour lies beyond ring 1 when the bound does not, drops queued candidates whose EXACT d2 is beyond it, and lets targets
// with fewer than k points in reach finish with a short list (the rest NOIDX / +inf, as a bounded query returns).  With BLEND too (the
// capped fused query) a row with at least one neighbour is blended over what it has, and a row with none is not written; those
// variants read cap2 only (no caller brings per-target bounds to a blended query), which keeps the bound in a scalar register.
// DBL: an fp64 cloud (TileDouble, pt_internal.h).

// KC: length of pass 1's per-lane value chain (<= K).  The merges and the ranking run at width K (a power of two); a chain of KC
// entries leaves l32[KC..K) at +inf, which is all a query with k <= KC needs: the reference's K = 20 runs the K = 32 body with
// a 24-deep chain (three quarters of pass 1's per-candidate work).
template <int K, int TILE_CAP, int TWG, bool WIDE = false, bool BLEND = false, bool DBL = false, int KC = K, bool BND = false>
__global__ __launch_bounds__(TWG, TILE_CAP > 5000 ? 1 : (TWG == 384 ? 3 : 4)) void knn_tile_kernel(GridParams gp, const RecF* __restrict__ src, const uint32_t* __restrict__ cs,
                                                        const RecF* __restrict__ tgt, const uint32_t* __restrict__ tblock_start, int k,
                                                        uint32_t* __restrict__ out_idx, double* __restrict__ out_d2,
                                                        uint32_t* __restrict__ todo, uint32_t* __restrict__ todo_n, TileBlend bl, TileBlocks tb,
                                                        TileDouble dd) {
  constexpr int NW = TWG / 64;
  constexpr int TILE_QUADS = TWG / 4;
  constexpr int TILE_QCAP = TileQ<K, WIDE>::CAP, TILE_LCAP = TileQ<K, WIDE>::LCAP;
  __shared__ __attribute__((aligned(16))) RecF lrec[TILE_CAP];
  __shared__ uint16_t lstart[TILE_CELLS + 8];
  __shared__ __attribute__((aligned(16))) uint16_t queue[TWG * (TILE_LCAP + 1)];          // doubles as rowdesc[] during staging
  __shared__ uint32_t wsum[NW];
  __shared__ uint32_t ptotal;
  // per region row: global starts of its left halo cell / its run of 8 cells / its right halo cell, and the LDS offsets
  // of cells 0, 1, 9 and of the next row (two 16-bit pairs)
  uint4* rowdesc = reinterpret_cast<uint4*>(queue);
  uint32_t* rowdesc_e = reinterpret_cast<uint32_t*>(queue) + 4 * TILE_R * TILE_R;
  static_assert(sizeof(queue) >= 5 * TILE_R * TILE_R * sizeof(uint32_t), "rowdesc aliases the queue");
  static_assert(TILE_CAP < 65536, "LDS offsets are 16-bit");

  uint32_t b = blockIdx.x;
  if (tb.blocks) b = tb.blocks[blockIdx.x];
  const uint32_t ts = tblock_start[b], te = tblock_start[b + 1];   // (waited for only after the cell-table loads below are out)
  // block id -> cell origin of the block
  const uint32_t macro = b >> 9, m9 = b & 511u;
  const int bx = (int)(macro % (uint32_t)gp.mdim[0]) * 8 + (int)((m9 & 1u) | ((m9 >> 2) & 2u) | ((m9 >> 4) & 4u));
  const int by = (int)((macro / (uint32_t)gp.mdim[0]) % (uint32_t)gp.mdim[1]) * 8 + (int)(((m9 >> 1) & 1u) | ((m9 >> 3) & 2u) | ((m9 >> 5) & 4u));
  const int bz = (int)(macro / (uint32_t)(gp.mdim[0] * gp.mdim[1])) * 8 + (int)(((m9 >> 2) & 1u) | ((m9 >> 4) & 2u) | ((m9 >> 6) & 4u));
#if defined(PT_ABLATE) && PT_ABLATE == 4
  // timing-only build: every workgroup stages the region of one of 512 HOT blocks (one macro block in the middle of the grid:
  // L2 / Infinity-Cache resident) and its targets are shifted into that block -- same ranking work, no HBM traffic for staging
  const uint32_t hmacro = (uint32_t)(((gp.mdim[2] / 2) * gp.mdim[1] + gp.mdim[1] / 2) * gp.mdim[0] + gp.mdim[0] / 2), hm9 = b & 511u;
  const int hbx = (int)(hmacro % (uint32_t)gp.mdim[0]) * 8 + (int)((hm9 & 1u) | ((hm9 >> 2) & 2u) | ((hm9 >> 4) & 4u));
  const int hby = (int)((hmacro / (uint32_t)gp.mdim[0]) % (uint32_t)gp.mdim[1]) * 8 + (int)(((hm9 >> 1) & 1u) | ((hm9 >> 3) & 2u) | ((hm9 >> 5) & 4u));
  const int hbz = (int)(hmacro / (uint32_t)(gp.mdim[0] * gp.mdim[1])) * 8 + (int)(((hm9 >> 2) & 1u) | ((hm9 >> 4) & 2u) | ((hm9 >> 6) & 4u));
  const double hshift[3] = {(double)((hbx - bx) * 8) * gp.h, (double)((hby - by) * 8) * gp.h, (double)((hbz - bz) * 8) * gp.h};
  const int ox = hbx * 8 - 1, oy = hby * 8 - 1, oz = hbz * 8 - 1;
#else
  const int ox = bx * 8 - 1, oy = by * 8 - 1, oz = bz * 8 - 1;          // cell coordinates of region cell (0,0,0)
#endif

  // ---- A: region cell table (global start + LDS offset of each of the 1000 cells).  One thread per region ROW (y, z):
  //         cells x = 1..8 of a row are eight consecutive keys of one block, so a row needs three key computations
  //         (left halo cell, the run, right halo cell) and 13 table words.  Waves 0 and 1 do this; the rest go to the barrier.
  constexpr int NROWS = TILE_R * TILE_R;
  if (threadIdx.x < 128) {
    const int row = threadIdx.x;
    uint32_t g[TILE_R], cnt[TILE_R], sum = 0;
#pragma unroll
    for (int i = 0; i < TILE_R; ++i) { g[i] = 0; cnt[i] = 0; }
    if (row < NROWS) {
      const int y = oy + row % TILE_R, z = oz + row / TILE_R;
      if (y >= 0 && y < gp.dim[1] && z >= 0 && z < gp.dim[2]) {
        const uint32_t km = cell_key(gp, ox + 1, y, z);              // cells ox+1 .. ox+8: keys km .. km+7 (32-byte aligned)
        const uint4 m0 = *reinterpret_cast<const uint4*>(cs + km), m1 = *reinterpret_cast<const uint4*>(cs + km + 4);
        const uint32_t m8 = cs[km + 8];
        uint32_t l0 = 0, l1 = 0, r0 = 0, r1 = 0;
        if (ox >= 0) { const uint32_t kl = cell_key(gp, ox, y, z); l0 = cs[kl]; l1 = cs[kl + 1]; }
        if (ox + 9 < gp.dim[0]) { const uint32_t kr = cell_key(gp, ox + 9, y, z); r0 = cs[kr]; r1 = cs[kr + 1]; }
        g[0] = l0; g[1] = m0.x; g[2] = m0.y; g[3] = m0.z; g[4] = m0.w; g[5] = m1.x; g[6] = m1.y; g[7] = m1.z; g[8] = m1.w; g[9] = r0;
        cnt[0] = l1 - l0; cnt[9] = r1 - r0;
        cnt[1] = m0.y - m0.x; cnt[2] = m0.z - m0.y; cnt[3] = m0.w - m0.z; cnt[4] = m1.x - m0.w;
        cnt[5] = m1.y - m1.x; cnt[6] = m1.z - m1.y; cnt[7] = m1.w - m1.z; cnt[8] = m8 - m1.w;
      }
#pragma unroll
      for (int i = 0; i < TILE_R; ++i) sum += cnt[i];
    }
    // INVARIANT: ts and te are loaded from tblock_start[b] with b a function of blockIdx.x only, so they are the same in
    // every lane of every wave of the workgroup: either ALL waves return here (and in the else branch below) or none does,
    // and every wave that stays executes exactly one s_barrier in its branch -- the table waves the one between their scan
    // halves, the other waves the one in the else branch -- before all of them meet again at the __syncthreads() below.
    // (The test sits here rather than at the top so that the cell-table loads are in flight while ts / te arrive.)
    if (ts == te) return;                               // no targets in this block
    const uint32_t incl = wave_incl_scan(sum);
    if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = incl;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();                       // all waves: waves >= 2 execute the matching s_barrier in the else branch
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const uint32_t w0 = wsum[0], w1 = wsum[1];
    uint32_t ex = (threadIdx.x >= 64 ? w0 : 0u) + incl - sum;
    if (row < NROWS) {
      uint32_t lo[TILE_R + 1];
#pragma unroll
      for (int i = 0; i < TILE_R; ++i) {
        lo[i] = ex < 65535u ? ex : 65535u;
        lstart[row * TILE_R + i] = (uint16_t)lo[i];
        ex += cnt[i];
      }
      lo[TILE_R] = ex < 65535u ? ex : 65535u;
      rowdesc[row] = make_uint4(g[0], g[1], g[9], lo[0] | (lo[1] << 16));
      rowdesc_e[row] = lo[9] | (lo[TILE_R] << 16);
    }
    if (threadIdx.x == 0) { const uint32_t tot = w0 + w1; lstart[TILE_CELLS] = (uint16_t)(tot < 65535u ? tot : 65535u); ptotal = tot; }
  } else {
    if (ts == te) return;                               // same workgroup-uniform test as above
    __builtin_amdgcn_s_barrier();                       // pairs with the barrier between the two table waves' scan halves
  }
  __syncthreads();
  const uint32_t P = ptotal;
  if (P > (uint32_t)TILE_CAP) {                     // denser than the LDS budget
    bool again = false;
    if constexpr (!WIDE) again = tb.retry && P <= tb.retry_cap;
    if (again) {                                    // ... but not than the large geometry's: that launch takes the block
      if constexpr (!WIDE) { if (threadIdx.x == 0) tb.retry[atomicAdd(tb.retry_n, 1u)] = b; }
    } else {                                        // the group kernel takes the whole tile
      for (uint32_t t = ts + threadIdx.x; t < te; t += TWG) todo[atomicAdd(todo_n, 1u)] = t;
    }
    return;
  }
  // the first round's target of this quad: requested here so that it arrives during the staging (loaded where it is first used,
  // every round began with a memory latency that nothing else of the wave could cover)
  RecF tr_first;
  tr_first.x = tr_first.y = tr_first.z = 0.f; tr_first.id = 0;
  if constexpr (!DBL) { if (ts + (threadIdx.x >> 2) < te) tr_first = tgt[ts + (threadIdx.x >> 2)]; }
  // ---- B: stage the region, HBM -> LDS directly (global_load_lds_dwordx4: wave-uniform LDS base + lane * 16, per-lane
  //         source address; no staging registers).  Cells x = 1..8 of a region row are one contiguous run in HBM and in
  //         LDS: two DMA instructions per row (<= 128 records) with wave-uniform (scalar) addresses; the 200 halo cells
  //         (x = 0 and 9) follow through registers.  Every load of the tile is in flight before the first wait.
  {
    const uint4* __restrict__ src4 = reinterpret_cast<const uint4*>(src);     // records move as raw 16-byte words
    uint4* l4 = reinterpret_cast<uint4*>(lrec);
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    constexpr int RPW = (NROWS + NW - 1) / NW;                      // rows per wave (9 or 13)
    bool long_rows = false;
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      const int rr = w + i * NW;
      if (rr < NROWS) {                                             // wave-uniform
        const uint32_t g1 = __builtin_amdgcn_readfirstlane(rowdesc[rr].y);
        const uint32_t p01 = __builtin_amdgcn_readfirstlane(rowdesc[rr].w), p9 = __builtin_amdgcn_readfirstlane(rowdesc_e[rr]);
        const uint32_t la1 = p01 >> 16, nm = (p9 & 0xFFFFu) - la1;
        if ((uint32_t)lane < nm) glds16(src4 + g1 + lane, l4 + la1);
        if ((uint32_t)lane + 64u < nm) glds16(src4 + g1 + 64 + lane, l4 + la1 + 64u);
        long_rows |= nm > 128u;
      }
    }
    // halo cells: 16 records would waste a 64-lane DMA each, so 8-lane groups move them through registers
    const int g8 = threadIdx.x >> 3, l8 = threadIdx.x & 7;
    constexpr int NHALO = 2 * NROWS;
    constexpr int HC = (NHALO + TWG / 8 - 1) / (TWG / 8);           // halo cells per 8-lane group
    uint4 h0[HC], h1[HC];
    uint32_t hla[HC], hlen[HC];
    bool long_cells = false;
#pragma unroll
    for (int i = 0; i < HC; ++i) {
      const int hcr = g8 + i * (TWG / 8);
      const int hc = hcr < NHALO ? hcr : NHALO - 1;
      const int c = (hc >> 1) * TILE_R + ((hc & 1) ? TILE_R - 1 : 0);
      hla[i] = lstart[c];
      hlen[i] = hcr < NHALO ? lstart[c + 1] - hla[i] : 0u;
      const uint32_t ga = (hc & 1) ? rowdesc[hc >> 1].z : rowdesc[hc >> 1].x;
      h0[i] = make_uint4(0, 0, 0, 0); h1[i] = make_uint4(0, 0, 0, 0);
      if ((uint32_t)l8 < hlen[i]) h0[i] = src4[ga + l8];
      if ((uint32_t)l8 + 8u < hlen[i]) h1[i] = src4[ga + l8 + 8u];
      long_cells |= hlen[i] > 16u;
    }
#pragma unroll
    for (int i = 0; i < HC; ++i) {
      if ((uint32_t)l8 < hlen[i]) l4[hla[i] + l8] = h0[i];
      if ((uint32_t)l8 + 8u < hlen[i]) l4[hla[i] + l8 + 8u] = h1[i];
    }
    if (long_rows) {                                                // very dense rows: the rest synchronously
      for (int rr = w; rr < NROWS; rr += NW) {
        const uint32_t g1 = rowdesc[rr].y, la1 = rowdesc[rr].w >> 16, nm = (rowdesc_e[rr] & 0xFFFFu) - la1;
        for (uint32_t p = lane + 128u; p < nm; p += 64) l4[la1 + p] = src4[g1 + p];
      }
    }
    if (long_cells) {
      for (int hc = g8; hc < NHALO; hc += TWG / 8) {
        const int c = (hc >> 1) * TILE_R + ((hc & 1) ? TILE_R - 1 : 0);
        const uint32_t a0 = lstart[c], n0 = lstart[c + 1] - a0, ga = (hc & 1) ? rowdesc[hc >> 1].z : rowdesc[hc >> 1].x;
        for (uint32_t p = l8 + 16u; p < n0; p += 8) l4[a0 + p] = src4[ga + p];
      }
    }
  }
  __syncthreads();                                  // rowdesc is dead from here on: the queue takes its place
#if defined(PT_ABLATE) && PT_ABLATE == 1
  if (lrec[threadIdx.x % (P ? P : 1u)].id == 0xFFFFFFFEu) out_idx[0] = 1;   // keeps the staging alive
  return;                                           // timing-only build: staging cost alone (results are garbage)
#endif

  // ---- C: four lanes per target, 192 targets per round ----------------------------------------------------------------
  const double h2 = gp.h * gp.h;
  const int quad = threadIdx.x >> 2, ql = threadIdx.x & 3;
  for (uint32_t base = ts; base < te; base += TILE_QUADS) {
    const uint32_t t = base + quad;
    const bool active = t < te;                                        // whole quads are active or not
    RecF tr;
    tr.x = tr.y = tr.z = 0.f; tr.id = 0;
    double q[3] = {0.0, 0.0, 0.0};
    if constexpr (DBL) {
      if (active) { const RecD td = dd.tgt[t]; q[0] = td.x; q[1] = td.y; q[2] = td.z; tr.x = (float)td.x; tr.y = (float)td.y; tr.z = (float)td.z; tr.id = td.id; }
    } else {
      if (base == ts) tr = tr_first;                    // (workgroup-uniform test)
      else if (active) tr = tgt[t];
#if defined(PT_ABLATE) && PT_ABLATE == 4
      tr.x = (float)((double)tr.x + hshift[0]); tr.y = (float)((double)tr.y + hshift[1]); tr.z = (float)((double)tr.z + hshift[2]);
#endif
      q[0] = (double)tr.x; q[1] = (double)tr.y; q[2] = (double)tr.z;
    }
    double u[3];
    int cc[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      u[a] = (q[a] - gp.bbmin[a]) * gp.inv_h;
      cc[a] = (int)fmin(fmax(u[a], 0.0), (double)(gp.dim[a] - 1));
    }
    const int rx = active ? cc[0] - ox : 1, ry = active ? cc[1] - oy : 1, rz = active ? cc[2] - oz : 1;   // in [1, 8]
    const int cbase = (rz * TILE_R + ry) * TILE_R + (rx - 1);          // region cell left of the target's cell
    // The four lanes of a quad walk every run of records together, lane ql taking records ql, ql+4, ... of it: the quad
    // reads 64 contiguous bytes per step, every lane sees a quarter of every cell (even shares), and the trip counts are
    // the same for the whole quad.

    // ---- pass 1: the K smallest fp32 distances (values only) of the 2x2x2 cells nearest to the target -- on each axis
    //      the target's cell and its neighbour on the target's side.  Any candidate set with >= k members gives a valid
    //      bound; this one holds most of the k nearest at a quarter of ring 1's reads.  (Fewer than k points there: the
    //      bound is +inf, the queue overflows and the target goes to the todo list.)  Per-lane lists shorter than K would
    //      still be valid but loosen the bound: measured 3.7 % of the targets overflow the queue with 3K/4, 17 % with K/2. ----
    const int sx = (u[0] - (double)cc[0]) >= 0.5 ? 0 : -1, sy = (u[1] - (double)cc[1]) >= 0.5 ? 0 : -1, sz = (u[2] - (double)cc[2]) >= 0.5 ? 0 : -1;
    double bnd = INFINITY;
    if constexpr (BND && BLEND) bnd = tb.cap2;          // (the fused blend comes with the uniform cap only: a scalar, no registers per lane)
    else if constexpr (BND) {
      if (active) bnd = tb.bound ? fmin(tb.bound[tr.id], tb.cap2) : tb.cap2;
    }
    const bool scan1 = active && !(BND && bnd < 0.0);      // (a negative bound -- "nothing from this cloud" -- skips pass 1 too; pass 2 prunes itself)
    float l32[K];
#pragma unroll
    for (int j = 0; j < K; ++j) l32[j] = INFINITY;
    auto push1 = [&](float x) {
      float prev = l32[0];
      l32[0] = fminf(x, prev);
#pragma unroll
      for (int j = 1; j < KC; ++j) { const float cur = l32[j]; l32[j] = __builtin_amdgcn_fmed3f(x, prev, cur); prev = cur; }
    };
    {
      uint32_t ps[4], pe[4];
#pragma unroll
      for (int o = 0; o < 4; ++o) {                    // all eight table reads in flight together
        const int c = cbase + ((sz + (o >> 1)) * TILE_R + (sy + (o & 1))) * TILE_R + 1 + sx;
        ps[o] = (uint32_t)lstart[c] + ql;
        pe[o] = scan1 ? (uint32_t)lstart[c + 2] : 0u;
      }
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        uint32_t p = ps[o];
        const uint32_t e = pe[o];
        for (; p + 4 < e; p += 8) {
          RecF a, b;
          lds_rec2(&lrec[p], &lrec[p + 4], a, b);
          push1(dist2_f32(tr.x, tr.y, tr.z, a)); push1(dist2_f32(tr.x, tr.y, tr.z, b));
        }
        if (p < e) push1(dist2_f32(tr.x, tr.y, tr.z, lds_rec(&lrec[p])));
      }
    }
    // the quad's K smallest: two bitonic merges through DPP (all lanes of the wave take part: no divergence here)
    quad_merge_sorted<K, DPP_QP_1032>(l32);
    float kv;
    if (k == K) {                                      // only the K-th smallest is wanted: the largest of the bitonic lower half
      kv = fminf(l32[0], dpp_f32<DPP_QP_2301>(l32[K - 1]));
#pragma unroll
      for (int j = 1; j < K; ++j) kv = fmaxf(kv, fminf(l32[j], dpp_f32<DPP_QP_2301>(l32[K - 1 - j])));
    } else {
      quad_merge_sorted<K, DPP_QP_2301>(l32);
      kv = l32[0];
#pragma unroll
      for (int j = 1; j < K; ++j) kv = (j == k - 1) ? l32[j] : kv;
    }
    float thr = kth_bound32(kv);
    if constexpr (BND) {
      // a candidate with exact d2 <= bnd has d32 <= bnd (1 + 2^-21): the bound rounded UP to fp32, times 1 + 2^-20
      thr = bnd < 0.0 ? -1.f : fminf(thr, __double2float_ru(bnd) * 1.000001f + 1e-30f);
    }
    if constexpr (DBL) {
      // Rounded coordinates move every difference by at most E per axis (source + target rounding), i.e. every distance
      // by at most sqrt(3) E: k candidates lie within sqrt(kv') + sqrt(3) E of the target, so the true top k do, and
      // their rounded distances are within another sqrt(3) E.  (1.0000005 covers sqrtf's rounding.)  A caller's bound (BND) is on
      // EXACT distances: what it lets through has a rounded distance within ONE sqrt(3) E of it, so the same widening covers it.
      if (!BND || thr >= 0.f) {
        const float e_t = 5.9604645e-8f * fmaxf(fmaxf(fabsf(tr.x), fabsf(tr.y)), fabsf(tr.z));
        const float r = sqrtf(thr) * 1.0000005f + 3.4642f * (dd.e_src + e_t) * 1.000001f;
        thr = r * r * 1.0000039f + 1e-30f;
      }
    }
#if defined(PT_ABLATE) && PT_ABLATE == 2
    if (thr >= 0.f) continue;                       // timing-only build: staging + pass 1 (results are garbage)
#endif

    // ---- pass 2: scan ring 1 under the bound; what is within it goes to this lane's own queue segment.  Rows and their end
    //      cells are pruned in fp32 on the target's position inside its cell, with gaps UNDER-estimated by a slack far above
    //      the rounding of the products, so nothing that could hold a candidate within the bound is skipped. ----
    const float fx = (float)(u[0] - (double)cc[0]), fy = (float)(u[1] - (double)cc[1]), fz = (float)(u[2] - (double)cc[2]);
    const float h2f = (float)h2;
    auto gapf = [&](float f, int d) -> float {         // distance (in cells) from offset f in the centre cell to cell d = -1, 0, +1
      const float g = fmaxf((float)d - f, f - (float)(d + 1)) - 4e-6f * (1.f + fabsf(f));
      return fmaxf(g, 0.f);
    };
    const float g2x[3] = {gapf(fx, -1) * gapf(fx, -1), 0.f, gapf(fx, 1) * gapf(fx, 1)};
    const float g2y[3] = {gapf(fy, -1) * gapf(fy, -1), gapf(fy, 0) * gapf(fy, 0), gapf(fy, 1) * gapf(fy, 1)};
    const float g2z[3] = {gapf(fz, -1) * gapf(fz, -1), gapf(fz, 0) * gapf(fz, 0), gapf(fz, 1) * gapf(fz, 1)};
    // branch-free append: the position is always stored at the segment's next slot and the count only moves when the
    // candidate is within the bound (a rejected one is overwritten by its successor); slot TILE_LCAP takes the spill.
    uint16_t* myq = &queue[threadIdx.x * (TILE_LCAP + 1)];
    uint32_t nmine = 0;
    auto push2 = [&](float x, uint32_t p) {
      myq[nmine < (uint32_t)TILE_LCAP ? nmine : (uint32_t)TILE_LCAP] = (uint16_t)p;
      nmine += (x <= thr) ? 1u : 0u;
    };
    {
      uint32_t qs[9], qe[9];
#pragma unroll
      for (int r = 0; r < 9; ++r) {                    // the runs of all nine rows first: their table reads overlap
        const int dy = r % 3 - 1, dz = r / 3 - 1;
        const int c = cbase + (dz * TILE_R + dy) * TILE_R;
        const float s2 = g2y[dy + 1] + g2z[dz + 1];
        const bool row_on = active && !(s2 * h2f > thr);
        const bool lo_on = !((g2x[0] + s2) * h2f > thr), hi_on = !((g2x[2] + s2) * h2f > thr);
        qe[r] = row_on ? (uint32_t)lstart[hi_on ? c + 3 : c + 2] : 0u;
        qs[r] = (uint32_t)lstart[lo_on ? c : c + 1] + ql;
      }
#pragma unroll
      for (int r = 0; r < 9; ++r) {
        uint32_t p = qs[r];
        const uint32_t e = qe[r];
        for (; p + 4 < e; p += 8) {
          RecF a, b;
          lds_rec2(&lrec[p], &lrec[p + 4], a, b);
          push2(dist2_f32(tr.x, tr.y, tr.z, a), p); push2(dist2_f32(tr.x, tr.y, tr.z, b), p + 4);
        }
        if (p < e) push2(dist2_f32(tr.x, tr.y, tr.z, lds_rec(&lrec[p])), p);
      }
    }
    // A quad's segments are written and read by lanes of ONE wave: the LDS executes a wave's operations in issue order and
    // the scans above have reconverged, so no workgroup barrier is needed -- only a compiler fence.
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();

    // ---- pass 3: exact metric, ranking by all-pairs counting inside the quad ----
    const uint32_t n0 = dpp_u32<DPP_QP_0000>(nmine), n1 = dpp_u32<DPP_QP_1111>(nmine), n2 = dpp_u32<DPP_QP_2222>(nmine),
                   n3 = dpp_u32<DPP_QP_3333>(nmine);
    const uint32_t p1 = n0, p2 = n0 + n1, p3 = p2 + n2, nq = p3 + n3;
    const bool overflow = nq > (uint32_t)TILE_QCAP || n0 > (uint32_t)TILE_LCAP || n1 > (uint32_t)TILE_LCAP || n2 > (uint32_t)TILE_LCAP ||
                          n3 > (uint32_t)TILE_LCAP;                                 // quad-uniform by construction
#if defined(PT_ABLATE) && PT_ABLATE == 3
    if (nq < 1000u) continue;                          // timing-only build: staging + passes 1, 2
#endif
    double od[TILE_QCAP / 4];
    uint32_t oi[TILE_QCAP / 4];
    int rk[TILE_QCAP / 4];
#pragma unroll
    for (int j = 0; j < TILE_QCAP / 4; ++j) {          // my entries of the concatenated segments: ql, ql+4, ...
      const uint32_t e = (uint32_t)(4 * j + ql);
      od[j] = INFINITY; oi[j] = PT_NOIDX_U; rk[j] = 0;
      if (e < nq && !overflow) {
        const uint32_t seg = (uint32_t)(e >= p1) + (uint32_t)(e >= p2) + (uint32_t)(e >= p3);
        const uint32_t off = e - (seg == 0 ? 0u : (seg == 1 ? p1 : (seg == 2 ? p2 : p3)));
        const RecF r = lrec[queue[((threadIdx.x & ~3u) + seg) * (TILE_LCAP + 1) + off]];
        if constexpr (DBL) { const RecD rd = dd.src[r.id]; od[j] = dist2(q, rd); oi[j] = rd.id; }     // r.id: sorted position of the exact record
        else { od[j] = dist2(q, r); oi[j] = r.id; }
        if constexpr (BND) if (od[j] > bnd) { od[j] = INFINITY; oi[j] = PT_NOIDX_U; }   // let through by the widened fp32 bound only
      }
    }
    // (BND) entries that survived the exact test -- the list is short when fewer than k did; without BND every queued entry counts
    uint32_t nval = nq;
    if constexpr (BND) {
      nval = 0;
#pragma unroll
      for (int j = 0; j < TILE_QCAP / 4; ++j) nval += oi[j] != PT_NOIDX_U ? 1u : 0u;
      nval += dpp_u32<DPP_QP_1032>(nval);
      nval += dpp_u32<DPP_QP_2301>(nval);
    }
    // Ranking counts, for each of my entries, the queue entries with a smaller distance.  Equal distances (rare) leave
    // two entries with the same count: the ranks then do not add up to 0 + 1 + ... + (nq-1) and the quad redoes the count
    // under the full order (d2, index).
    auto rank_all = [&](auto lt) {
#pragma unroll
      for (int j = 0; j < TILE_QCAP / 4; ++j) {        // round j: the four lanes' j-th entries visit every lane
        if ((uint32_t)(4 * j) < nq) {                  // quad-uniform
          const double b0 = dpp_f64<DPP_QP_0000>(od[j]), b1 = dpp_f64<DPP_QP_1111>(od[j]), b2 = dpp_f64<DPP_QP_2222>(od[j]),
                       b3 = dpp_f64<DPP_QP_3333>(od[j]);
          const uint32_t i0 = dpp_u32<DPP_QP_0000>(oi[j]), i1 = dpp_u32<DPP_QP_1111>(oi[j]), i2 = dpp_u32<DPP_QP_2222>(oi[j]),
                         i3 = dpp_u32<DPP_QP_3333>(oi[j]);
#pragma unroll
          for (int m = 0; m < TILE_QCAP / 4; ++m) {
            if ((uint32_t)(4 * m) < nq)                // quad-uniform: slots beyond the queue hold +inf and rank nowhere
              rk[m] += (int)lt(b0, i0, od[m], oi[m]) + (int)lt(b1, i1, od[m], oi[m]) + (int)lt(b2, i2, od[m], oi[m]) +
                       (int)lt(b3, i3, od[m], oi[m]);
          }
        }
      }
    };
    if constexpr (K > 16 && (WIDE || (BLEND && DBL))) {   // (register budget of the wide and of the fp64 + blend variants: one ranking body only)
      rank_all([](double ad, uint32_t ai, double bd, uint32_t bi) { return key_lt(ad, ai, bd, bi); });
    } else {
      rank_all([](double ad, uint32_t, double bd, uint32_t) { return ad < bd; });
      int rs = 0;
#pragma unroll
      for (int j = 0; j < TILE_QCAP / 4; ++j) rs += (oi[j] != PT_NOIDX_U) ? rk[j] : 0;
      rs += (int)dpp_u32<DPP_QP_1032>((uint32_t)rs);
      rs += (int)dpp_u32<DPP_QP_2301>((uint32_t)rs);
      const uint32_t nv = overflow ? 0u : nval;
      if ((uint32_t)rs != nv * (nv - 1u) / 2u) {       // quad-uniform
#pragma unroll
        for (int j = 0; j < TILE_QCAP / 4; ++j) rk[j] = 0;
        rank_all([](double ad, uint32_t ai, double bd, uint32_t bi) { return key_lt(ad, ai, bd, bi); });
      }
    }
    // exact k-th squared distance of ring 1 (rank k-1), known to one lane -> quad minimum
    double kd = INFINITY;
#pragma unroll
    for (int j = 0; j < TILE_QCAP / 4; ++j) if (oi[j] != PT_NOIDX_U && rk[j] == k - 1) kd = od[j];
    kd = fmin(kd, dpp_f64<DPP_QP_1032>(kd));
    kd = fmin(kd, dpp_f64<DPP_QP_2301>(kd));
    bool covered = true;
    double dout = INFINITY;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int lo = cc[a] - 1, hi = cc[a] + 1;
      if (lo > 0) { covered = false; dout = fmin(dout, u[a] - (double)lo); }
      if (hi < gp.dim[a] - 1) { covered = false; dout = fmin(dout, (double)(hi + 1) - u[a]); }
    }
    dout = fmax(dout - PT_CELL_EPS, 0.0);
    const bool done = !overflow && (covered || dout * dout * h2 > (BND ? fmin(kd, bnd) : kd));
    if (active) {
      if (done) {
        const size_t row = (size_t)tr.id * (size_t)k;
        // (BLEND) the k neighbours' attribute records are gathered right here, GB of a lane's gathers issued before anything waits
        // for one, the first group before the result stores (the memory counter is in order: a load behind a store waits for it).
        // Gather, wait, accumulate per neighbour -- the first form of this -- cost a lane six random-access latencies in a row.
        // GB: all six entries at k <= 8, four at a time beyond (registers); the fp64 + blend variants have none left and keep
        // gathering one by one.  The loads are unconditional -- an entry that is not among the k reads record 0, one cached line
        // for the whole chip -- because behind a branch each the compiler still put a full wait between them.
        constexpr int NE = TILE_QCAP / 4;
        constexpr int GB = (BLEND && !DBL) ? (NE <= 6 ? NE : 4) : 1;
        auto store_results = [&]() {
#pragma unroll
          for (int j = 0; j < NE; ++j)
            if (oi[j] != PT_NOIDX_U && rk[j] < k) { out_idx[row + rk[j]] = oi[j]; if (out_d2) out_d2[row + rk[j]] = od[j]; }
          for (uint32_t sl = nval + ql; sl < (uint32_t)k; sl += 4) { out_idx[row + sl] = PT_NOIDX_U; if (out_d2) out_d2[row + sl] = INFINITY; }
        };
        if constexpr (!BLEND) store_results();
        if constexpr (BLEND) {
          // blended as pt_attr.hip's blend_kernel does: fp64 sums, then one normalisation
          double ws = 0.0, c0 = 0.0, c1 = 0.0, c2 = 0.0, n0 = 0.0, n1 = 0.0, n2 = 0.0;
#pragma unroll
          for (int g0 = 0; g0 < NE; g0 += GB) {
            Attr at[GB];
            if constexpr (GB > 1) {
#pragma unroll
              for (int q = 0; q < GB; ++q) {
                const int j = g0 + q < NE ? g0 + q : NE - 1;
                at[q] = pt_gather_attr(bl.attr, (g0 + q < NE && oi[j] != PT_NOIDX_U && rk[j] < k && oi[j] < bl.n_attr) ? oi[j] : 0u);
              }
            }
            if (g0 == 0) store_results();
#pragma unroll
            for (int q = 0; q < GB; ++q) {
              const int j = g0 + q < NE ? g0 + q : NE - 1;
              if (g0 + q < NE && oi[j] != PT_NOIDX_U && rk[j] < k && oi[j] < bl.n_attr) {
                const double w = (bl.mode == 1) ? 1.0 / (od[j] + 1e-12) : 1.0;
                Attr a;
                if constexpr (GB > 1) a = at[q]; else a = pt_gather_attr(bl.attr, oi[j]);
                ws += w;
                c0 += w * (double)(a.rgba & 0xFFu); c1 += w * (double)((a.rgba >> 8) & 0xFFu); c2 += w * (double)((a.rgba >> 16) & 0xFFu);
                n0 += w * (double)a.nx; n1 += w * (double)a.ny; n2 += w * (double)a.nz;
              }
            }
          }
          auto quad_sum = [](double v) { v += dpp_f64<DPP_QP_1032>(v); v += dpp_f64<DPP_QP_2301>(v); return v; };
          ws = quad_sum(ws); c0 = quad_sum(c0); c1 = quad_sum(c1); c2 = quad_sum(c2); n0 = quad_sum(n0); n1 = quad_sum(n1); n2 = quad_sum(n2);
          if (ws > 0.0) {
            // The sums above are fp64 (normals may cancel); the finishing touches use the hardware reciprocal and
            // reciprocal square root (v_rcp_f64 / v_rsq_f64, ~2^-23 relative: two orders inside the 1e-5 bar) instead of
            // four fp64 divisions and a square root, which were a third of this epilogue's instructions.
            const double iw = __builtin_amdgcn_rcp(ws);
            c0 *= iw; c1 *= iw; c2 *= iw;
            const double l2 = n0 * n0 + n1 * n1 + n2 * n2;
            const double sc = (l2 * iw * iw >= 1e-24) ? __builtin_amdgcn_rsq(l2) : iw;      // |mean normal| >= 1e-12: renormalise
            n0 *= sc; n1 *= sc; n2 *= sc;
          }
          float* o = (ql == 0) ? bl.rgb_out : bl.nrm_out;
          if (ql < 2 && o && (!BND || nval != 0)) {            // (capped: a row with no neighbour in reach keeps what the caller put there)
            o[3 * (size_t)tr.id] = (float)(ql == 0 ? c0 : n0); o[3 * (size_t)tr.id + 1] = (float)(ql == 0 ? c1 : n1);
            o[3 * (size_t)tr.id + 2] = (float)(ql == 0 ? c2 : n2);
          }
        }
      } else if (ql == 0) {
        todo[atomicAdd(todo_n, 1u)] = t;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");     // next round's segment writes stay behind this round's reads
    __builtin_amdgcn_wave_barrier();
  }
}

}  // namespace

// ---- the blocks that hold targets, as a list (round 4): what the tile kernel is launched over on clouds that leave most of their grid
// empty -- a surface in a fine grid has one block in a dozen occupied, and an empty block's workgroup still costs its launch and two loads
__global__ __launch_bounds__(WG) void tblock_list_kernel(const uint32_t* __restrict__ tblock_start, uint32_t nblocks, uint32_t* __restrict__ list, uint32_t* count) {
  const uint32_t b = blockIdx.x * WG + threadIdx.x;
  const bool has = b < nblocks && tblock_start[b + 1] > tblock_start[b];
  const unsigned long long mask = __ballot(has);
  if (!mask) return;                                        // wave-uniform
  uint32_t base = 0;
  if ((threadIdx.x & 63) == 0) base = atomicAdd(count, (uint32_t)__popcll(mask));
  base = (uint32_t)__shfl((int)base, 0);
  if (has) list[base + (uint32_t)__popcll(mask & ((1ull << (threadIdx.x & 63)) - 1ull))] = b;      // (block order kept inside a wave: neighbours in the list are neighbours in the grid)
}
void pt_launch_tblock_list(const uint32_t* tblock_start, uint32_t nblocks, uint32_t* list, uint32_t* count, hipStream_t s) {
  (void)hipMemsetAsync(count, 0, 4, s);
  if (nblocks) hipLaunchKernelGGL(tblock_list_kernel, dim3((nblocks + WG - 1) / WG), dim3(WG), 0, s, tblock_start, nblocks, list, count);
}

namespace {

// The launch of PT_TILE_ROUTE[ROW].  The three run-time booleans become template arguments one call at a time (F... grows to
// <BLEND, DBL, BND>); then the instantiation is named from the same constexpr row as the code that is returned, so the code cannot
// drift from the launch.  Nine rows x eight combinations: every knn_tile_kernel there is, and no other.
template <int ROW, bool... F>
uint32_t tile_launch_row(const TileLaunch& t, uint32_t nb) {
  constexpr TileRoute R = PT_TILE_ROUTE[ROW];
  constexpr bool FLAG[3] = {F...};
  constexpr bool BLEND = FLAG[0], DBL = FLAG[1], BND = FLAG[2];
  const TileBlocks tbk{t.blocks, t.retry, t.retry_n, (uint32_t)PT_TILE_CAP_LARGE, t.bound, t.cap2};
  hipLaunchKernelGGL((knn_tile_kernel<R.K, R.CAP, R.TWG, R.WIDE, BLEND, DBL, R.KC, BND>), dim3(nb), dim3(R.TWG), 0, t.stream, t.gp, t.src, t.cell_start, t.tgt,
                     t.tblock_start, t.k, t.out_idx, t.out_d2, t.todo, t.todo_n, t.blend, tbk, t.dbl);
  return pt_tile_code(R, BLEND, DBL, BND, t.blocks != nullptr);
}
template <int ROW, bool... F, class... Rest>
uint32_t tile_launch_row(const TileLaunch& t, uint32_t nb, bool f, Rest... rest) {
  return f ? tile_launch_row<ROW, F..., true>(t, nb, rest...) : tile_launch_row<ROW, F..., false>(t, nb, rest...);
}

}  // namespace

// The bounded variants (BND) answer per-target bounds (pt_stream_query's chunks; never with a blend: the blended variants read cap2
// only), the context's max_dist (cap2), or both; blend.attr selects the fused blend, dbl.src the fp64 variants.
// (round 3: the K = 32 body on 1024 threads -- 16 waves per CU, 128 VGPRs with 56 bytes of spills, 7680-record region -- measured 6.77 ms
//  against 6.74 at 100M / 10M: more waves of one workgroup do not shorten its latency chain, DESIGN.md section 6.  No such route.)
uint32_t pt_launch_knn_tile(const TileLaunch& t) {
  const uint32_t nb = t.blocks ? t.nblocks_listed : (uint32_t)t.gp.nblocks;
  if (!nb) return 0u;
  const bool blend = t.blend.attr != nullptr, dbl = t.dbl.src != nullptr, capped = t.cap2 < INFINITY, bnd = t.bound || capped;
  static_assert(PT_TILE_ROUTES == 9, "one case per row of PT_TILE_ROUTE");
  switch (pt_tile_route_row(t.k, t.geometry, bnd, capped)) {
    case 0: return tile_launch_row<0>(t, nb, blend, dbl, bnd);
    case 1: return tile_launch_row<1>(t, nb, blend, dbl, bnd);
    case 2: return tile_launch_row<2>(t, nb, blend, dbl, bnd);
    case 3: return tile_launch_row<3>(t, nb, blend, dbl, bnd);
    case 4: return tile_launch_row<4>(t, nb, blend, dbl, bnd);
    case 5: return tile_launch_row<5>(t, nb, blend, dbl, bnd);
    case 6: return tile_launch_row<6>(t, nb, blend, dbl, bnd);
    case 7: return tile_launch_row<7>(t, nb, blend, dbl, bnd);
    default: return tile_launch_row<8>(t, nb, blend, dbl, bnd);
  }
}
