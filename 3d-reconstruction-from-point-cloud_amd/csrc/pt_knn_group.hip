// pt_knn_group.hip -- the group kernel of the exact k-NN search (pt_knn_common.h): EIGHT LANES PER TARGET, for gfx950 (MI355X).
//
// knn_kernel answers what the tile kernel does not take: fp64 clouds, radius-bounded multi-GPU queries, the todo list.
// 8 lanes per target, 8 targets per wave64, 32 per 256-thread workgroup:
//   - ring 1 (the 3x3x3 cells around the target) is 9 x-rows of 3 cells.  The group's lanes look the rows'
//     cell ranges up in parallel (one latency for all of them), then the rows are processed centre first;
//     a row's surviving cells are flattened into one index space so that the 8 lanes always read 8 consecutive
//     candidates (128-B lines of 16-B records), a whole row's records are requested in one batch, and the next
//     row's batch is already in flight while the current one is ranked;
//   - the running top-k lives in registers, distributed over the group's lanes (lane L holds ranks
//     [L*KPL, (L+1)*KPL), KPL = ceil(k/8)), ordered by the total order (d2, original index);
//   - a candidate is offered with one group ballot, accepted through one ballot bit of the lane that holds rank
//     k-1, and inserted as a one-position shift across lanes done with DPP row operations (no LDS traffic);
//   - rings >= 2 (needed by the few targets whose k-th neighbour is farther than one cell) use a plain
//     row-by-row walk.
// Control flow is uniform inside a group (all lanes of a group take every branch together), so cross-lane
// operations never see an inactive partner; different groups of a wave diverge freely.
#include "pt_knn_common.h"

using namespace pt_knn;

namespace {

constexpr int GL = 8;   // lanes per target

// broadcast lane 7 (resp. lane 0) of every 8-lane group to the whole group; L = lane index inside the group
__device__ inline uint32_t bcast7(uint32_t v, int L) { const uint32_t a = dpp_u32<DPP_QUAD3>(v), b = dpp_u32<DPP_HMIRROR>(a); return L < 4 ? b : a; }
__device__ inline double bcast7(double v, int L) { const double a = dpp_f64<DPP_QUAD3>(v), b = dpp_f64<DPP_HMIRROR>(a); return L < 4 ? b : a; }

// ---- the running top list of one target, spread over the 8 lanes of its group ------------------------------------
template <int KPL>
struct TopList {
  double ld[KPL];
  uint32_t li[KPL];
  double lim_d, bnd_d;     // acceptance limit = min(entry of rank k-1, caller's bound); index NOIDX when it is a bare bound
  uint32_t lim_i;
  int L, hl, hr;
  uint32_t notfirst;       // 0 for lane 0 of the group, 1 otherwise
  bool fullk;              // k == 8*KPL: the rank k-1 entry is the last entry of lane 7
#ifdef PT_VISITS
  uint32_t nv;             // instrumented build (tools/probe_visits.py): offers made (8 records each)
#endif

  __device__ void init(int lane_in_group, int k, double bound) {
#pragma unroll
    for (int j = 0; j < KPL; ++j) { ld[j] = INFINITY; li[j] = PT_NOIDX_U; }
    L = lane_in_group;
    notfirst = lane_in_group != 0 ? 1u : 0u;
    hl = (k - 1) / KPL;
    hr = (k - 1) % KPL;
    fullk = (k == GL * KPL);
    bnd_d = bound;
    lim_d = bound;
    lim_i = PT_NOIDX_U;
#ifdef PT_VISITS
    nv = 0;
#endif
  }
  // cheap pre-test against the cached limit (may be stale, i.e. too permissive -- never too strict)
  __device__ bool may_accept(double d, uint32_t i) const { return key_lt(d, i, lim_d, lim_i); }

  // Try to insert (xd, xi), known by every lane of the group.  The exact acceptance test is the comparison with the
  // entry of rank k-1, which lives in lane hl: its verdict reaches the group through one ballot bit, so the k-th
  // entry itself never has to be broadcast.  Returns whether the list changed.
  __device__ bool try_insert(double xd, uint32_t xi, int gshift) {
    bool cj[KPL];
#pragma unroll
    for (int j = 0; j < KPL; ++j) cj[j] = key_lt(xd, xi, ld[j], li[j]);
    bool csel = cj[0];
#pragma unroll
    for (int j = 1; j < KPL; ++j) if (hr == j) csel = cj[j];
    const bool acc = ((__ballot(csel) >> (gshift + hl)) & 1ull) != 0ull;   // group-uniform
    if (!acc) return false;
    // one-position shift: the lane below hands over its last entry if the new key sorts before it.
    // (every cross-lane move is executed by ALL lanes of the group: never under a lane-dependent branch, or the
    //  source lane may be masked off; lane 0's incoming value is discarded arithmetically instead)
    const double pd = dpp_f64<DPP_SHR1>(ld[KPL - 1]);
    const uint32_t pi = dpp_u32<DPP_SHR1>(li[KPL - 1]);
    const bool pc = (dpp_u32<DPP_SHR1>(cj[KPL - 1] ? 1u : 0u) & notfirst) != 0u;
#pragma unroll
    for (int j = KPL - 1; j >= 1; --j) {
      if (cj[j - 1]) { ld[j] = ld[j - 1]; li[j] = li[j - 1]; }
      else if (cj[j]) { ld[j] = xd; li[j] = xi; }
    }
    if (pc) { ld[0] = pd; li[0] = pi; }
    else if (cj[0]) { ld[0] = xd; li[0] = xi; }
    return true;
  }

  // re-read the limit after insertions: the entry of rank k-1, unless the caller's bound is tighter
  __device__ void refresh_limit() {
    double kd;
    uint32_t ki;
    if (fullk) {
      kd = bcast7(ld[KPL - 1], L);
      ki = bcast7(li[KPL - 1], L);
    } else {
      kd = ld[0];
      ki = li[0];
#pragma unroll
      for (int j = 1; j < KPL; ++j) if (hr == j) { kd = ld[j]; ki = li[j]; }
      kd = __shfl(kd, hl, GL);
      ki = __shfl(ki, hl, GL);
    }
    if (key_lt(kd, ki, bnd_d, PT_NOIDX_U)) { lim_d = kd; lim_i = ki; }
    else { lim_d = bnd_d; lim_i = PT_NOIDX_U; }
  }

  // offer one candidate per lane (d = +inf / id = NOIDX for lanes without one)
  __device__ void offer(double d, uint32_t id, int gshift) {
#ifdef PT_VISITS
    ++nv;
#endif
    const bool pass = may_accept(d, id) && !(d > bnd_d);
    uint32_t mask = (uint32_t)(__ballot(pass) >> gshift) & 0xFFu;
    if (mask) {
      bool changed = false;
      do {
        const int t = __ffs(mask) - 1;
        mask &= mask - 1;
        const double xd = __shfl(d, t, GL);
        const uint32_t xi = __shfl(id, t, GL);
        changed |= try_insert(xd, xi, gshift);
      } while (mask);
      if (changed) refresh_limit();
    }
  }
};

// geometry of one target relative to the grid
struct TargetGeom {
  double q[3], u[3];
  int c[3];
  double h2;
  // distance (cell units, >= 0) from the target to the cell interval [lo, hi] along axis a, minus the slack
  __device__ double gap(int a, int lo, int hi) const {
    const double g = fmax((double)lo - u[a], u[a] - (double)(hi + 1)) - PT_CELL_EPS;
    return fmax(g, 0.0);
  }
};

// =====================================================================================================================
// Search over the REFINED grid (pt_refine.hip), used by the group kernel (knn_kernel<.., HIER = true>): a cell that carries a node
// is not scanned end to end but descended into.  Inside a node the 64 rows of sub-cells are tested against the current bound
// eight at a time (one lane each), the surviving rows are cut to the sub-cells the bound still reaches, leaf sub-cells are scanned
// as before and sub-cells that are nodes themselves are descended into the same way (PT_REFINE_DEPTH levels).  The sub-cell that
// holds the target is visited FIRST on every level, so the bound is tight before the neighbours are looked at; it is skipped when
// the sweep over the rows comes by, so no point is ever offered twice.  Exact for the same reason the group kernel is: a box is
// skipped only if Distance::min_distance_to_rectangle (reference src/Distance.h:27-57) of it exceeds the current k-th distance.
template <class Rec, int KPL>
struct HierScan {
  const GridParams& gp;
  const Rec* __restrict__ src;
  const uint32_t* __restrict__ nodes;
  const TargetGeom& T;
  TopList<KPL>& top;
  int gshift;

  __device__ void range(uint32_t s, uint32_t e) {
    for (uint32_t base = s; base < e; base += GL) {
      const uint32_t p = base + (uint32_t)top.L;
      double d = INFINITY;
      uint32_t id = PT_NOIDX_U;
      if (p < e) { const Rec r = src[p]; d = dist2(T.q, r); id = r.id; }
      top.offer(d, id, gshift);
    }
  }
  // squared distance (cell units) from the target to the interval [lo, hi] on axis a, under-estimated by the slack
  __device__ double gap2(int a, double lo, double hi) const {
    const double g = fmax(fmax(lo - T.u[a], T.u[a] - hi) - PT_CELL_EPS, 0.0);
    return g * g;
  }
  template <int DEPTH>
  __device__ void node(uint32_t nid) {
    const uint32_t* __restrict__ N = nodes + (size_t)(nid - 1u) * PT_NODE_WORDS;
    const double* hd = reinterpret_cast<const double*>(N);
    const double ox = hd[0], oy = hd[1], oz = hd[2], inv = hd[3], w = hd[4];        // w = 1 / inv: sub-cell side in cell units (a power of 1/8)
    // the sub-cell the target falls in, if it is inside this node's box
    const double rx = (T.u[0] - ox) * inv, ry = (T.u[1] - oy) * inv, rz = (T.u[2] - oz) * inv;
    const bool inside = rx >= 0.0 && rx < 8.0 && ry >= 0.0 && ry < 8.0 && rz >= 0.0 && rz < 8.0;
    const uint32_t own = inside ? (uint32_t)(((int)rz << 6) | ((int)ry << 3) | (int)rx) : 0xFFFFFFFFu;
    // per-axis gaps of the eight slabs of sub-cells, one per lane: every box test below is two or three shuffles and adds
    const double fl = (double)top.L;
    const double gxl = gap2(0, ox + fl * w, ox + (fl + 1.0) * w), gyl = gap2(1, oy + fl * w, oy + (fl + 1.0) * w), gzl = gap2(2, oz + fl * w, oz + (fl + 1.0) * w);
    // the rows (sy, sz) that can hold anything under the bound as it is now -- geometry only, no memory touched; lane L tests
    // the rows with sy = L, one sz per step
    uint32_t live_lo = 0, live_hi = 0;                     // bit sz * 8 + sy, group-uniform
#pragma unroll
    for (int sz = 0; sz < 8; ++sz) {
      const bool ok = !((gyl + __shfl(gzl, sz, GL)) * T.h2 > top.lim_d);
      const uint32_t m8 = (uint32_t)((__ballot(ok) >> gshift) & 0xFFull);
      if (sz < 4) live_lo |= m8 << (8 * sz); else live_hi |= m8 << (8 * (sz - 4));
    }
    live_lo &= N[PT_NODE_ROWMASK];                         // ... and are not empty (the node's row mask, next to its header)
    live_hi &= N[PT_NODE_ROWMASK + 1];
    // Sweep: first the target's own sub-cell alone (so that the bound is tight before anything else is looked at), then the live
    // rows of eight sub-cells; the own sub-cell is skipped when its row comes by.  One code path serves both, so that the scan and
    // the descent are instantiated once per level.  A row's nine starts and eight child links are fetched by the eight lanes in
    // ONE go (a single memory latency per row) and handed round by shuffles.
    bool first = inside;
    while (first || (live_lo | live_hi)) {                  // group-uniform
      int r2, xa, xb;
      if (first) { r2 = (int)(own >> 3); xa = xb = (int)(own & 7u); }
      else {
        if (live_lo) { r2 = __ffs((int)live_lo) - 1; live_lo &= live_lo - 1; }
        else { r2 = 32 + __ffs((int)live_hi) - 1; live_hi &= live_hi - 1; }
        const double t2 = __shfl(gyl, r2 & 7, GL) + __shfl(gzl, r2 >> 3, GL);
        if (t2 * T.h2 > top.lim_d) continue;                // the bound may have tightened since the ballots
        xa = 0; xb = 7;
        while (xa <= xb && (__shfl(gxl, xa, GL) + t2) * T.h2 > top.lim_d) ++xa;
        while (xb >= xa && (__shfl(gxl, xb, GL) + t2) * T.h2 > top.lim_d) --xb;
        if (xa > xb) continue;
      }
      const bool sweep = !first;
      first = false;
      const uint32_t stl = N[PT_NODE_START + r2 * 8 + top.L], end8 = N[PT_NODE_START + r2 * 8 + 8];
      uint32_t chl = 0;
      if constexpr (DEPTH + 1 < PT_REFINE_DEPTH) chl = N[PT_NODE_CHILD + r2 * 8 + top.L];
      // leaf sub-cells next to each other are one contiguous run of records, scanned in one go; a sub-cell that is a node, the
      // own sub-cell (already done) and the end of the row cut the run
      uint32_t run_s = 0, run_e = 0;
      for (int x = xa; x <= xb + 1; ++x) {
        const uint32_t sub = (uint32_t)(r2 * 8 + x);
        uint32_t child = 0;
        bool cut = x > xb || (sweep && sub == own);
        if constexpr (DEPTH + 1 < PT_REFINE_DEPTH) {
          if (!cut) {
            child = (uint32_t)__shfl((int)chl, x, GL);
            if (child & PT_LEAF_TRUNC) child = 0u;          // a leaf of identical points with its lowest indices in front (pt_common.h): scanned whole here, which is exact too
            cut = child != 0u;
          }
        }
        if (!cut) {
          if (run_e == run_s) run_s = (uint32_t)__shfl((int)stl, x, GL);
          run_e = x < 7 ? (uint32_t)__shfl((int)stl, x + 1, GL) : end8;
          continue;
        }
        if (run_e > run_s) range(run_s, run_e);
        run_s = run_e = 0;
        if constexpr (DEPTH + 1 < PT_REFINE_DEPTH) { if (child) node<DEPTH + 1>(child); }
      }
    }
  }
};

// Heavy cells met by the group kernel (HIER builds) are not scanned on the spot but remembered -- their key, in the group's slice of
// an LDS list -- and descended into at ONE place of the kernel (the descent is three levels of inlined code: one copy is enough).
constexpr int PEND_CAP = 32;
struct Pending {
  uint32_t* slot;          // this group's PEND_CAP words of LDS
  uint32_t n;              // group-uniform
  uint32_t thr;            // cells with more points than this may carry a node (0xFFFFFFFF: the grid has none)
  __device__ bool heavy(uint32_t s, uint32_t e) const { return e - s > thr; }
  __device__ bool push(uint32_t key, int lane) {           // false: list full, the caller scans the cell linearly (exact, only slower)
    if (n >= (uint32_t)PEND_CAP) return false;
    if (lane == 0) slot[n] = key;
    ++n;
    return true;
  }
};

// generic walk of cells [xa, xb] x {y} x {z} (inside the grid): prune by the box lower bound, then scan block by block
template <class Rec, int KPL>
__device__ void scan_row_generic(const GridParams& gp, const Rec* __restrict__ src, const uint32_t* __restrict__ cs, const TargetGeom& T,
                                 TopList<KPL>& top, int gshift, int xa, int xb, int y, int z, Pending* pend = nullptr) {
  const double gy = T.gap(1, y, y), gz = T.gap(2, z, z);
  const double s2 = gy * gy + gz * gz;
  if (s2 * T.h2 > top.lim_d) return;
  while (xa < xb) { const double g = T.gap(0, xa, xa); if ((g * g + s2) * T.h2 > top.lim_d) ++xa; else break; }
  while (xb > xa) { const double g = T.gap(0, xb, xb); if ((g * g + s2) * T.h2 > top.lim_d) --xb; else break; }
  { const double g = T.gap(0, xa, xb); if ((g * g + s2) * T.h2 > top.lim_d) return; }
  for (int bx = xa >> 3; bx <= (xb >> 3); ++bx) {
    const int pa = max(xa, bx << 3), pb = min(xb, (bx << 3) + 7);
    const uint32_t key = cell_key(gp, pa, y, z);
    uint32_t s = cs[key], e = cs[key + (uint32_t)(pb - pa) + 1u];
    if (pend && pend->heavy(s, e)) {
      // a run that may hold heavy cells: those are set aside for the descent, the light ones in between are scanned here
      const uint32_t e_all = e;
      e = s;
      for (int i = 0; i <= pb - pa; ++i) {
        const uint32_t s1 = cs[key + (uint32_t)i], e1 = cs[key + (uint32_t)i + 1u];
        const bool defer = pend->heavy(s1, e1) && pend->push(key + (uint32_t)i, top.L);
        if (!defer) { e = e1; continue; }
        for (uint32_t base = s; base < e; base += GL) {
          const uint32_t p = base + (uint32_t)top.L;
          double d = INFINITY;
          uint32_t id = PT_NOIDX_U;
          if (p < e) { const Rec r = src[p]; d = dist2(T.q, r); id = r.id; }
          top.offer(d, id, gshift);
        }       // (the light run collected so far)
        s = e = e1;
      }
      (void)e_all;
    }
    for (uint32_t base = s; base < e; base += GL) {
      const uint32_t p = base + (uint32_t)top.L;
      double d = INFINITY;
      uint32_t id = PT_NOIDX_U;
      if (p < e) { const Rec r = src[p]; d = dist2(T.q, r); id = r.id; }
      top.offer(d, id, gshift);
    }
  }
}

template <class Rec> struct Batch { static constexpr int N = sizeof(Rec) == 16 ? 4 : 2; };   // steps requested at once

// the cells of one row that survive pruning, flattened: virtual position v -> record index
struct RowPlan {
  uint32_t a0, a1, a2;     // first record of the three cells
  uint32_t n0, n01, T;     // prefix sums of the surviving cells' sizes: n0, n0+n1, n0+n1+n2
  __device__ uint32_t addr(uint32_t v) const { return v < n0 ? a0 + v : (v < n01 ? a1 + (v - n0) : a2 + (v - n01)); }
};

template <class Rec, int KPL, bool HIER>
__global__ __launch_bounds__(WG, HIER ? (KPL == 4 ? 3 : 4) : 1) void knn_kernel(GridParams gp, const Rec* __restrict__ src, const uint32_t* __restrict__ cs,
                                                 const Rec* __restrict__ tgt, uint32_t m, int k, const double* __restrict__ bound2,
                                                 uint32_t* __restrict__ out_idx, double* __restrict__ out_d2,
                                                 const uint32_t* __restrict__ list, const uint32_t* __restrict__ list_n, HierArgs ha) {
  constexpr int NB = Batch<Rec>::N;
  __shared__ uint32_t pend_lds[HIER ? (WG / GL) * PEND_CAP : 1];
  const uint32_t gid = (blockIdx.x * WG + threadIdx.x) / GL;
  if (gid >= (list ? *list_n : m)) return;    // whole groups leave together
  const int L = threadIdx.x & (GL - 1);
  const int gshift = (threadIdx.x & 63) & ~(GL - 1);
  const Rec tr = tgt[list ? list[gid] : gid];  // `list`: positions (in the sorted target array) left over by the tile kernel
#ifdef PT_VISITS
  const unsigned long long pt_t0 = wall_clock64();
#endif
  TargetGeom T;
  T.q[0] = (double)tr.x; T.q[1] = (double)tr.y; T.q[2] = (double)tr.z;
  T.h2 = gp.h * gp.h;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    T.u[a] = (T.q[a] - gp.bbmin[a]) * gp.inv_h;
    T.c[a] = (int)fmin(fmax(T.u[a], 0.0), (double)(gp.dim[a] - 1));
  }
  TopList<KPL> top;
  const double bnd0 = bound2 ? bound2[tr.id] : INFINITY;
  if (bnd0 < 0.0) {            // a negative bound: this target wants nothing from this cloud (pt_stream_query's "not this chunk") -- group-uniform
    const size_t row0 = (size_t)tr.id * (size_t)k;
    for (int e = L; e < k; e += GL) { out_idx[row0 + e] = PT_NOIDX_U; if (out_d2) out_d2[row0 + e] = INFINITY; }
    return;
  }
  top.init(L, k, bnd0);
  const int c0 = T.c[0], c1 = T.c[1], c2 = T.c[2];
  Pending pend{&pend_lds[HIER ? (threadIdx.x / GL) * PEND_CAP : 0], 0u, HIER ? ha.thr : 0xFFFFFFFFu};
  Pending* const pp = HIER ? &pend : nullptr;

  // ---- ring 1, phase A: cell ranges of the 9 rows.  Every lane looks up the centre row (row 0); lane L also
  //      looks up row L+1.  12 independent loads per lane, one memory latency for the whole neighbourhood.
  uint32_t cS[3], cE[3], mS[3], mE[3];          // centre row / my row: [start, end) of cells x = c0-1, c0, c0+1
  {
    const int my = L + 1;
    const int y = c1 + row_dy(my), z = c2 + row_dz(my);
    const bool rowok = y >= 0 && y < gp.dim[1] && z >= 0 && z < gp.dim[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int x = c0 - 1 + j;
      const bool xok = x >= 0 && x < gp.dim[0];
      cS[j] = cE[j] = mS[j] = mE[j] = 0;
      if (xok) {
        const uint32_t kc = cell_key(gp, x, c1, c2);
        cS[j] = cs[kc]; cE[j] = cs[kc + 1];
        if (rowok) {
          const uint32_t km = cell_key(gp, x, y, z);
          mS[j] = cs[km]; mE[j] = cs[km + 1];
        }
      }
    }
  }

  if (ha.heavy) {                                           // group-uniform
    uint32_t pop = (mE[0] - mS[0]) + (mE[1] - mS[1]) + (mE[2] - mS[2]);
    uint32_t big = max(max(mE[0] - mS[0], mE[1] - mS[1]), mE[2] - mS[2]);
    pop += (uint32_t)__shfl_xor((int)pop, 1, GL); pop += (uint32_t)__shfl_xor((int)pop, 2, GL); pop += (uint32_t)__shfl_xor((int)pop, 4, GL);
    big = max(big, (uint32_t)__shfl_xor((int)big, 1, GL)); big = max(big, (uint32_t)__shfl_xor((int)big, 2, GL)); big = max(big, (uint32_t)__shfl_xor((int)big, 4, GL));
    pop += (cE[0] - cS[0]) + (cE[1] - cS[1]) + (cE[2] - cS[2]);
    big = max(big, max(max(cE[0] - cS[0], cE[1] - cS[1]), cE[2] - cS[2]));
    if (pop >= ha.wave_min) {
      // marked by position in the sorted target array (2: a refined cell among the 27 -- those need the descending variant of the
      // wave kernel, which runs at half the occupancy); the marks are compacted IN ORDER afterwards, so that the wave kernel meets
      // the targets cell by cell and neighbours share what they read through L2
      if (L == 0) ha.heavy[list ? list[gid] : gid] = (HIER && big > ha.thr) ? 2u : 1u;
      return;                                               // whole groups leave together
    }
  }

  // plan of row r under the current limit: which cells survive, where their records are
  auto make_plan = [&](int r) -> RowPlan {
    RowPlan P;
    P.a0 = P.a1 = P.a2 = 0; P.n0 = P.n01 = P.T = 0;
    const int y = c1 + row_dy(r), z = c2 + row_dz(r);
    if (y < 0 || y >= gp.dim[1] || z < 0 || z >= gp.dim[2]) return P;
    const double gy = T.gap(1, y, y), gz = T.gap(2, z, z);
    const double s2 = gy * gy + gz * gz;
    if (s2 * T.h2 > top.lim_d) return P;
    uint32_t S[3], E[3];
    if (r == 0) {
#pragma unroll
      for (int j = 0; j < 3; ++j) { S[j] = cS[j]; E[j] = cE[j]; }
    } else {
#pragma unroll
      for (int j = 0; j < 3; ++j) { S[j] = __shfl(mS[j], r - 1, GL); E[j] = __shfl(mE[j], r - 1, GL); }
    }
    uint32_t n[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int x = c0 - 1 + j;
      const double g = T.gap(0, x, x);
      n[j] = ((g * g + s2) * T.h2 > top.lim_d) ? 0u : (E[j] - S[j]);   // cells outside the grid have S == E == 0
    }
    if constexpr (HIER) {
      // heavy cells leave the flat plan for the pending list; the middle cell first, so that in row 0 (planned first) the target's
      // own cell heads the list and its descent tightens the bound for all the others
#pragma unroll
      for (int jj = 0; jj < 3; ++jj) {
        const int j = jj == 0 ? 1 : (jj == 1 ? 0 : 2);
        if (n[j] && pend.heavy(S[j], E[j]) && pend.push(cell_key(gp, c0 - 1 + j, y, z), L)) n[j] = 0u;
      }
    }
    P.a0 = S[0]; P.a1 = S[1]; P.a2 = S[2];
    P.n0 = n[0]; P.n01 = n[0] + n[1]; P.T = P.n01 + n[2];
    return P;
  };
  auto request = [&](const RowPlan& P, Rec (&R)[NB]) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const uint32_t v = b * GL + L;
      if (v < P.T) R[b] = src[P.addr(v)];
    }
  };
  auto rank_batch = [&](const RowPlan& P, const Rec (&R)[NB]) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      if ((uint32_t)(b * GL) < P.T) {            // group-uniform
        const uint32_t v = b * GL + L;
        double d = INFINITY;
        uint32_t id = PT_NOIDX_U;
        if (v < P.T) { d = dist2(T.q, R[b]); id = R[b].id; }
        top.offer(d, id, gshift);
      }
    }
    for (uint32_t vb = NB * GL; vb < P.T; vb += GL) {   // rows longer than one batch (dense cells)
      const uint32_t v = vb + L;
      double d = INFINITY;
      uint32_t id = PT_NOIDX_U;
      if (v < P.T) { const Rec r = src[P.addr(v)]; d = dist2(T.q, r); id = r.id; }
      top.offer(d, id, gshift);
    }
  };

  // ---- ring 1, phase B: rows in centre-first order, the next row's records in flight while this one is ranked
  {
    Rec Rn[NB];
    RowPlan Pn = make_plan(0);
    request(Pn, Rn);
#pragma unroll 1
    for (int r = 0; r < 9; ++r) {
      Rec Rc[NB];
      const RowPlan Pc = Pn;
#pragma unroll
      for (int b = 0; b < NB; ++b) Rc[b] = Rn[b];
      if (r + 1 < 9) {
        Pn = make_plan(r + 1);        // planned under the limit as it is now: conservative, never wrong
        request(Pn, Rn);
      }
      rank_batch(Pc, Rc);
    }
  }

  // ---- rings >= 2: only while something outside the scanned box can still beat the limit ---------------------------
  const int ring_limit = max(PT_RING_LIMIT, (int)cbrtf(0.07f * (float)gp.nblocks));
  for (int r = 1;; ++r) {
    if constexpr (HIER) {
      // the heavy cells of the ring just scanned (ring 1 on the first pass): descended into here, the ONLY place -- before the
      // termination test, which therefore sees the bound they leave
      if (pend.n) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");        // lane 0's list entries, for the whole group
        __builtin_amdgcn_wave_barrier();
        HierScan<Rec, KPL> H{gp, src, ha.nodes, T, top, gshift};
        for (uint32_t i = 0; i < pend.n; ++i) {
          const uint32_t key = pend.slot[i];
          int x, y, z;
          pt_decode_cell(gp, key, x, y, z);
          const double gx = T.gap(0, x, x), gy = T.gap(1, y, y), gz = T.gap(2, z, z);
          if ((gx * gx + gy * gy + gz * gz) * T.h2 > top.lim_d) continue;      // the bound has tightened since the cell was set aside
          const uint32_t nid = ha.cell_node[key];
          if (nid) H.template node<0>(nid); else H.range(cs[key], cs[key + 1]);   // (no node: the table was full when the cell asked)
        }
        pend.n = 0;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");        // the next ring's entries stay behind these reads
        __builtin_amdgcn_wave_barrier();
      }
    }
    // every unscanned point lies beyond one of the box faces that still has cells behind it
    bool covered = true;
    double dout = INFINITY;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int lo = T.c[a] - r, hi = T.c[a] + r;
      if (lo > 0) { covered = false; dout = fmin(dout, T.u[a] - (double)lo); }
      if (hi < gp.dim[a] - 1) { covered = false; dout = fmin(dout, (double)(hi + 1) - T.u[a]); }
    }
    if (covered) break;
    dout = fmax(dout - PT_CELL_EPS, 0.0);
    if (dout * dout * T.h2 > top.lim_d) break;
    if (r >= ring_limit) {
      // Far from the points (a stray target, a gap in the cloud): walking ever larger, mostly empty shells costs O(r^2)
      // per ring.  Sweep the BLOCKS instead -- skip the empty ones, prune the others by their box, scan what is left --
      // starting the list again so that no point is offered twice.  O(blocks) per such target, exact like the walk; taken
      // once the walk has cost about as much as the sweep will (ring_limit^3 ~ blocks / 14).
      top.init(L, k, bound2 ? bound2[tr.id] : INFINITY);
      const uint32_t nb = (uint32_t)gp.nblocks;
      for (uint32_t b0 = 0; b0 < nb; b0 += GL) {
        const uint32_t b = b0 + (uint32_t)L;             // lane L looks at block b0 + L
        uint32_t bs_ = 0, be_ = 0;
        if (b < nb) { bs_ = cs[(size_t)b * PT_BLOCK_CELLS]; be_ = cs[((size_t)b + 1) * PT_BLOCK_CELLS]; }
        bool want = be_ > bs_;
        if (want) {
          const uint32_t macro = b >> 9, m9 = b & 511u;
          const int bx = (int)(macro % (uint32_t)gp.mdim[0]) * 8 + (int)((m9 & 1u) | ((m9 >> 2) & 2u) | ((m9 >> 4) & 4u));
          const int by = (int)((macro / (uint32_t)gp.mdim[0]) % (uint32_t)gp.mdim[1]) * 8 + (int)(((m9 >> 1) & 1u) | ((m9 >> 3) & 2u) | ((m9 >> 5) & 4u));
          const int bz = (int)(macro / (uint32_t)(gp.mdim[0] * gp.mdim[1])) * 8 + (int)(((m9 >> 2) & 1u) | ((m9 >> 4) & 2u) | ((m9 >> 6) & 4u));
          const double gx = T.gap(0, bx * 8, bx * 8 + 7), gy = T.gap(1, by * 8, by * 8 + 7), gz = T.gap(2, bz * 8, bz * 8 + 7);
          want = !((gx * gx + gy * gy + gz * gz) * T.h2 > top.lim_d);
        }
        uint32_t mask = (uint32_t)((__ballot(want) >> gshift) & 0xFFull);      // the group's eight verdicts
        while (mask) {                                    // group-uniform
          const int j = __ffs((int)mask) - 1;
          mask &= mask - 1;
          const uint32_t s0 = (uint32_t)__shfl(bs_, gshift + j), e0 = (uint32_t)__shfl(be_, gshift + j);
          for (uint32_t base = s0; base < e0; base += GL) {
            const uint32_t p = base + (uint32_t)top.L;
            double d = INFINITY;
            uint32_t id = PT_NOIDX_U;
            if (p < e0) { const Rec r = src[p]; d = dist2(T.q, r); id = r.id; }
            top.offer(d, id, gshift);
          }
        }
      }
      break;
    }
    const int rr = r + 1;                      // scan the shell box(rr) \ box(rr-1)
    const int x0 = max(c0 - rr, 0), x1 = min(c0 + rr, gp.dim[0] - 1);
    const int y0 = max(c1 - rr, 0), y1 = min(c1 + rr, gp.dim[1] - 1);
    const int z0 = max(c2 - rr, 0), z1 = min(c2 + rr, gp.dim[2] - 1);
    for (int z = z0; z <= z1; ++z)
      for (int y = y0; y <= y1; ++y) {
        const bool shell = (z == c2 - rr) || (z == c2 + rr) || (y == c1 - rr) || (y == c1 + rr);
        if (shell) scan_row_generic<Rec, KPL>(gp, src, cs, T, top, gshift, x0, x1, y, z, pp);
        else {
          if (c0 - rr >= 0) scan_row_generic<Rec, KPL>(gp, src, cs, T, top, gshift, c0 - rr, c0 - rr, y, z, pp);
          if (c0 + rr <= gp.dim[0] - 1) scan_row_generic<Rec, KPL>(gp, src, cs, T, top, gshift, c0 + rr, c0 + rr, y, z, pp);
        }
      }
  }

  const size_t row = (size_t)tr.id * (size_t)k;
#pragma unroll
  for (int j = 0; j < KPL; ++j) {
    const int e = L * KPL + j;
    if (e < k) {
      out_idx[row + e] = top.li[j];
      if (out_d2) out_d2[row + e] = top.ld[j];
    }
  }
#ifdef PT_VISITS
  __builtin_amdgcn_wave_barrier();
  if (out_d2 && L == GL - 1) {                                              // (results are garbage in these columns)
    out_d2[row + k - 1] = (double)top.nv * GL;
    if (k >= 4) { out_d2[row + k - 2] = (double)(wall_clock64() - pt_t0); out_d2[row + k - 3] = (double)pt_t0; out_d2[row + k - 4] = (double)(blockIdx.x * 4u + threadIdx.x / 64u); }
  }
#endif
}

}  // namespace

template <class Rec>
void pt_launch_knn(const GridParams& gp, const Rec* src, const uint32_t* cell_start, const Rec* tgt, uint32_t m, int k, const double* bound2,
                   uint32_t* out_idx, double* out_d2, const uint32_t* list, const uint32_t* list_n, hipStream_t s, uint8_t* heavy, uint32_t wave_min) {
  if (!m) return;
  const uint32_t nwg = (uint32_t)(((uint64_t)m * GL + WG - 1) / WG);
  const HierArgs ha{nullptr, nullptr, 0xFFFFFFFFu, heavy, wave_min};
  if (k <= 8)
    hipLaunchKernelGGL((knn_kernel<Rec, 1, false>), dim3(nwg), dim3(WG), 0, s, gp, src, cell_start, tgt, m, k, bound2, out_idx, out_d2, list, list_n, ha);
  else if (k <= 16)
    hipLaunchKernelGGL((knn_kernel<Rec, 2, false>), dim3(nwg), dim3(WG), 0, s, gp, src, cell_start, tgt, m, k, bound2, out_idx, out_d2, list, list_n, ha);
  else
    hipLaunchKernelGGL((knn_kernel<Rec, 4, false>), dim3(nwg), dim3(WG), 0, s, gp, src, cell_start, tgt, m, k, bound2, out_idx, out_d2, list, list_n, ha);
}
template void pt_launch_knn<RecF>(const GridParams&, const RecF*, const uint32_t*, const RecF*, uint32_t, int, const double*, uint32_t*, double*,
                                  const uint32_t*, const uint32_t*, hipStream_t, uint8_t*, uint32_t);
template void pt_launch_knn<RecD>(const GridParams&, const RecD*, const uint32_t*, const RecD*, uint32_t, int, const double*, uint32_t*, double*,
                                  const uint32_t*, const uint32_t*, hipStream_t, uint8_t*, uint32_t);

template <class Rec>
void pt_launch_knn_hier(const GridParams& gp, const Rec* src, const uint32_t* cell_start, const uint32_t* cell_node, const uint32_t* nodes, uint32_t node_thr,
                        const Rec* tgt, uint32_t m, int k, const double* bound2, uint32_t* out_idx, double* out_d2, const uint32_t* list,
                        const uint32_t* list_n, hipStream_t s, uint8_t* heavy, uint32_t wave_min) {
  if (!m) return;
  const uint32_t nwg = (uint32_t)(((uint64_t)m * GL + WG - 1) / WG);
  const HierArgs ha{cell_node, nodes, node_thr, heavy, wave_min};
  if (k <= 8)
    hipLaunchKernelGGL((knn_kernel<Rec, 1, true>), dim3(nwg), dim3(WG), 0, s, gp, src, cell_start, tgt, m, k, bound2, out_idx, out_d2, list, list_n, ha);
  else if (k <= 16)
    hipLaunchKernelGGL((knn_kernel<Rec, 2, true>), dim3(nwg), dim3(WG), 0, s, gp, src, cell_start, tgt, m, k, bound2, out_idx, out_d2, list, list_n, ha);
  else
    hipLaunchKernelGGL((knn_kernel<Rec, 4, true>), dim3(nwg), dim3(WG), 0, s, gp, src, cell_start, tgt, m, k, bound2, out_idx, out_d2, list, list_n, ha);
}
template void pt_launch_knn_hier<RecF>(const GridParams&, const RecF*, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t, const RecF*, uint32_t, int, const double*,
                                       uint32_t*, double*, const uint32_t*, const uint32_t*, hipStream_t, uint8_t*, uint32_t);
template void pt_launch_knn_hier<RecD>(const GridParams&, const RecD*, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t, const RecD*, uint32_t, int, const double*,
                                       uint32_t*, double*, const uint32_t*, const uint32_t*, hipStream_t, uint8_t*, uint32_t);
