// pt_knn_wave.hip -- the wave kernel of the exact k-NN search (pt_knn_common.h): one wave per target, for gfx950 (MI355X).
#include "pt_knn_common.h"
#include <type_traits>

using namespace pt_knn;

namespace {

// =====================================================================================================================
// Wave kernel: ONE WAVE (64 lanes) PER TARGET -- the targets of dense neighbourhoods (clouds with strong density contrast).
//
// Why a third kernel: the group kernel keeps eight targets per wave in lockstep, and in a dense cell every step of eight records
// ends in the insertion path for SOME group (k ln(n / k) insertions per target, ~100 VALU instructions each at k = 32, seven
// groups idle meanwhile): measured on the clustered generator it looks at 1e11 records/s whatever the index offers.  Here the
// whole wave serves one target: 64 records per step with wave-uniform control flow; the k best live one entry per lane -- an
// unsorted pool whose k-th smallest key, found by pivoting, is the scalar limit (see WaveScan: THE LIST) -- and are sorted once, at
// the end.  Cells, shells, blocks and the rows of refined nodes are looked up 64 at a time, one per lane.
// Same order, same bounds, same results as the group kernel (exact); k <= 32 (PT_MAX_K).
constexpr int WV_RING_MAX = 31;          // shells are walked up to this ring at most (then the blocks are swept)
constexpr uint32_t WV_RUN = 16;          // consecutive workgroups (64 targets) that share an XCD

// key_lt without short-circuit evaluation: no branches around the comparisons (the compiler turns `a < b || (a == b && i < j)` on
// per-lane values into three exec-masked blocks)
__device__ inline bool key_lt_flat(double ad, uint32_t ai, double bd, uint32_t bi) {
  const bool lt = ad < bd, eq = ad == bd, il = ai < bi;
  return lt | (eq & il);
}
__device__ inline double readlane_f64(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ inline uint32_t readlane_u32(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }
// lane l of v := the wave-uniform value x (no builtin for it in this compiler).  M0 is free in the kernels that use this (no LDS-DMA,
// no GWS): the compiler's warning about the clobber is silenced.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ inline uint32_t writelane_u32(uint32_t v, uint32_t x, int l) {
  asm volatile("s_mov_b32 m0, %2\n\tv_writelane_b32 %0, %1, m0" : "+v"(v) : "s"(x), "s"(l) : "m0");     // (one SGPR per VOP3: the lane goes through M0)
  return v;
}
#pragma clang diagnostic pop

// attribute blend fused into the wave kernel (attr == null: none): the table, its length, the mode and the two outputs
struct WaveBlend { const Attr* attr; uint32_t n_attr; int mode; float* rgb_out; float* nrm_out; };
template <class Rec>
struct WaveScan {
  const Rec* __restrict__ src;
  const uint32_t* __restrict__ nodes;
  double q[3], u[3], h2;       // the target, its position in cell units, squared cell side: wave-uniform
  double ld;                   // my entry of the pool of the k best (+inf, NOIDX: none); after finish(): lane i holds rank i
  uint32_t li;
  double lim_d, bnd_d;         // acceptance limit = min(entry of rank k-1, caller's bound): wave-uniform
  uint32_t lim_i;
  // fp32 clouds: a step whose 64 records are all beyond the limit ALREADY IN FP32 (most steps of a long scan) skips the fp64 metric
  // and everything after it.  d32 <= d (1 + 2^-21) (dist2_f32), so a record with d <= lim_d has d32 <= lim32 := lim_d (1 + 2^-20)
  // rounded to float (nearest: 2^-24 at most the wrong way), plus a slack for fp32 underflow; +inf stays +inf.
#ifdef PT_NOPRE32
  static constexpr bool PRE32 = false;                   // (A/B builds: tools/sweep_pend.sh)
#else
  static constexpr bool PRE32 = IsRecF<Rec>::value;
#endif
  float qf[3], lim32;
  __device__ __forceinline__ void set_lim32() { lim32 = (float)(lim_d * 1.00000095367431640625) + 1e-30f; }
  int k, lane;
  // candidates set aside: this wave's 64 slots in LDS and how many are taken (wave-uniform); see offer()
  uint4* pend;                 // slot: (d2 low word, d2 high word, index, -)
  uint32_t npend;
#ifdef PT_VISITS
  uint32_t nv = 0, nn = 0, nmerge = 0;     // instrumented build: steps of 64 records, nodes entered, selections (sort-merges until round 4)
#endif

  // THE LIST (round 4, second form).  Rounds 2 - 4 kept the k best SORTED across the lanes and paid a 27-stage bitonic sort-merge (361 VALU
  // instructions) for every 16 - 48 candidates, 4.5 of them per sheet target of config 5 -- 46 % of a kernel that is bound by VALU issue (32
  // more fp32 instructions per step of 64 records cost their full 3 cycles each: tools/ab_c5.sh, -DPT_WABLATE).  Nothing needs the order
  // before the end: a scan needs the k-th smallest key, as its limit, and somewhere to keep the k best.  So the lanes hold an UNSORTED POOL
  // (an empty lane: +inf, NOIDX), candidates collect in the wave's 64 LDS slots as before, and a flush
  //   places them into free lanes (lane j, the r-th free one, reads slot r: one prefix count, two LDS reads),
  //   selects the k-th smallest key of the pool by pivoting (a lane's key against all: one ballot and a count per probe, ~ 8 probes of ~ 6
  //   VALU + scalar work on random data; every decision is scalar), makes it the limit and empties the lanes beyond it:
  // ~ 70 VALU instructions instead of 361.  One 21-stage sort of the pool at the very end puts rank i into lane i for the output.
  uint32_t npool;              // entries in the pool (wave-uniform)
  __device__ void reset() { ld = INFINITY; li = PT_NOIDX_U; lim_d = bnd_d; lim_i = PT_NOIDX_U; npend = 0; npool = 0; set_lim32(); }
  // one step's 64 records: fp32 clouds look at the fp32 distance first
  __device__ __forceinline__ void step(const Rec& r, bool have) {
    if constexpr (PRE32) {
      const bool near32 = have & (dist2_f32(qf[0], qf[1], qf[2], r) <= lim32);      // (no short circuit: a branch around six instructions costs more than they do)
      if (!ballot64(near32)) return;                        // wave-uniform
    }
    offer(dist2(q, r), r.id, have);                         // (lanes without a record computed on whatever record their registers held: `have` keeps them out)
  }
  // Many candidates at once (the first steps of a target: with fewer than k points seen every record is one): sort the 64 candidate
  // slots across the lanes (bitonic, 21 exchange stages), take the 64 smallest of list and candidates (list[i] against candidate
  // [63 - i]) and sort that bitonic sequence (6 stages) -- ~500 instructions whatever the number of candidates, against ~35 for
  // each one-by-one insertion.  Keys are distinct (ids) except the empty slots (+inf, NOIDX), whose order does not matter.
  // The exchanges never touch the LDS: partner lane ^ 1, ^ 2 by DPP quad permutes, ^ 4 by two bank-masked row shifts, ^ 8 by a row
  // rotation, ^ 16 and ^ 32 by gfx950's v_permlane16_swap / v_permlane32_swap (both copies of the value go in; each lane picks the
  // one that holds its partner's).  With ds_bpermute every one of the 27 stages was an LDS round trip.
  template <int J>
  __device__ __forceinline__ uint32_t xor_lane(uint32_t x) const {
    if constexpr (J == 1) return dpp_u32<0xB1>(x);                                       // quad_perm [1,0,3,2]
    else if constexpr (J == 2) return dpp_u32<0x4E>(x);                                  // quad_perm [2,3,0,1]
    else if constexpr (J == 4) {
      const int t = __builtin_amdgcn_update_dpp((int)x, (int)x, 0x104, 0xF, 0x5, false);  // row_shl:4 into lanes 0-3, 8-11 of a row
      return (uint32_t)__builtin_amdgcn_update_dpp(t, (int)x, 0x114, 0xF, 0xA, false);    // row_shr:4 into lanes 4-7, 12-15
    } else if constexpr (J == 8) return (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x128, 0xF, 0xF, false);   // row_ror:8
    else if constexpr (J == 16) { const auto r = __builtin_amdgcn_permlane16_swap(x, x, false, false); return (lane & 16) ? r[0] : r[1]; }
    else { const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false); return (lane & 32) ? r[0] : r[1]; }
  }
  template <int J>
  __device__ __forceinline__ void exchange(double& xd, uint32_t& xi, bool keep_min) const {
    const uint32_t plo = xor_lane<J>((uint32_t)__double2loint(xd)), phi = xor_lane<J>((uint32_t)__double2hiint(xd)), pi = xor_lane<J>(xi);
    const double pd = __hiloint2double((int)phi, (int)plo);
    // keep_min: take the partner's if it is smaller; else take it unless it is smaller (equal keys -- two empty slots -- swap to no effect)
    if (key_lt_flat(pd, pi, xd, xi) == keep_min) { xd = pd; xi = pi; }
  }
  // the exchange stages of one bitonic block size k2 (partners ^ k2/2 ... ^ 1); k2 is a constant wherever this is used
  __device__ __forceinline__ void stages(double& xd, uint32_t& xi, int k2, int l) const {
    const bool up = (l & k2) == 0;
    if (k2 > 32) exchange<32>(xd, xi, ((l & 32) == 0) == up);          // wave-uniform tests
    if (k2 > 16) exchange<16>(xd, xi, ((l & 16) == 0) == up);
    if (k2 > 8) exchange<8>(xd, xi, ((l & 8) == 0) == up);
    if (k2 > 4) exchange<4>(xd, xi, ((l & 4) == 0) == up);
    if (k2 > 2) exchange<2>(xd, xi, ((l & 2) == 0) == up);
    exchange<1>(xd, xi, ((l & 1) == 0) == up);
  }
#ifndef PT_PEND_FLUSH
#define PT_PEND_FLUSH 24
#endif
  static constexpr int PEND_FLUSH = PT_PEND_FLUSH;
  // The flush is ONE function in the code object (as the sort-merge was), values in and values out -- nothing of the scan's state goes through
  // memory: inlined at every place a scan may flush (65 of them in the descending variant) it pushed other members out of line, and a member
  // called as a function takes `this`, i.e. the whole scan state moves to scratch memory (26 -> 84 ms for that launch at config 5's shape).
  //   place:  slots [done, done + take) -> the first `take` free lanes (lane j, the r-th free one, reads slot r)
  //   select: the k-th smallest key of the pool by pivoting -- the lowest / the highest lane in question by turns (records arrive in memory
  //           order, not by distance; a pool that happens to be sorted one way round still halves every other probe); every decision is
  //           scalar, the set in question shrinks with every probe; the key found is the limit, the lanes beyond it are emptied.
  // Arguments arrive in VGPRs: the wave-uniform ones are said to be uniform, or the loops are compiled for divergent lanes.
  struct Pool { double ld; uint32_t li; uint32_t npool; double lim_d; uint32_t lim_i; uint32_t nsel; };
  __device__ __attribute__((noinline)) static Pool flush_core(double ld_, uint32_t li_, uint32_t npool_, uint32_t n_, uint32_t k_, double lim_d_, uint32_t lim_i_,
                                                              const uint4* pend_) {
    const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)n_), k = (uint32_t)__builtin_amdgcn_readfirstlane((int)k_);
    uint32_t npool = (uint32_t)__builtin_amdgcn_readfirstlane((int)npool_), nsel = 0;
    double lim_d = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(lim_d_)), __builtin_amdgcn_readfirstlane(__double2loint(lim_d_)));
    uint32_t lim_i = (uint32_t)__builtin_amdgcn_readfirstlane((int)lim_i_);
    const uint4* pend = reinterpret_cast<const uint4*>(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)((uint64_t)pend_ >> 32)) << 32) |
                                                       (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint64_t)pend_));
    uint32_t done = 0;
    while (done < n) {                                      // wave-uniform; one trip unless more arrived than there are free lanes
      const uint32_t take = min(n - done, 64u - npool);
      {
        const bool fre = li_ == PT_NOIDX_U && ld_ == INFINITY;
        const unsigned long long F = ballot64(fre);
        const uint32_t r = __builtin_amdgcn_mbcnt_hi((uint32_t)(F >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)F, 0u));
        if (fre && r < take) { const uint4 v = pend[done + r]; ld_ = __hiloint2double((int)v.y, (int)v.x); li_ = v.z; }
        npool += take;
      }
      done += take;
      if (npool >= k) {
        ++nsel;
        unsigned long long A = ballot64(!(li_ == PT_NOIDX_U && ld_ == INFINITY));      // the lanes still in question
        uint32_t need = k;                                                             // rank sought among them
        double td = INFINITY;
        uint32_t ti = PT_NOIDX_U;
        bool found = false;
        int flip = 0;
        while (!found) {                                    // wave-uniform: A and need are scalars; A shrinks with every probe
          const int p = flip ? 63 - __builtin_clzll(A) : __ffsll((long long)A) - 1;
          flip ^= 1;
          const double pd = readlane_f64(ld_, p);
          const uint32_t pi = readlane_u32(li_, p);
          const unsigned long long L = ballot64(key_lt_flat(ld_, li_, pd, pi)) & A;
          const uint32_t cl = (uint32_t)__popcll(L);
          if (need <= cl) A = L;
          else if (need == cl + 1u) { td = pd; ti = pi; found = true; }
          else { need -= cl + 1u; A &= ~L; A &= ~(1ull << p); }
        }
        if (key_lt_flat(td, ti, ld_, li_)) { ld_ = INFINITY; li_ = PT_NOIDX_U; }       // beyond the k-th: out
        npool = k;
        lim_d = td; lim_i = ti;                             // (<= the caller's bound: nothing beyond it was ever offered)
      }
    }
    return Pool{ld_, li_, npool, lim_d, lim_i, nsel};
  }
  __device__ __forceinline__ void flush() {
    if (!npend) return;                                     // wave-uniform
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the slots were written by this wave's own lanes: LDS keeps a wave's order
    __builtin_amdgcn_wave_barrier();
    const Pool r = flush_core(ld, li, npool, npend, (uint32_t)k, lim_d, lim_i, pend);
    npend = 0;
    ld = r.ld; li = r.li;
    npool = (uint32_t)__builtin_amdgcn_readfirstlane((int)r.npool);
    lim_d = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(r.lim_d)), __builtin_amdgcn_readfirstlane(__double2loint(r.lim_d)));
    lim_i = (uint32_t)__builtin_amdgcn_readfirstlane((int)r.lim_i);
    set_lim32();
#ifdef PT_VISITS
    nmerge += (uint32_t)__builtin_amdgcn_readfirstlane((int)r.nsel);
#endif
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // ... and the next round's writes stay behind these reads
    __builtin_amdgcn_wave_barrier();
  }
  // one candidate per lane (d = +inf for lanes without one)
  __device__ __forceinline__ void offer(double d, uint32_t id, bool have) {
    const bool pass = have & key_lt_flat(d, id, lim_d, lim_i) & !(d > bnd_d);
    const unsigned long long mask = ballot64(pass);
    if (!mask) return;                                      // wave-uniform (as every branch below)
    const uint32_t c = (uint32_t)__popcll(mask);
    if (npend + c > 64u) flush();                           // (no room in the slots: the pool takes what is there first)
    const uint32_t slot = npend + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
    if (pass) pend[slot] = make_uint4((uint32_t)__double2loint(d), (uint32_t)__double2hiint(d), id, 0u);      // one 16-byte LDS write
    npend += c;
    if (npend >= (uint32_t)PEND_FLUSH) flush();
  }
  // the end of a search: rank i into lane i (the empty lanes sort last)
  // (the pool's <= k entries are gathered in the low lanes first -- through the slots, free by now -- so that the sort spans 8, 16 or 32 lanes:
  //  6, 10 or 15 exchange stages instead of the 21 that 64 lanes take)
  __device__ __forceinline__ void finish() {                // (forced: called as a function it takes `this`, and the whole scan state moves to scratch memory)
    flush();
    const bool has = !(li == PT_NOIDX_U && ld == INFINITY);
    const unsigned long long M = ballot64(has);
    const uint32_t r = __builtin_amdgcn_mbcnt_hi((uint32_t)(M >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)M, 0u));
    if (has) pend[r] = make_uint4((uint32_t)__double2loint(ld), (uint32_t)__double2hiint(ld), li, 0u);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    ld = INFINITY; li = PT_NOIDX_U;
    if ((uint32_t)lane < (uint32_t)__popcll(M)) { const uint4 v = pend[lane]; ld = __hiloint2double((int)v.y, (int)v.x); li = v.z; }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    stages(ld, li, 2, lane); stages(ld, li, 4, lane); stages(ld, li, 8, lane);
    if (k > 8) stages(ld, li, 16, lane);                    // wave-uniform
    if (k > 16) stages(ld, li, 32, lane);
    if (k > 32) stages(ld, li, 64, lane);
  }
  // WPF steps of loads are in flight while a step is ranked: with one, every step of 64 records cost a full memory latency (60 us
  // per target at 25 - 35 steps, measured: the steps' arithmetic is ~0.15 us)
#ifndef PT_WPF
#define PT_WPF 1
#endif
  static constexpr int WPF = PT_WPF;
  // Two register sets take turns (a is ranked while b's load is in flight and the other way round): with one set and a copy per step the
  // compiler waits for a load right after issuing it, to move its words into the set the ranking reads.  For the same reason a 16-byte record
  // travels as ONE four-word value (four consecutive registers, the load's own destination) until the step takes it apart: as a struct of four
  // scalars its index word was given a register elsewhere, and the move into it waited for the load.
  using Vec = typename std::conditional<IsRecF<Rec>::value, float4, Rec>::type;
  __device__ __forceinline__ static Vec loadv(const Rec* p) {
    if constexpr (IsRecF<Rec>::value) return *reinterpret_cast<const float4*>(p); else return *p;
  }
  __device__ __forceinline__ void stepv(const Vec& v, bool have) {
    if constexpr (IsRecF<Rec>::value) { RecF r; r.x = v.x; r.y = v.y; r.z = v.z; r.id = __float_as_uint(v.w); step(r, have); }
    else step(v, have);
  }
  __device__ __forceinline__ void range(uint32_t s, uint32_t e) {
    // (every load is UNCONDITIONAL, its index clamped to the last record: a load under `if (p < e)` merges with the old value behind it, and the
    //  copy that merge needs waits for the load on the spot -- the prefetch gone; lanes beyond the end rank a record twice and `have` discards it)
    if (s >= e) return;                                     // wave-uniform
    const uint32_t last = e - 1u;
    Vec a = loadv(src + min(s + (uint32_t)lane, last)), b;
    for (uint32_t base = s; base < e; base += 128u) {       // wave-uniform trip count, no early exit
      const uint32_t p = base + (uint32_t)lane;
      b = loadv(src + min(p + 64u, last));
#ifdef PT_VISITS
      ++nv;
#endif
      stepv(a, p < e);
      if (base + 64u < e) {                                 // wave-uniform
        a = loadv(src + min(p + 128u, last));
#ifdef PT_VISITS
        ++nv;
#endif
        stepv(b, p + 64u < e);
      }
    }
  }
  // Up to 64 runs of records as ONE stream: lane j brings its run's first record S and length C (0: none); virtual record v of the
  // stream is record v - P[j] of the run j whose prefix interval holds v.  64 records per step whatever the runs' lengths, and the
  // next step's loads are in flight while this one is ranked -- a run costs no memory latency of its own (cell by cell, the 27
  // cells of ring 1 cost 27: 40 us per target, measured).  No pruning inside the stream: the caller decides the runs beforehand.
  __device__ __forceinline__ void stream(uint32_t S, uint32_t C) {
    const uint32_t pin = wave_incl_scan(C), pex = pin - C;
    const uint32_t T = readlane_u32(pin, 63);
    if (!T) return;                                         // wave-uniform
    // my cursor: the run my current virtual record is in -- its interval [c_lo, c_hi) of the stream and its first record.  When a
    // lane leaves its run, ALL lanes search the prefix sums again: a binary search of six shuffles, unrolled, with no loop around it
    // (a `while any lane must advance` loop was turned by the compiler into one that lanes leave one by one, and a shuffle reads
    // nothing from a lane that has left).
    uint32_t c_lo = 0, c_hi = 0, c_S = 0;
    auto locate = [&](uint32_t v) -> uint32_t {             // address of virtual record v (any value for v >= T)
      const bool out = v < T && v >= c_hi;
      if (ballot64(out) != 0ull) {                          // wave-uniform
        int sg = 0;                                         // number of runs that end at or before v
#pragma unroll
        for (int step = 32; step >= 1; step >>= 1) {
          const uint32_t pe = (uint32_t)__shfl((int)pin, sg + step - 1);
          sg += v >= pe ? step : 0;
        }
        sg = min(sg, 63);
        const uint32_t nS = (uint32_t)__shfl((int)S, sg), nlo = (uint32_t)__shfl((int)pex, sg), nhi = (uint32_t)__shfl((int)pin, sg);
        if (out) { c_S = nS; c_lo = nlo; c_hi = nhi; }
      }
      return c_S + (v - c_lo);
    };
    const uint32_t last = T - 1u;                           // two register sets taking turns and unconditional loads, as in range()
    Vec a = loadv(src + locate(min((uint32_t)lane, last))), b;
    for (uint32_t base = 0; base < T; base += 128u) {       // wave-uniform trip count, no early exit
      const uint32_t v = base + (uint32_t)lane;
      b = loadv(src + locate(min(v + 64u, last)));
#ifdef PT_VISITS
      ++nv;
#endif
      stepv(a, v < T);
      if (base + 64u < T) {                                 // wave-uniform
        a = loadv(src + locate(min(v + 128u, last)));
#ifdef PT_VISITS
        ++nv;
#endif
        stepv(b, v + 64u < T);
      }
    }
  }
  __device__ double gap2(int a, double lo, double hi) const {
    const double g = cell_gap(u[a], lo, hi);
    return g * g;
  }
  // refined cell (pt_refine.hip): the 64 rows of sub-cells are tested one per lane, the target's own sub-cell goes first.  Little is
  // kept across a descent into a child (three levels of this are inlined into one another): the node's address, the rows still to
  // visit, the children of the current row -- the header is read again (scalar loads) whenever a row needs its geometry.
  template <int DEPTH>
  __device__ void node(uint32_t nid) {
    const uint32_t* N = nodes + (size_t)((uint32_t)__builtin_amdgcn_readfirstlane((int)nid) - 1u) * PT_NODE_WORDS;     // (wave-uniform: scalar loads)
    uint32_t own = 0xFFFFFFFFu;
    unsigned long long live;
#ifdef PT_VISITS
    ++nn;
#endif
    flush();                                                // the rows are chosen by the limit
    {
      const double* hd = reinterpret_cast<const double*>(N);
      const double ox = hd[0], oy = hd[1], oz = hd[2], inv = hd[3], w = hd[4];
      const double rx = (u[0] - ox) * inv, ry = (u[1] - oy) * inv, rz = (u[2] - oz) * inv;
      if (rx >= 0.0 && rx < 8.0 && ry >= 0.0 && ry < 8.0 && rz >= 0.0 && rz < 8.0) own = (uint32_t)(((int)rz << 6) | ((int)ry << 3) | (int)rx);
      const double fy = (double)(lane & 7), fz = (double)(lane >> 3);          // my row (sy, sz) = (lane & 7, lane >> 3)
      const double s2 = gap2(1, oy + fy * w, oy + (fy + 1.0) * w) + gap2(2, oz + fz * w, oz + (fz + 1.0) * w);
      live = ballot64(!(s2 * h2 > lim_d)) & ((unsigned long long)N[PT_NODE_ROWMASK] | ((unsigned long long)N[PT_NODE_ROWMASK + 1] << 32));
    }
    bool first = own != 0xFFFFFFFFu;
    while (first || live) {                                 // wave-uniform
      int r2, xa, xb;
      if (first) { r2 = (int)(own >> 3); xa = xb = (int)(own & 7u); }
      else {
        r2 = __ffsll((long long)live) - 1;
        live &= live - 1;
        uint32_t again = 0;
        asm volatile("" : "+s"(again));                     // (read the header again rather than keep it across the descents)
        const double* hd = reinterpret_cast<const double*>(N + again);
        const double ox = hd[0], oy = hd[1], oz = hd[2], w = hd[4];
        const double fy = (double)(r2 & 7), fz = (double)(r2 >> 3);
        const double t2 = gap2(1, oy + fy * w, oy + (fy + 1.0) * w) + gap2(2, oz + fz * w, oz + (fz + 1.0) * w);
        if (t2 * h2 > lim_d) continue;                      // the limit has moved since the ballot
        xa = 0; xb = 7;
        while (xa <= xb && (gap2(0, ox + (double)xa * w, ox + (double)(xa + 1) * w) + t2) * h2 > lim_d) ++xa;
        while (xb >= xa && (gap2(0, ox + (double)xb * w, ox + (double)(xb + 1) * w) + t2) * h2 > lim_d) --xb;
        if (xa > xb) continue;
      }
      const bool sweep = !first;
      first = false;
      uint32_t stl = 0, chl = 0;                            // lane x: start of sub-cell x of the row (x = 8: its end) and its child
      if (lane < 9) stl = N[PT_NODE_START + r2 * 8 + lane];
      if (lane < 8) chl = N[PT_NODE_CHILD + r2 * 8 + lane];  // (the last level has no children, but its leaves may carry the identical-points tag)
      // leaf sub-cells next to each other are one contiguous run of records, scanned in one go; a sub-cell that is a node, the own
      // sub-cell (already done) and the end of the row cut the run.  The row's leaves first, then its children one by one.
      uint32_t kids = 0, run_s = 0, run_e = 0;
      for (int x = xa; x <= xb + 1; ++x) {
        bool cut = x > xb || (sweep && (uint32_t)(r2 * 8 + x) == own);
        uint32_t front = 0;                                   // > 0: a leaf of identical points, this many of them (the lowest indices) are all a search needs
        if (!cut) {
          const uint32_t ch = readlane_u32(chl, x);
          if (ch & PT_LEAF_TRUNC) { front = ch & ~PT_LEAF_TRUNC; cut = true; }
          else if (ch != 0u) { kids |= 1u << x; cut = true; }
        }
        if (!cut) {
          if (run_e == run_s) run_s = readlane_u32(stl, x);
          run_e = readlane_u32(stl, x + 1);
          continue;
        }
        if (run_e > run_s) range(run_s, run_e);
        run_s = run_e = 0;
        if (front) { const uint32_t fs = readlane_u32(stl, x); range(fs, fs + front); }
      }
      if constexpr (DEPTH + 1 < PT_REFINE_DEPTH) {
        while (kids) {
          const int x = __ffs((int)kids) - 1;
          kids &= kids - 1;
          node<DEPTH + 1>(readlane_u32(chl, x));
        }
      }
    }
  }
};

#ifndef PT_WV_MINW_H
#define PT_WV_MINW_H 6
#endif
#ifndef PT_WV_MINW
#define PT_WV_MINW 8
#endif
template <class Rec, bool HIER>
__global__ __launch_bounds__(WG, HIER ? PT_WV_MINW_H : PT_WV_MINW) void knn_wave_kernel(GridParams gp, const Rec* __restrict__ src, const uint32_t* __restrict__ cs, const Rec* __restrict__ tgt,
                                                      uint32_t m, int k, const double* __restrict__ bound2, uint32_t* __restrict__ out_idx,
                                                      double* __restrict__ out_d2, const uint32_t* __restrict__ list, const uint32_t* __restrict__ list_n,
                                                      HierArgs ha, WaveBlend wb) {
  // Consecutive workgroups go to different XCDs (8 of them, each with its own L2): hand the list out in runs of WV_RUN workgroups
  // per XCD, so that the targets of neighbouring cells -- which read the same 27 cells -- meet in one L2, while all XCDs still
  // advance through the list together (one contiguous eighth per XCD: the dense parts of the cloud end up on a few XCDs, 1.6 x slower).
  const uint32_t count = list ? *list_n : m;
  const uint32_t j = blockIdx.x >> 3, wgl = ((j / WV_RUN) * 8u + (blockIdx.x & 7u)) * WV_RUN + j % WV_RUN;
  const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(wgl * 4u + (threadIdx.x >> 6)));       // wave-uniform by construction: said so, the target and everything derived from it live in SGPRs
  if (wid >= count) return;                                 // whole waves leave together
  const int lane = threadIdx.x & 63;
  const Rec tr = tgt[list ? list[wid] : wid];
#ifdef PT_VISITS
  const unsigned long long pt_t0 = wall_clock64();
  unsigned long long pt_ph[4] = {pt_t0, pt_t0, pt_t0, pt_t0};      // cells known / own cell done / ring-1 stream done / search done
#endif
  __shared__ uint4 pend[WG / 64][64];
  WaveScan<Rec> W;
  W.src = src; W.nodes = ha.nodes; W.k = k; W.lane = lane;
  W.pend = pend[threadIdx.x >> 6];
  W.q[0] = (double)tr.x; W.q[1] = (double)tr.y; W.q[2] = (double)tr.z;
  W.qf[0] = (float)tr.x; W.qf[1] = (float)tr.y; W.qf[2] = (float)tr.z;      // (used by fp32 clouds only, whose targets are fp32 too)
  W.h2 = gp.h * gp.h;
  int c[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    W.u[a] = (W.q[a] - gp.bbmin[a]) * gp.inv_h;
    c[a] = (int)fmin(fmax(W.u[a], 0.0), (double)(gp.dim[a] - 1));
  }
  W.bnd_d = bound2 ? bound2[tr.id] : INFINITY;
  if (W.bnd_d < 0.0) {         // (as in knn_kernel: nothing wanted from this cloud; wave-uniform)
    if (lane < k) { const size_t row0 = (size_t)tr.id * (size_t)k; out_idx[row0 + lane] = PT_NOIDX_U; if (out_d2) out_d2[row0 + lane] = INFINITY; }
    return;
  }
  W.reset();
  const int ring_limit = min(WV_RING_MAX, max(PT_RING_LIMIT, (int)cbrtf(0.07f * (float)gp.nblocks)));
  // One loop serves ring 1 (27 cells, the target's own first, then its row, then the rest centre-first) and every further shell
  // (64 of its cells per step), so that the scan and the descent exist once in the code.
  int rr = 1, st = -1, nst = 0;
  for (;;) {
    int x = 0, y = 0, z = 0;
    bool valid;
    if (st < 0) {                                           // ring 1: lane i < 27 -> row i / 3 (centre-first), cell 0, -1, +1 of it
      const int r = lane / 3, j = lane - 3 * r;
      valid = lane < 27;
      x = c[0] + (j == 0 ? 0 : (j == 1 ? -1 : 1)); y = c[1] + row_dy(valid ? r : 0); z = c[2] + row_dz(valid ? r : 0);
    } else {
      // cell i of the shell of ring rr (side^3 - (side - 2)^3 of them), 64 per step: the two full planes dz = -rr, +rr row by row, then
      // for every plane in between its perimeter -- row dy = -rr, row dy = +rr, column dx = -rr, column dx = +rr
      const uint32_t side = 2u * (uint32_t)rr + 1u, in = side - 2u, plane = side * side, per = 4u * side - 4u;
      const uint32_t i = (uint32_t)st * 64u + (uint32_t)lane;
      valid = i < 2u * plane + in * per;
      int dx, dy, dz;
      if (i < 2u * plane) {
        const uint32_t j = i < plane ? i : i - plane, row = j / side;
        dz = i < plane ? -rr : rr; dy = (int)row - rr; dx = (int)(j - row * side) - rr;
      } else {
        const uint32_t j = i - 2u * plane, pz = j / per, q = j - pz * per;
        dz = -rr + 1 + (int)pz;
        if (q < 2u * side) { dy = q < side ? -rr : rr; dx = (int)(q < side ? q : q - side) - rr; }
        else { const uint32_t t = q - 2u * side; dx = t < in ? -rr : rr; dy = -rr + 1 + (int)(t < in ? t : t - in); }
      }
      x = c[0] + dx; y = c[1] + dy; z = c[2] + dz;
    }
    valid = valid && x >= 0 && x < gp.dim[0] && y >= 0 && y < gp.dim[1] && z >= 0 && z < gp.dim[2];
    uint32_t key = 0, S = 0, E = 0;
    double g2 = 0.0;
    if (valid) {
      key = cell_key(gp, x, y, z);
      S = cs[key]; E = cs[key + 1];
      const double gx = cell_gap(W.u, 0, x, x), gy = cell_gap(W.u, 1, y, y), gz = cell_gap(W.u, 2, z, z);
      g2 = gx * gx + gy * gy + gz * gz;
    }
#ifdef PT_VISITS
    if (st < 0) { asm volatile("" ::"v"(S), "v"(E)); pt_ph[0] = wall_clock64(); }      // the 27 cells' table entries are here
#endif
    // refined cells are descended into (one by one: the target's own first); everything else of this step is ONE stream, after the
    // own cell on the first step so that the bound it leaves decides which of the other 26 are read at all
    uint32_t nid = 0;
    if constexpr (HIER) { if (E - S > ha.thr) nid = ha.cell_node[key]; }       // (S == E == 0 for lanes without a cell)
    if (st < 0) {
      const uint32_t s0 = readlane_u32(S, 0), e0 = readlane_u32(E, 0), n0 = readlane_u32(nid, 0);
      if (n0) W.template node<0>(n0);
      else W.range(s0, e0);
      if (lane == 0) { S = E = 0; nid = 0; }
      W.flush();                                            // the limit the own cell leaves decides which of the other 26 are read
#ifdef PT_VISITS
      asm volatile("" ::"v"(W.ld)); pt_ph[1] = wall_clock64();
#endif
    }
    const bool on = E > S && !(g2 * W.h2 > W.lim_d);
    W.stream(S, on && !nid ? E - S : 0u);
#ifdef PT_VISITS
    if (st < 0) { asm volatile("" ::"v"(W.ld)); pt_ph[2] = wall_clock64(); }
#endif
    if constexpr (HIER) {
      unsigned long long want = ballot64(on && nid);
      while (want) {                                        // wave-uniform
        const int i = __ffsll((long long)want) - 1;
        want &= want - 1;
        if (readlane_f64(g2, i) * W.h2 > W.lim_d) continue; // the limit has moved since the ballot
        W.template node<0>(readlane_u32(nid, i));
      }
    }
    if (st >= 0 && ++st < nst) continue;
    // ring rr is complete: every unscanned point lies beyond one of the box faces that still has cells behind it
    W.flush();
    bool covered = true;
    double dout = INFINITY;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int lo = c[a] - rr, hi = c[a] + rr;
      if (lo > 0) { covered = false; dout = fmin(dout, W.u[a] - (double)lo); }
      if (hi < gp.dim[a] - 1) { covered = false; dout = fmin(dout, (double)(hi + 1) - W.u[a]); }
    }
    if (covered) break;
    dout = fmax(dout - PT_CELL_EPS, 0.0);
    if (dout * dout * W.h2 > W.lim_d) break;
    if (rr >= ring_limit) {
      // far from the points: sweep the BLOCKS (skip the empty ones, prune by box, scan the rest), the list started again so that
      // no point is offered twice -- as the group kernel does, 64 blocks per step
      W.reset();
      const uint32_t nb = (uint32_t)gp.nblocks;
      for (uint32_t b0 = 0; b0 < nb; b0 += 64u) {
        const uint32_t b = b0 + (uint32_t)lane;
        uint32_t bs_ = 0, be_ = 0;
        double bg2 = 0.0;
        if (b < nb) { bs_ = cs[(size_t)b * PT_BLOCK_CELLS]; be_ = cs[((size_t)b + 1) * PT_BLOCK_CELLS]; }
        if (be_ > bs_) {
          const uint32_t macro = b >> 9, m9 = b & 511u;
          const int bx = (int)(macro % (uint32_t)gp.mdim[0]) * 8 + (int)((m9 & 1u) | ((m9 >> 2) & 2u) | ((m9 >> 4) & 4u));
          const int by = (int)((macro / (uint32_t)gp.mdim[0]) % (uint32_t)gp.mdim[1]) * 8 + (int)(((m9 >> 1) & 1u) | ((m9 >> 3) & 2u) | ((m9 >> 5) & 4u));
          const int bz = (int)(macro / (uint32_t)(gp.mdim[0] * gp.mdim[1])) * 8 + (int)(((m9 >> 2) & 1u) | ((m9 >> 4) & 2u) | ((m9 >> 6) & 4u));
          const double gx = cell_gap(W.u, 0, bx * 8, bx * 8 + 7), gy = cell_gap(W.u, 1, by * 8, by * 8 + 7), gz = cell_gap(W.u, 2, bz * 8, bz * 8 + 7);
          bg2 = gx * gx + gy * gy + gz * gz;
        }
        W.stream(bs_, be_ > bs_ && !(bg2 * W.h2 > W.lim_d) ? be_ - bs_ : 0u);
      }
      break;
    }
    ++rr;
    st = 0;
    { const int side = 2 * rr + 1; nst = (side * side * side - (side - 2) * (side - 2) * (side - 2) + 63) / 64; }
  }
  W.finish();                                               // (the block sweep ends with candidates set aside; the pool is sorted for the output)
#ifdef PT_VISITS
  asm volatile("" ::"v"(W.ld)); pt_ph[3] = wall_clock64();
#endif
  if (lane < k) {
    const size_t row = (size_t)tr.id * (size_t)k;
    out_idx[row + lane] = W.li;
    if (out_d2) out_d2[row + lane] = W.ld;
  }
  if (wb.attr) {
    // the blend of pt_attr.hip's blend_one, one neighbour per lane: a single gather instruction per target, whose latency hides
    // behind the other waves' ranking (as a kernel of its own the 1.6e9 gathers of 50 M targets at k = 32 take 50 ms)
    double w = 0.0, a0 = 0.0, a1 = 0.0, a2 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
    if (lane < k && W.li != PT_NOIDX_U && W.li < wb.n_attr) {
      w = wb.mode == 1 ? __builtin_amdgcn_rcp(W.ld + 1e-12) : 1.0;      // (v_rcp_f64 / v_rsq_f64, as in the tile kernel's epilogue: no division expanded into FMAs in this kernel)
      const Attr a = pt_gather_attr(wb.attr, W.li);
      a0 = w * (double)(a.rgba & 0xFFu); a1 = w * (double)((a.rgba >> 8) & 0xFFu); a2 = w * (double)((a.rgba >> 16) & 0xFFu);
      b0 = w * (double)a.nx; b1 = w * (double)a.ny; b2 = w * (double)a.nz;
    }
#pragma unroll 1
    for (int o = 32; o > 0; o >>= 1) {
      w += __shfl_xor(w, o); a0 += __shfl_xor(a0, o); a1 += __shfl_xor(a1, o); a2 += __shfl_xor(a2, o);
      b0 += __shfl_xor(b0, o); b1 += __shfl_xor(b1, o); b2 += __shfl_xor(b2, o);
    }
    if (lane == 0) {
      if (w > 0.0) {
        const double iw = __builtin_amdgcn_rcp(w);
        a0 *= iw; a1 *= iw; a2 *= iw; b0 *= iw; b1 *= iw; b2 *= iw;
        const double l2 = (b0 * b0 + b1 * b1) + b2 * b2;
        if (l2 >= 1e-24) { const double il = __builtin_amdgcn_rsq(l2); b0 *= il; b1 *= il; b2 *= il; }
      }
      const size_t t3 = 3 * (size_t)tr.id;
      if (wb.rgb_out) { wb.rgb_out[t3] = (float)a0; wb.rgb_out[t3 + 1] = (float)a1; wb.rgb_out[t3 + 2] = (float)a2; }
      if (wb.nrm_out) { wb.nrm_out[t3] = (float)b0; wb.nrm_out[t3 + 1] = (float)b1; wb.nrm_out[t3 + 2] = (float)b2; }
    }
  }
#ifdef PT_VISITS
  __builtin_amdgcn_wave_barrier();
  if (out_d2 && lane == 0 && k >= 4) {                      // (results are garbage in these columns)
    const size_t row = (size_t)tr.id * (size_t)k;
    out_d2[row + k - 1] = (double)W.nv * 64.0; out_d2[row + k - 2] = (double)(wall_clock64() - pt_t0); out_d2[row + k - 3] = (double)pt_t0;
    out_d2[row + k - 4] = -(double)(W.nn + 1u);            // negative: a wave-kernel row, and how many nodes it entered (+1)
    if (k >= 12) {                                          // phase times (tools/probe_wave_visits.py) and the number of sort-merges
      out_d2[row + k - 5] = (double)(pt_ph[0] - pt_t0); out_d2[row + k - 6] = (double)(pt_ph[1] - pt_ph[0]); out_d2[row + k - 7] = (double)(pt_ph[2] - pt_ph[1]);
      out_d2[row + k - 8] = (double)(pt_ph[3] - pt_ph[2]); out_d2[row + k - 9] = (double)(wall_clock64() - pt_ph[3]); out_d2[row + k - 10] = (double)W.nmerge;
    }
  }
#endif
}

}  // namespace

// wave kernel over a list of `count` target positions (list == nullptr: all m targets); cell_node / nodes may be null (no refined cells)
template <class Rec>
void pt_launch_knn_wave(const GridParams& gp, const Rec* src, const uint32_t* cell_start, const uint32_t* cell_node, const uint32_t* nodes, uint32_t node_thr,
                        const Rec* tgt, uint32_t count, int k, const double* bound2, uint32_t* out_idx, double* out_d2, const uint32_t* list,
                        const uint32_t* list_n, hipStream_t s, const Attr* attr, uint32_t n_attr, int blend_mode, float* rgb_out, float* nrm_out) {
  if (!count) return;
  const WaveBlend wb{attr, n_attr, blend_mode, rgb_out, nrm_out};
  const uint32_t nwg = (((count + 3u) / 4u + 8u * WV_RUN - 1u) / (8u * WV_RUN)) * 8u * WV_RUN;      // whole rounds of 8 XCDs x WV_RUN workgroups (the kernel's mapping)
  const HierArgs ha{cell_node, nodes, node_thr, nullptr, 0u};
  if (nodes) hipLaunchKernelGGL((knn_wave_kernel<Rec, true>), dim3(nwg), dim3(WG), 0, s, gp, src, cell_start, tgt, count, k, bound2, out_idx, out_d2, list, list_n, ha, wb);
  else hipLaunchKernelGGL((knn_wave_kernel<Rec, false>), dim3(nwg), dim3(WG), 0, s, gp, src, cell_start, tgt, count, k, bound2, out_idx, out_d2, list, list_n, ha, wb);
}
template void pt_launch_knn_wave<RecF>(const GridParams&, const RecF*, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t, const RecF*, uint32_t, int, const double*,
                                       uint32_t*, double*, const uint32_t*, const uint32_t*, hipStream_t, const Attr*, uint32_t, int, float*, float*);
template void pt_launch_knn_wave<RecD>(const GridParams&, const RecD*, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t, const RecD*, uint32_t, int, const double*,
                                       uint32_t*, double*, const uint32_t*, const uint32_t*, hipStream_t, const Attr*, uint32_t, int, float*, float*);
