// pt_knn_common.h -- device-side helpers shared by the k-NN search kernels (pt_knn_group.hip, pt_knn_wave.hip, pt_knn_tile.hip), for
// gfx950 (MI355X).  No kernels here.
//
// The search replaces the reference's query loop
//     K_neighbor_search search(tree, vertices[...], K);  for (it = search.begin(); ...)
// (reference src/pointsTransfer.cpp:462-479; CGAL Orthogonal_k_neighbor_search, eps = 0, results ascending)
// with one launch over all targets.  Metric: reference src/Distance.h:6-11, evaluated in fp64 as
// (dx*dx + dy*dy) + dz*dz with contraction off -- the same 3 mul + 2 add the reference's flags produce.
// Cell pruning is Distance::min_distance_to_rectangle (reference src/Distance.h:27-57) applied to cell
// boxes; ring termination is the same bound applied to the faces of the box already scanned.
//
// Three kernels, all exact:
//   knn_tile_kernel  (pt_knn_tile.hip) fp32 clouds and fp32 shadows of fp64 clouds, k <= 32 -- the throughput path.  One
//                    workgroup per 8^3-cell block stages the 10^3-cell region around it in LDS and ranks it with a DPP quad
//                    per target: fp32 bound -> queue -> exact fp64 re-rank.  What ring 1 cannot settle goes to a todo list.
//   knn_kernel       (pt_knn_group.hip) everything else: fp64 clouds, radius-bounded multi-GPU queries, the todo list.
//                    8 lanes per target, 8 targets per wave64, 32 per 256-thread workgroup.
//   knn_wave_kernel  (pt_knn_wave.hip) ONE WAVE PER TARGET, for dense neighbourhoods of clouds with strong density contrast,
//                    k > 16 leftovers of the tile kernel and surfaces.
#pragma once
#include "pt_internal.h"

namespace pt_knn {

constexpr int WG = 256;
constexpr int PT_RING_LIMIT = 8;   // least number of rings walked shell by shell before the group and wave kernels sweep the blocks instead

__device__ inline bool key_lt(double ad, uint32_t ai, double bd, uint32_t bi) { return ad < bd || (ad == bd && ai < bi); }

template <class Rec>
__device__ inline double dist2(const double (&q)[3], const Rec& r) {
#pragma clang fp contract(off)
  const double dx = q[0] - (double)r.x;
  const double dy = q[1] - (double)r.y;
  const double dz = q[2] - (double)r.z;
  return (dx * dx + dy * dy) + dz * dz;     // reference src/Distance.h:10, left to right, unfused
}

// ---- DPP helpers: data movement inside the 8-lane group without touching LDS ---------------------------------
template <int CTRL>
__device__ inline uint32_t dpp_u32(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}
template <int CTRL>
__device__ inline double dpp_f64(double v) {
  const uint32_t lo = dpp_u32<CTRL>((uint32_t)__double2loint(v)), hi = dpp_u32<CTRL>((uint32_t)__double2hiint(v));
  return __hiloint2double((int)hi, (int)lo);
}
constexpr int DPP_SHR1 = 0x111;          // row_shr:1      lane i <- lane i-1
constexpr int DPP_QUAD3 = 0xFF;          // quad_perm [3,3,3,3]
constexpr int DPP_HMIRROR = 0x141;       // row_half_mirror: lane i <- lane 7-i of the same 8 lanes

__device__ inline uint32_t cell_key(const GridParams& gp, int x, int y, int z) {
  return (pt_block_id(gp.mdim, x, y, z) << 9) + pt_local_cell(x, y, z);
}

// The cell-box bound: distance (cell units, >= 0) from the coordinate u to the interval [lo, hi] of its axis, under-estimated by the slack.
// The wave kernel's pruning tests (cells, blocks, the sub-cells of refined nodes) are built from it; the group kernel spells the same
// arithmetic out in TargetGeom::gap and HierScan::gap2 (calling this there changes its instruction schedule: DESIGN.md section 14).
__device__ inline double cell_gap(double u, double lo, double hi) { return fmax(fmax(lo - u, u - hi) - PT_CELL_EPS, 0.0); }
// ... of the target at u (cell units) to the cells lo .. hi of axis a
__device__ inline double cell_gap(const double (&u)[3], int a, int lo, int hi) { return cell_gap(u[a], (double)lo, (double)(hi + 1)); }

// (dy,dz)+1 of the 9 rows of ring 1, packed 2 bits each, centre row first, then faces, then edges:
// dy = 0,-1,1,0,0,-1,1,-1,1 ; dz = 0,0,0,-1,1,-1,-1,1,1
constexpr uint32_t ROW_OY = 139617u, ROW_OZ = 164373u;
__device__ inline int row_dy(int r) { return (int)((ROW_OY >> (2 * r)) & 3u) - 1; }
__device__ inline int row_dz(int r) { return (int)((ROW_OZ >> (2 * r)) & 3u) - 1; }

// HIER: the grid carries refined cells (pt_refine.hip: cell_node / nodes / node_thr).  Cells with more than node_thr points are then
// left out of the flat scans, remembered in the group's pending list and descended into (HierScan) at the head of the ring loop.
// heavy / heavy_n / wave_min: targets whose 27 nearest cells hold at least wave_min points are not answered by the group kernel but listed
// (their position in the sorted target array) for the wave kernel -- one wave per target pays off where the scans are long.
// heavy: one byte per target position, zeroed by the caller; 1 = wave kernel, 2 = its descending variant (a refined cell among the 27).
struct HierArgs { const uint32_t* cell_node; const uint32_t* nodes; uint32_t thr; uint8_t* heavy; uint32_t wave_min; };

// fp32 pre-filter distance of the tile and wave kernels (fp32 records, fp32 targets): 3 sub, 1 mul, 2 fma on exact inputs, all
// terms >= 0 -- relative error < 2^-21.  Never a result: what passes is evaluated again in fp64, unfused.
__device__ inline float dist2_f32(float qx, float qy, float qz, const RecF& r) {
  const float dx = qx - r.x, dy = qy - r.y, dz = qz - r.z;
  return __builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, dz * dz));
}
template <class Rec> struct IsRecF { static constexpr bool value = false; };
template <> struct IsRecF<RecF> { static constexpr bool value = true; };

// __ballot(bool) goes through an integer compare: the compiler materialises the predicate (v_cndmask 0 / 1) and compares it with zero
// again -- two VALU instructions per ballot in a kernel bound by VALU issue.  The builtin takes the condition's mask as it is.
__device__ __forceinline__ unsigned long long ballot64(bool p) { return __builtin_amdgcn_ballot_w64(p); }

}  // namespace pt_knn
