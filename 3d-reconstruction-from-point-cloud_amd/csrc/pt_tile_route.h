// pt_tile_route.h -- which instantiation of the LDS tile kernel (pt_knn_tile.hip) answers a query: the ONE description of that
// decision.  Plain C++ (no HIP): the launcher dispatches on it, pt_api.hip names the geometry with it, and
// host/tile_route_selftest.cpp prints it for the CPU suite to compare with tests/_tile_variants.py.
#pragma once
#include <stdint.h>

// Geometries: Large  = one 768-thread workgroup per CU, 8448 staged records (132 KB of LDS), for rho ~ 6-8;
//             Small  = two 512-thread workgroups per CU (80 KB each: one stages while the other ranks), k <= 16;
//             Medium = two 384-thread workgroups per CU, the K = 32 body on a 3888-record region, k in 17..24: for clouds whose regions
//                      are small because most of their cells are empty (surfaces).
// (k in 25..32 runs the WIDE body whatever is asked for: 512 threads, 8960 staged records, a 64-entry queue, one workgroup per CU.)
enum class TileGeometry { Large, Small, Medium };

// staged-region capacities (records) of the tile kernel's geometries: what is left of 80 KB (two workgroups per CU) or
// 160 KB (one) after the per-lane queue segments and the cell table
constexpr int PT_TILE_CAP_SMALL_8 = 4400, PT_TILE_CAP_SMALL_16 = 3888, PT_TILE_CAP_LARGE = 8448, PT_TILE_CAP_WIDE = 8960;

// knn_tile_kernel<K, CAP, TWG, WIDE, BLEND, DBL, KC, BND>: the arguments the route decides (BLEND, DBL, BND are the launch's own)
struct TileRoute { int K, CAP, TWG; bool WIDE; int KC; };

// Every route there is; with the eight BLEND / DBL / BND combinations these are all the instantiations that exist.  K is the list width
// (a power of two), KC the length of pass 1's value chain: the reference's K = 20 (src/pointsTransfer.cpp:128) runs the K = 32 body
// with a chain of 20, k in 21..24 with one of 24.
constexpr int PT_TILE_ROUTES = 9;
constexpr TileRoute PT_TILE_ROUTE[PT_TILE_ROUTES] = {
    {8, PT_TILE_CAP_SMALL_8, 512, false, 8},     {16, PT_TILE_CAP_SMALL_16, 512, false, 16},      // small
    {32, PT_TILE_CAP_SMALL_16, 384, false, 20},  {32, PT_TILE_CAP_SMALL_16, 384, false, 24},      // medium
    {8, PT_TILE_CAP_LARGE, 768, false, 8},       {16, PT_TILE_CAP_LARGE, 768, false, 16},         // large
    {32, PT_TILE_CAP_LARGE, 768, false, 20},     {32, PT_TILE_CAP_LARGE, 768, false, 24},
    {32, PT_TILE_CAP_WIDE, 512, true, 32},                                                        // wide
};

// Row of PT_TILE_ROUTE for a query of k neighbours (k <= 32) that asks for geometry g.  bounded: the targets bring bounds (per-target
// ones, the max_dist cap, or both); capped: the cap is among them.
constexpr int pt_tile_route_row(int k, TileGeometry g, bool bounded, bool capped) {
  if (k > 24) return 8;
  const int bucket = k <= 8 ? 0 : (k <= 16 ? 1 : (k <= 20 ? 2 : 3));
  // The bounded medium geometry is taken only under a cap: per-target bounds without one are the chunks of a streamed source
  // (pt_stream_query), and those keep the large geometry they always had.
  if (g == TileGeometry::Medium && k > 16 && (!bounded || capped)) return bucket;
  if (g == TileGeometry::Small && k <= 16) return bucket;       // (K = 32 needs more registers than two 512-thread workgroups per CU leave)
  return 4 + bucket;
}
constexpr TileRoute pt_tile_route(int k, TileGeometry g, bool bounded, bool capped) { return PT_TILE_ROUTE[pt_tile_route_row(k, g, bounded, capped)]; }

// the route code of one tile launch (pt_stats_t::tile_variant, include/pt_api.h): the instantiation's template arguments, packed
constexpr uint32_t pt_tile_code(const TileRoute& r, bool blend, bool dbl, bool bnd, bool listed) {
  return (uint32_t)r.K | (uint32_t)r.KC << 6 | (uint32_t)(r.TWG / 64) << 12 | (uint32_t)r.WIDE << 16 | (uint32_t)blend << 17 | (uint32_t)dbl << 18 |
         (uint32_t)bnd << 19 | (uint32_t)listed << 20;
}
