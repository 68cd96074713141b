// tile_route_selftest -- prints the tile launcher's route table (csrc/pt_tile_route.h) for the CPU suite: one line
//   k geometry bound K CAP TWG WIDE KC
// for every k in 1..32 x {large, small, medium} x {none: unbounded, stream: per-target bounds without a cap, cap: the max_dist cap}.
// tests/test_boundary.py compares every line with tests/_tile_variants.py.
#include <cstdio>

#include "../csrc/pt_tile_route.h"

// every row of the table is reachable and codes tell the rows apart: checked at compile time, the table being constexpr
static_assert(pt_tile_route(20, TileGeometry::Medium, true, false).TWG == 768, "bounded medium without a cap runs the large geometry");
static_assert(pt_tile_code(pt_tile_route(20, TileGeometry::Large, false, false), false, false, false, false) == (32u | 20u << 6 | 12u << 12), "code layout");

int main() {
  const TileGeometry geo[3] = {TileGeometry::Large, TileGeometry::Small, TileGeometry::Medium};
  const char* const geo_name[3] = {"large", "small", "medium"};
  const char* const bound_name[3] = {"none", "stream", "cap"};
  for (int k = 1; k <= 32; ++k)
    for (int g = 0; g < 3; ++g)
      for (int b = 0; b < 3; ++b) {
        const TileRoute r = pt_tile_route(k, geo[g], b != 0, b == 2);
        std::printf("%d %s %s %d %d %d %d %d\n", k, geo_name[g], bound_name[b], r.K, r.CAP, r.TWG, (int)r.WIDE, r.KC);
      }
  return 0;
}
