// pt_bake.hip -- per-face detail transfer into the UV atlas ("texture bake") and edge padding, for gfx950 (MI355X).
//
// Replaces the body of the reference's face loop after the neighbour search and its rasteriser and post-processing:
//   reference src/pointsTransfer.cpp:466-479  union of the three corners' neighbour lists
//                                    :484-537  plane through the face, projection, barycentric in-triangle filter
//                                    :539-581  per-face Delaunay triangulation of corners + interior points, UV of the interior
//                                              points by barycentric interpolation of the corner UVs
//                                    :66-107   draw_triangle: barycentric colour mix per pixel, BGRA bytes at (resolution - j, i)
//                                    :593-611  25x25 dilate, ~alpha mask, add  (edge padding)
// The reference leans on CGAL (Plane_3::to_2d, Triangle_coordinates_2, Delaunay_triangulation_2) and OpenCV (dilate) for these;
// neither is in this image, so the exact results are BUILD-DEFINED where the libraries (or undefined behaviour) decide them --
// the definition is written out in DESIGN.md ("Texture bake") and restated on the CPU by the test oracle; this file follows it
// operation for operation in fp64 with contraction off, so that the atlas bytes are identical:
//   * neighbour union de-duplicated by ORIGINAL INDEX, ascending;   * orthonormal plane frame at corner 0 (e1 along corner 0 -> 1);
//   * Delaunay = every non-degenerate triple whose circumcircle holds no other point strictly inside, predicates evaluated on the
//     index-sorted tuple (consistent signs), enumerated in lexicographic (i, j, k) order;
//   * a pixel covered by several triangles keeps the LAST one in (face, triangle) order -- the single-threaded reference's result:
//     here every covered pixel does one 64-bit atomicMax on a key {face * 256 + triangle + 1, BGRA}; a second pass keeps the BGRA.
//
// Object-space normal map ("Normal map"): the same face pass can also write -- or write instead -- a second key
// plane whose payload is the barycentric mix of the three sub-triangle normals, renormalised PER PIXEL and encoded R = x, G = y, B = z.
//   * a corner's normal is the mesh vertex record's `normal` (double), an interior point's is the source point's attribute normal
//     (float, widened, AS UPLOADED: no per-point normalisation; a cloud built without normals holds zeros and its texels fall back);
//   * both kinds are kept as doubles in LDS next to pc[] (nothing is rounded to float: 11 KB per wave, 44 KB per workgroup);
//   * a mix of zero or non-finite length encodes (0, 0, 1);   * both planes carry the same key sequence, so the same (face, triangle)
//     wins a pixel in both;   * the edge padding of the normal plane is the colour plane's (a per-channel maximum: the padded ring is
//     NOT unit length).
// Height map ("Height map"): a third key plane whose payload is the barycentric mix of the kept points' SIGNED
// HEIGHTS over the face plane -- the third dot product of the projection, with the unit face normal e3 = n / |n|; a corner's is 0 --
// divided by the caller's height_range H and encoded as a grey byte (0 -> 128, +H -> 255, -H -> 0, saturating).  A candidate's height
// rides in a register from the projection to the slot fill (the same lane handles the same candidate in both), so the wave layout
// grows by ph[] alone.  The call's two scalars travel behind the key planes (BK_TRAILER words): the maximum |h| over the interior kept
// points, as the bit pattern of a non-negative double under atomicMax, and H -- the kernel's signature, and with it the colour-only
// and colour / normal instantiations, stay as they were.
// The map set is a compile-time property of the kernel (BakeCfg below): the colour-only kernel is the kernel this file always had,
// instruction for instruction.
//
// One wave64 per face (four per workgroup).  Nothing here is bandwidth-critical: the atlas is 64 M pixels, a face a few dozen.
#include "pt_internal.h"

#include <algorithm>
#include <type_traits>

namespace {

constexpr int BK_WG = 256, BK_WAVES = BK_WG / 64;
constexpr int BK_MAXNBR = 96;             // 3 corners x k <= 32
constexpr int BK_MAXPTS = 3 + BK_MAXNBR;
constexpr int BK_MAXTRI = 255;            // triangle number within a face must fit 8 bits of the pixel key

struct BakeWave {
  uint32_t raw[BK_MAXNBR + 32];           // the three neighbour lists as read, padded to 128
  uint32_t sorted[BK_MAXNBR];             // distinct indices, ascending
  double cx[BK_MAXNBR], cy[BK_MAXNBR];    // 2-D image of candidate e (sorted order)
  double cu[BK_MAXNBR], cv[BK_MAXNBR];    // its interpolated UV
  uint8_t cin[BK_MAXNBR + 32];            // inside the face?
  double px[BK_MAXPTS], py[BK_MAXPTS], pu[BK_MAXPTS], pv[BK_MAXPTS];   // kept points: corners 0..2, then interior points
  uint32_t pc[BK_MAXPTS];                 // their colour, r | g << 8 | b << 16
  uint32_t tri[BK_MAXTRI];                // accepted triangles, i | j << 8 | k << 16, in enumeration order
};
struct BakeWaveN : BakeWave {              // the instantiations that write the normal plane
  double pnx[BK_MAXPTS], pny[BK_MAXPTS], pnz[BK_MAXPTS];   // the kept points' normals, as stored (not normalised)
};
struct BakeWaveH : BakeWave { double ph[BK_MAXPTS]; };     // the instantiations that write the height plane: the kept points' heights
struct BakeWaveNH : BakeWaveN { double ph[BK_MAXPTS]; };
constexpr int BK_COLOR = 1, BK_NORMAL = 2, BK_HEIGHT = 4;   // = PT_MAP_COLOR, PT_MAP_NORMAL, PT_MAP_HEIGHT
constexpr int bk_planes(int maps) { return (maps & BK_COLOR ? 1 : 0) + (maps & BK_NORMAL ? 1 : 0) + (maps & BK_HEIGHT ? 1 : 0); }
static_assert(sizeof(BakeWaveN) * BK_WAVES <= 64 * 1024 && sizeof(BakeWaveH) * BK_WAVES <= 64 * 1024 && sizeof(BakeWaveNH) * BK_WAVES <= 64 * 1024,
              "the bake's LDS must fit the 64 KB static limit");
static_assert(BK_TRAILER == 2, "behind the key planes: max |h| (bits of a non-negative double), then height_range");
// The face kernel is a template on ONE type: the cloud's coordinate type for the colour-only kernel, WithMaps<coordinate type, map set>
// for the instantiations that write the normal plane.  A plain second parameter (template <class T, int MAPS = BK_COLOR>) compiles the
// same colour-only body, but renames the instantiation (bake_faces_kernel<float, 1>), and tools/isa_diff.py pairs kernels of two builds
// by name and template arguments: this form keeps bake_faces_kernel<float> / <double> paired with every earlier build's.  (The mangled
// symbol does change -- its parameters are spelled BakeCfg<T>::Real -- which the tool masks.)  The body sits in the kernel itself:
// behind a device function, even a forced-inline one, the compiler schedules the colour-only kernel differently.
template <class T, int MAPS> struct WithMaps {};
template <class C> struct BakeCfg { using Real = C; using Wave = BakeWave; static constexpr int maps = BK_COLOR; };
template <class T, int M> struct BakeCfg<WithMaps<T, M>> {
  using Real = T;
  using Wave = std::conditional_t<(M & BK_HEIGHT) != 0, std::conditional_t<(M & BK_NORMAL) != 0, BakeWaveNH, BakeWaveH>, BakeWaveN>;
  static constexpr int maps = M;
};

__device__ inline double cross2(double ax, double ay, double bx, double by) { return ax * by - ay * bx; }
__device__ inline bool finite_d(double v) { return v == v && v - v == 0.0; }
// barycentric coordinates of X in (v0, v1, v2), A = cross(v1 - v0, v2 - v0)
__device__ inline void bary2(double Xx, double Xy, double x0, double y0, double x1, double y1, double x2, double y2, double A, double (&b)[3]) {
  b[0] = cross2(x1 - Xx, y1 - Xy, x2 - Xx, y2 - Xy) / A;
  b[1] = cross2(x2 - Xx, y2 - Xy, x0 - Xx, y0 - Xy) / A;
  b[2] = (1.0 - b[0]) - b[1];
}
__device__ inline double incircle_sorted(const double* px, const double* py, int w, int x, int y, int z) {
  const double adx = px[w] - px[z], ady = py[w] - py[z], bdx = px[x] - px[z], bdy = py[x] - py[z], cdx = px[y] - px[z], cdy = py[y] - py[z];
  const double al = adx * adx + ady * ady, bl = bdx * bdx + bdy * bdy, cl = cdx * cdx + cdy * cdy;
  return (al * (bdx * cdy - bdy * cdx) - bl * (adx * cdy - ady * cdx)) + cl * (adx * bdy - ady * bdx);
}
__device__ inline bool in_circumcircle(const double* px, const double* py, int i, int j, int k, int l, int os) {
  double d;
  int par;
  if (l > k) { d = incircle_sorted(px, py, i, j, k, l); par = 1; }
  else if (l > j) { d = incircle_sorted(px, py, i, j, l, k); par = -1; }
  else if (l > i) { d = incircle_sorted(px, py, i, l, j, k); par = 1; }
  else { d = incircle_sorted(px, py, l, i, j, k); par = -1; }
  return (double)(os * par) * d > 0.0;
}

// what a triangle needs for the normal plane: its vertices' normals and the second key plane; nothing in the colour-only instantiation
struct TriNormals { double v[3][3]; unsigned long long* __restrict__ keys; };
struct NoNormals {};
template <int MAPS> using TriN = std::conditional_t<(MAPS & BK_NORMAL) != 0, TriNormals, NoNormals>;
// ... and for the height plane: its vertices' heights, the range that maps to a byte, and the third key plane
struct TriHeights { double h[3]; double range; unsigned long long* __restrict__ keys; };
struct NoHeights {};
template <int MAPS> using TriH = std::conditional_t<(MAPS & BK_HEIGHT) != 0, TriHeights, NoHeights>;

// reference draw_triangle (:66-107), the wave's 64 lanes striding over the pixels of the bounding box that land inside the texture
template <int MAPS>
__device__ inline void draw_triangle(const double (&U)[3], const double (&V)[3], const uint32_t (&col)[3], int R, unsigned long long seq,
                                     unsigned long long* __restrict__ keys, int lane, const TriN<MAPS> tn, const TriH<MAPS> th = {}) {
  const double px = U[0] * R, py = V[0] * R, qx = U[1] * R, qy = V[1] * R, rx = U[2] * R, ry = V[2] * R;
  if (!(finite_d(px) && finite_d(py) && finite_d(qx) && finite_d(qy) && finite_d(rx) && finite_d(ry))) return;
  const double A = cross2(qx - px, qy - py, rx - px, ry - py);
  if (!(A != 0.0) || !finite_d(A)) return;
  const double xmin = fmin(px, fmin(qx, rx)), xmax = fmax(px, fmax(qx, rx));
  const double ymin = fmin(py, fmin(qy, ry)), ymax = fmax(py, fmax(qy, ry));
  const double fi0 = floor(xmin), fi1 = floor(xmax), fj0 = floor(ymin), fj1 = floor(ymax);
  // a bounding box wholly outside the texture is rejected in double, so that every cast below sees a value in [0, R]
  if (fi1 < 0.0 || fi0 > (double)(R - 1) || fj1 < 1.0 || fj0 > (double)R) return;
  const int i0 = (int)fmax(fi0, 0.0), i1 = (int)fmin(fi1, (double)(R - 1));                      // column i in [0, R)
  const int j0 = (int)fmax(fj0, 1.0), j1 = (int)fmin(fj1, (double)R);                            // row R - j in [0, R)
  const unsigned long long ni = (unsigned long long)(i1 - i0 + 1), total = ni * (unsigned long long)(j1 - j0 + 1);
  for (unsigned long long pix = (unsigned long long)lane; pix < total; pix += 64ull) {
    const int i = i0 + (int)(pix % ni), j = j0 + (int)(pix / ni);
    const int x = i >= R ? R - 1 : i, y = j >= R ? R - 1 : j;
    double b[3];
    bary2((double)x, (double)y, px, py, qx, qy, rx, ry, A, b);
    if (b[0] >= 0 && b[1] >= 0 && b[2] >= 0) {
      if constexpr ((MAPS & BK_COLOR) != 0) {
        uint32_t bgra = 0xFF000000u;
#pragma unroll
        for (int c = 0; c < 3; ++c) {                      // :95-97: double products summed, stored to a float, truncated to a byte
          const double c0 = (double)((col[0] >> (8 * c)) & 0xFFu), c1 = (double)((col[1] >> (8 * c)) & 0xFFu), c2 = (double)((col[2] >> (8 * c)) & 0xFFu);
          const float f = (float)((b[0] * c0 + b[1] * c1) + b[2] * c2);
          const float g = f < 0.f ? 0.f : (f > 255.f ? 255.f : f);
          bgra |= (uint32_t)g << (8 * (2 - c));            // byte 0 = B, 1 = G, 2 = R
        }
        atomicMax(&keys[(size_t)(R - j) * (size_t)R + (size_t)i], (seq << 32) | (unsigned long long)bgra);
      }
      if constexpr ((MAPS & BK_NORMAL) != 0) {             // the colour mix's shape on the normals, then unit length per pixel
        double m[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) m[c] = (b[0] * tn.v[0][c] + b[1] * tn.v[1][c]) + b[2] * tn.v[2][c];
        const double l = sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
        const bool unit = l > 0.0 && finite_d(l);          // zero, NaN, overflowed: straight up
        uint32_t bgra = 0xFF000000u;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double u = unit ? m[c] / l : (c == 2 ? 1.0 : 0.0);
          const double t = u * 127.5 + 127.5;
          const double r = fmin(fmax(t + 0.5, 0.0), 255.0);
          bgra |= (uint32_t)(int)r << (8 * (2 - c));       // byte 0 = z, 1 = y, 2 = x: R = x, G = y, B = z
        }
        atomicMax(&tn.keys[(size_t)(R - j) * (size_t)R + (size_t)i], (seq << 32) | (unsigned long long)bgra);
      }
      if constexpr ((MAPS & BK_HEIGHT) != 0) {             // the colour mix's shape on the heights, one grey byte
        const double m = (b[0] * th.h[0] + b[1] * th.h[1]) + b[2] * th.h[2];
        uint32_t g = 128u;                                 // a non-finite mix: zero height
        if (finite_d(m)) {
          const double t = m / th.range;
          const double u = t * 127.5 + 127.5;
          const double r = fmin(fmax(u + 0.5, 0.0), 255.0);
          g = (uint32_t)(int)r;
        }
        atomicMax(&th.keys[(size_t)(R - j) * (size_t)R + (size_t)i], (seq << 32) | (unsigned long long)(0xFF000000u | g * 0x010101u));
      }
    }
  }
}

// one face by one wave.  keys: one zeroed plane of R x R keys per map of the set, in the order colour, normal, height; behind them,
// when the set holds the height plane, BK_TRAILER words: max |h| (zeroed) and height_range
template <class T>
__global__ __launch_bounds__(BK_WG) void bake_faces_kernel(const typename BakeCfg<T>::Real* __restrict__ sx, const typename BakeCfg<T>::Real* __restrict__ sy,
                                                           const typename BakeCfg<T>::Real* __restrict__ sz,
                                                           const Attr* __restrict__ attr, uint32_t n, const unsigned char* __restrict__ verts /* 80-B records */,
                                                           uint32_t nv, const int32_t* __restrict__ faces, uint32_t nf,
                                                           const uint32_t* __restrict__ nbr, int k, int R, unsigned long long* __restrict__ keys) {
  __shared__ typename BakeCfg<T>::Wave sh[BK_WAVES];
  const int lane = threadIdx.x & 63;
  const uint32_t f = blockIdx.x * BK_WAVES + (threadIdx.x >> 6);
  if (f >= nf) return;                                     // whole waves leave; there is no workgroup barrier below
  typename BakeCfg<T>::Wave& W = sh[threadIdx.x >> 6];
  const int32_t f0 = faces[3 * (size_t)f], f1 = faces[3 * (size_t)f + 1], f2 = faces[3 * (size_t)f + 2];
  if (f0 < 0 || f1 < 0 || f2 < 0 || (uint32_t)f0 >= nv || (uint32_t)f1 >= nv || (uint32_t)f2 >= nv) return;      // malformed face
  const int32_t fv[3] = {f0, f1, f2};
  double c3[3][3], cu[3], cv[3];
  constexpr int MAPS = BakeCfg<T>::maps;
  constexpr bool NRM = (MAPS & BK_NORMAL) != 0;
  TriN<MAPS> tn;
  if constexpr (NRM) tn.keys = (MAPS & BK_COLOR) ? keys + (size_t)R * (size_t)R : keys;
  constexpr bool HGT = (MAPS & BK_HEIGHT) != 0;
  TriH<MAPS> th;
  if constexpr (HGT) {
    th.keys = keys + (size_t)(bk_planes(MAPS) - 1) * ((size_t)R * (size_t)R);
    th.range = __longlong_as_double((long long)th.keys[(size_t)R * (size_t)R + 1]);
    th.h[0] = 0.0; th.h[1] = 0.0; th.h[2] = 0.0;           // the corners lie in the plane
  }
  uint32_t ccol[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double* d = reinterpret_cast<const double*>(verts + (size_t)fv[c] * 80);
    const int* ci = reinterpret_cast<const int*>(verts + (size_t)fv[c] * 80 + 48);
    c3[c][0] = d[0]; c3[c][1] = d[1]; c3[c][2] = d[2];
    cu[c] = d[8]; cv[c] = d[9];
    if constexpr (NRM) { tn.v[c][0] = d[3]; tn.v[c][1] = d[4]; tn.v[c][2] = d[5]; }
    ccol[c] = (uint32_t)min(max(ci[0], 0), 255) | ((uint32_t)min(max(ci[1], 0), 255) << 8) | ((uint32_t)min(max(ci[2], 0), 255) << 16);
  }
  // ---- union of the three neighbour lists, by original index, ascending -----------------------------------------------
  const int nraw = 3 * k;
  for (int e = lane; e < BK_MAXNBR + 32; e += 64) {
    uint32_t id = PT_NOIDX_U;
    if (e < nraw) { id = nbr[(size_t)fv[e / k] * (size_t)k + (size_t)(e % k)]; if (id >= n) id = PT_NOIDX_U; }
    W.raw[e] = id;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  int nid = 0;
  {
    uint32_t val[2], pos[2];
    bool first[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int e = lane + 64 * h;
      val[h] = W.raw[e];
      first[h] = val[h] != PT_NOIDX_U;
      for (int q = 0; q < nraw && q < e; ++q) if (W.raw[q] == val[h]) first[h] = false;     // an equal index earlier in the lists
      W.cin[e] = first[h] ? 1 : 0;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      pos[h] = 0;
      for (int q = 0; q < nraw; ++q) if (W.cin[q] && W.raw[q] < val[h]) ++pos[h];           // rank among the distinct values
    }
    nid = (int)__popcll(__ballot(first[0])) + (int)__popcll(__ballot(first[1]));
#pragma unroll
    for (int h = 0; h < 2; ++h) if (first[h]) W.sorted[pos[h]] = val[h];
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  // ---- plane frame: origin corner 0, e1 along corner 0 -> 1, e2 = n x e1 (every lane computes the same values) ---------
  const double ax = c3[1][0] - c3[0][0], ay = c3[1][1] - c3[0][1], az = c3[1][2] - c3[0][2];
  const double bx = c3[2][0] - c3[0][0], by = c3[2][1] - c3[0][1], bz = c3[2][2] - c3[0][2];
  const double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
  const double la = sqrt((ax * ax + ay * ay) + az * az);
  const double e1x = ax / la, e1y = ay / la, e1z = az / la;
  const double tx = ny * e1z - nz * e1y, ty = nz * e1x - nx * e1z, tz = nx * e1y - ny * e1x;
  const double lt = sqrt((tx * tx + ty * ty) + tz * tz);
  const double e2x = tx / lt, e2y = ty / lt, e2z = tz / lt;
  const bool frame_ok = la > 0.0 && lt > 0.0 && finite_d(la) && finite_d(lt);
  const double P0x = 0.0, P0y = 0.0;
  const double P1x = (ax * e1x + ay * e1y) + az * e1z, P1y = (ax * e2x + ay * e2y) + az * e2z;
  const double P2x = (bx * e1x + by * e1y) + bz * e1z, P2y = (bx * e2x + by * e2y) + bz * e2z;
  const double A = frame_ok ? cross2(P1x - P0x, P1y - P0y, P2x - P0x, P2y - P0y) : 0.0;
  if (lane < 3) {
    W.px[lane] = lane == 0 ? P0x : (lane == 1 ? P1x : P2x);
    W.py[lane] = lane == 0 ? P0y : (lane == 1 ? P1y : P2y);
    W.pu[lane] = cu[lane]; W.pv[lane] = cv[lane]; W.pc[lane] = ccol[lane];
    if constexpr (NRM) {                                   // (selects, not tn.v[lane]: a lane-indexed register array would live in scratch)
      W.pnx[lane] = lane == 0 ? tn.v[0][0] : (lane == 1 ? tn.v[1][0] : tn.v[2][0]);
      W.pny[lane] = lane == 0 ? tn.v[0][1] : (lane == 1 ? tn.v[1][1] : tn.v[2][1]);
      W.pnz[lane] = lane == 0 ? tn.v[0][2] : (lane == 1 ? tn.v[1][2] : tn.v[2][2]);
    }
    if constexpr (HGT) W.ph[lane] = 0.0;
  }
  int np = 3;
  if (frame_ok && A != 0.0 && finite_d(A)) {
    // unit face normal (height plane): e1, e2, e3 is right-handed; unusable -> every interior height is 0
    [[maybe_unused]] double e3x = 0.0, e3y = 0.0, e3z = 0.0, hc[2] = {0.0, 0.0};
    if constexpr (HGT) {
      const double ln = sqrt((nx * nx + ny * ny) + nz * nz);
      if (ln > 0.0 && finite_d(ln)) { e3x = nx / ln; e3y = ny / ln; e3z = nz / ln; }
    }
    // ---- project the candidates, keep what is inside the face (:505-537) ----------------------------------------------
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int e = lane + 64 * h;
      bool inside = false;
      if (e < nid) {
        const size_t id = W.sorted[e];
        const double dx = (double)sx[id] - c3[0][0], dy = (double)sy[id] - c3[0][1], dz = (double)sz[id] - c3[0][2];
        const double Xx = (dx * e1x + dy * e1y) + dz * e1z, Xy = (dx * e2x + dy * e2y) + dz * e2z;
        double b[3];
        bary2(Xx, Xy, P0x, P0y, P1x, P1y, P2x, P2y, A, b);
        inside = b[0] >= 0 && b[1] >= 0 && b[2] >= 0;
        W.cx[e] = Xx; W.cy[e] = Xy;
        W.cu[e] = (b[0] * cu[0] + b[1] * cu[1]) + b[2] * cu[2];             // :571-572
        W.cv[e] = (b[0] * cv[0] + b[1] * cv[1]) + b[2] * cv[2];
        if constexpr (HGT) hc[h] = (dx * e3x + dy * e3y) + dz * e3z;
      }
      if (e < BK_MAXNBR + 32) W.cin[e] = inside ? 1 : 0;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // a candidate whose 2-D image equals a corner's or an EARLIER inside candidate's is dropped (the earliest of equals stays)
    bool keep[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int e = lane + 64 * h;
      keep[h] = e < nid && W.cin[e];
      if (keep[h]) {
        const double Xx = W.cx[e], Xy = W.cy[e];
        if ((Xx == P0x && Xy == P0y) || (Xx == P1x && Xy == P1y) || (Xx == P2x && Xy == P2y)) keep[h] = false;
        for (int q = 0; q < e; ++q) if (W.cin[q] && W.cx[q] == Xx && W.cy[q] == Xy) keep[h] = false;
      }
    }
    const unsigned long long m0 = __ballot(keep[0]), m1 = __ballot(keep[1]);
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (keep[h]) {
        const int e = lane + 64 * h;
        const int slot = 3 + (h ? (int)__popcll(m0) + (int)__popcll(m1 & below) : (int)__popcll(m0 & below));
        W.px[slot] = W.cx[e]; W.py[slot] = W.cy[e]; W.pu[slot] = W.cu[e]; W.pv[slot] = W.cv[e];
        W.pc[slot] = attr[W.sorted[e]].rgba & 0xFFFFFFu;
        if constexpr (NRM) { const Attr a = attr[W.sorted[e]]; W.pnx[slot] = (double)a.nx; W.pny[slot] = (double)a.ny; W.pnz[slot] = (double)a.nz; }
        if constexpr (HGT) W.ph[slot] = hc[h];
      }
    }
    np = 3 + (int)__popcll(m0) + (int)__popcll(m1);
    if constexpr (HGT) {
      // max |h| over the wave's interior kept points with a finite height; one atomic per wave, and none when it cannot raise the value
      double mh = 0.0;
#pragma unroll
      for (int h = 0; h < 2; ++h) if (keep[h] && finite_d(hc[h])) mh = fmax(mh, fabs(hc[h]));
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) mh = fmax(mh, __shfl_xor(mh, d, 64));
      if (lane == 0 && mh > 0.0) {
        unsigned long long* const slot = th.keys + (size_t)R * (size_t)R;
        const unsigned long long bits = (unsigned long long)__double_as_longlong(mh);      // monotone for non-negative doubles
        if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < bits) atomicMax(slot, bits);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  const unsigned long long seq0 = (unsigned long long)f * 256ull + 1ull;
  if (np == 3) {                                            // no interior points: the face itself (:540-544)
    draw_triangle<MAPS>(cu, cv, ccol, R, seq0, keys, lane, tn, th);
    return;
  }
  // ---- Delaunay by exhaustion: triples in lexicographic order, lanes over k (:546-581 with the build's definition) --------
  int ntri = 0;
  for (int i = 0; i < np - 2; ++i)
    for (int j = i + 1; j < np - 1; ++j)
      for (int kb = j + 1; kb < np; kb += 64) {
        const int kk = kb + lane;
        bool ok = false;
        if (kk < np) {
          const double o = cross2(W.px[j] - W.px[i], W.py[j] - W.py[i], W.px[kk] - W.px[i], W.py[kk] - W.py[i]);
          if (o != 0.0) {
            const int os = o > 0.0 ? 1 : -1;
            ok = true;
            for (int l = 0; l < np && ok; ++l)
              if (l != i && l != j && l != kk && in_circumcircle(W.px, W.py, i, j, kk, l, os)) ok = false;
          }
        }
        const unsigned long long m = __ballot(ok);
        if (ok) {
          const int slot = ntri + (int)__popcll(m & (lane ? (~0ull >> (64 - lane)) : 0ull));
          if (slot < BK_MAXTRI) W.tri[slot] = (uint32_t)i | ((uint32_t)j << 8) | ((uint32_t)kk << 16);
        }
        ntri += (int)__popcll(m);
      }
  if (ntri > BK_MAXTRI) ntri = BK_MAXTRI;                   // (2 np - 5 <= 193 triangles unless many points are co-circular)
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  for (int t = 0; t < ntri; ++t) {
    const uint32_t tr = W.tri[t];
    const int a = (int)(tr & 0xFFu), b = (int)((tr >> 8) & 0xFFu), c = (int)((tr >> 16) & 0xFFu);
    const double U[3] = {W.pu[a], W.pu[b], W.pu[c]}, V[3] = {W.pv[a], W.pv[b], W.pv[c]};
    const uint32_t col[3] = {W.pc[a], W.pc[b], W.pc[c]};
    if constexpr (NRM) {
      tn.v[0][0] = W.pnx[a]; tn.v[0][1] = W.pny[a]; tn.v[0][2] = W.pnz[a];
      tn.v[1][0] = W.pnx[b]; tn.v[1][1] = W.pny[b]; tn.v[1][2] = W.pnz[b];
      tn.v[2][0] = W.pnx[c]; tn.v[2][1] = W.pny[c]; tn.v[2][2] = W.pnz[c];
    }
    if constexpr (HGT) { th.h[0] = W.ph[a]; th.h[1] = W.ph[b]; th.h[2] = W.ph[c]; }
    draw_triangle<MAPS>(U, V, col, R, seq0 + (unsigned long long)t, keys, lane, tn, th);
  }
}

__global__ __launch_bounds__(BK_WG) void bake_resolve_kernel(const unsigned long long* __restrict__ keys, uint32_t* __restrict__ bgra, size_t npix) {
  const size_t i = (size_t)blockIdx.x * BK_WG + threadIdx.x;
  if (i < npix) bgra[i] = (uint32_t)(keys[i] & 0xFFFFFFFFull);           // untouched pixels hold key 0: transparent black
}

__device__ inline uint32_t bytemax(uint32_t a, uint32_t b) {
  uint32_t r = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) { const uint32_t x = (a >> (8 * c)) & 0xFFu, y = (b >> (8 * c)) & 0xFFu; r |= (x > y ? x : y) << (8 * c); }
  return r;
}
// separable ksize x ksize maximum per channel (what lies outside the image does not count), reference :594-597
__global__ __launch_bounds__(BK_WG) void dilate_rows_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int R, int h) {
  const size_t i = (size_t)blockIdx.x * BK_WG + threadIdx.x;
  if (i >= (size_t)R * R) return;
  const int x = (int)(i % (size_t)R);
  const size_t row = i - (size_t)x;
  uint32_t m = 0;
  for (int d = -h; d <= h; ++d) { const int xx = x + d; if (xx >= 0 && xx < R) m = bytemax(m, in[row + (size_t)xx]); }
  out[i] = m;
}
// vertical maximum of the row maxima, then edges = dilated & ~alpha (all four channels), padded = texture + edges, saturating (:598-611)
__global__ __launch_bounds__(BK_WG) void dilate_cols_pad_kernel(const uint32_t* __restrict__ rows, const uint32_t* __restrict__ tex, uint32_t* __restrict__ out,
                                                                int R, int h) {
  const size_t i = (size_t)blockIdx.x * BK_WG + threadIdx.x;
  if (i >= (size_t)R * R) return;
  const int x = (int)(i % (size_t)R), y = (int)(i / (size_t)R);
  uint32_t m = 0;
  for (int d = -h; d <= h; ++d) { const int yy = y + d; if (yy >= 0 && yy < R) m = bytemax(m, rows[(size_t)yy * R + x]); }
  const uint32_t t = tex[i];
  const uint32_t mask = (~(t >> 24)) & 0xFFu;
  uint32_t r = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const uint32_t s = ((t >> (8 * c)) & 0xFFu) + (((m >> (8 * c)) & 0xFFu) & mask);
    r |= (s > 255u ? 255u : s) << (8 * c);
  }
  out[i] = r;
}

}  // namespace

template <class T>
void pt_launch_bake_faces(const T* sx, const T* sy, const T* sz, const Attr* attr, uint32_t n, const void* verts_aos, uint32_t nv, const int32_t* faces,
                          uint32_t nf, const uint32_t* nbr, int k, int R, int maps, unsigned long long* keys, hipStream_t s) {
  if (!nf) return;
  const dim3 grid((nf + BK_WAVES - 1) / BK_WAVES), wg(BK_WG);
  const unsigned char* verts = (const unsigned char*)verts_aos;
#define BK_LAUNCH(...) hipLaunchKernelGGL((bake_faces_kernel<__VA_ARGS__>), grid, wg, 0, s, sx, sy, sz, attr, n, verts, nv, faces, nf, nbr, k, R, keys)
  switch (maps) {
    case BK_COLOR: BK_LAUNCH(T); break;
    case BK_NORMAL: BK_LAUNCH(WithMaps<T, BK_NORMAL>); break;
    case BK_COLOR | BK_NORMAL: BK_LAUNCH(WithMaps<T, BK_COLOR | BK_NORMAL>); break;
    case BK_HEIGHT: BK_LAUNCH(WithMaps<T, BK_HEIGHT>); break;
    case BK_HEIGHT | BK_COLOR: BK_LAUNCH(WithMaps<T, BK_HEIGHT | BK_COLOR>); break;
    case BK_HEIGHT | BK_NORMAL: BK_LAUNCH(WithMaps<T, BK_HEIGHT | BK_NORMAL>); break;
    case BK_HEIGHT | BK_NORMAL | BK_COLOR: BK_LAUNCH(WithMaps<T, BK_HEIGHT | BK_NORMAL | BK_COLOR>); break;
    default: break;                                        // (the C ABI admits no other set)
  }
#undef BK_LAUNCH
}
template void pt_launch_bake_faces<float>(const float*, const float*, const float*, const Attr*, uint32_t, const void*, uint32_t, const int32_t*, uint32_t,
                                          const uint32_t*, int, int, int, unsigned long long*, hipStream_t);
template void pt_launch_bake_faces<double>(const double*, const double*, const double*, const Attr*, uint32_t, const void*, uint32_t, const int32_t*, uint32_t,
                                           const uint32_t*, int, int, int, unsigned long long*, hipStream_t);
void pt_launch_bake_resolve(const unsigned long long* keys, uint32_t* bgra, size_t npix, hipStream_t s) {
  if (!npix) return;
  hipLaunchKernelGGL(bake_resolve_kernel, dim3((uint32_t)((npix + BK_WG - 1) / BK_WG)), dim3(BK_WG), 0, s, keys, bgra, npix);
}
void pt_launch_dilate_pad(const uint32_t* tex, uint32_t* tmp, uint32_t* out, int R, int ksize, hipStream_t s) {
  const size_t npix = (size_t)R * R;
  if (!npix) return;
  const uint32_t g = (uint32_t)((npix + BK_WG - 1) / BK_WG);
  hipLaunchKernelGGL(dilate_rows_kernel, dim3(g), dim3(BK_WG), 0, s, tex, tmp, R, ksize / 2);
  hipLaunchKernelGGL(dilate_cols_pad_kernel, dim3(g), dim3(BK_WG), 0, s, tmp, tex, out, R, ksize / 2);
}
