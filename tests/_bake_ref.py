"""The texture bake of DESIGN.md section 8, restated from its table in numpy float64 (numpy rounds every operation on its own) --
a second opinion on oracle/pt_oracle.c::pto_bake_texture that shares no code with it and does not follow its loops:

  union of the corners' lists       np.unique of the three rows, entries >= n dropped
  plane frame                       origin corner 0, e1 along corner 0 -> 1, e2 = n x e1, both unit; unusable (zero, non-finite) -> plain face
  inside test                       the three barycentrics of the 2-D image, all >= 0
  coincident projections            a point whose image equals a corner's or an earlier kept point's is dropped
  Delaunay                          NOT the oracle's fp64 sorted-tuple predicate: either scipy.spatial.Delaunay (points verified to be
                                    in general position with exact arithmetic) or exhaustive empty-circle with exact integer predicates
  order                             triangles as sorted index triples in lexicographic order, at most 255 of them
  rasteriser                        the reference's pixel loop; a later (face, triangle) overwrites an earlier one
"""
from fractions import Fraction
from itertools import combinations

import numpy as np

NOIDX = 0xFFFFFFFF
MAXTRI = 255
_EPS = 2.0 ** -53


# ---- rasteriser ----------------------------------------------------------------------------------------------------------------
def draw(tex, U, V, col, R):
    """reference draw_triangle (:66-107) over the bounding box at once: the operations of test_bake_oracle._numpy_draw on arrays.
    Pixels outside the atlas are skipped; a triangle with a non-finite or zero doubled area draws nothing."""
    with np.errstate(all="ignore"):
        px, py, qx, qy, rx, ry = (np.float64(v) * R for v in (U[0], V[0], U[1], V[1], U[2], V[2]))
        if not np.all(np.isfinite([px, py, qx, qy, rx, ry])):
            return
        A = (qx - px) * (ry - py) - (qy - py) * (rx - px)
        if A == 0 or not np.isfinite(A):
            return
        lo_i, hi_i = np.floor(min(px, qx, rx)), np.floor(max(px, qx, rx))
        lo_j, hi_j = np.floor(min(py, qy, ry)), np.floor(max(py, qy, ry))
        if hi_i < 0 or lo_i > R - 1 or hi_j < 1 or lo_j > R:
            return
        i = np.arange(int(max(lo_i, 0)), int(min(hi_i, R - 1)) + 1)[None, :]
        j = np.arange(int(max(lo_j, 1)), int(min(hi_j, R)) + 1)[:, None]
        x = np.minimum(i, R - 1).astype(np.float64); y = np.minimum(j, R - 1).astype(np.float64)
        b0 = ((qx - x) * (ry - y) - (qy - y) * (rx - x)) / A
        b1 = ((rx - x) * (py - y) - (ry - y) * (px - x)) / A
        b2 = (1.0 - b0) - b1
        m = (b0 >= 0) & (b1 >= 0) & (b2 >= 0)
        jj, ii = np.nonzero(m)
        rows, cols = R - j[jj, 0], i[0, ii]
        for c in range(3):
            f = ((b0[m] * float(col[0][c]) + b1[m] * float(col[1][c])) + b2[m] * float(col[2][c])).astype(np.float32)
            tex[rows, cols, 2 - c] = np.clip(f, np.float32(0), np.float32(255)).astype(np.uint8)
        tex[rows, cols, 3] = 255


# ---- exact predicates ------------------------------------------------------------------------------------------------------------
def _as_ints(P):
    """the fp64 coordinates as exact integers on one power-of-two grid (object array of Python ints)"""
    fr = [[Fraction(float(v)) for v in p] for p in P]
    den = max([f.denominator for p in fr for f in p] + [1])
    return np.array([[int(f * den) for f in p] for p in fr], dtype=object).reshape(len(fr), 2)


def _small(Z):
    return all(abs(int(v)) < (1 << 13) for v in Z.ravel())


def _orient(Z, a, b, c):
    return (Z[b, 0] - Z[a, 0]) * (Z[c, 1] - Z[a, 1]) - (Z[b, 1] - Z[a, 1]) * (Z[c, 0] - Z[a, 0])


def _incircle(Z, a, b, c, d):
    """> 0 iff d lies strictly inside the circle through a, b, c taken counter-clockwise (the textbook lifted determinant)"""
    ax, ay = Z[a, 0] - Z[d, 0], Z[a, 1] - Z[d, 1]
    bx, by = Z[b, 0] - Z[d, 0], Z[b, 1] - Z[d, 1]
    cx, cy = Z[c, 0] - Z[d, 0], Z[c, 1] - Z[d, 1]
    return (ax * ax + ay * ay) * (bx * cy - by * cx) + (bx * bx + by * by) * (cx * ay - cy * ax) + (cx * cx + cy * cy) * (ax * by - ay * bx)


def exact_delaunay(P):
    """Every triple i < j < k of non-zero orientation whose circumcircle holds no other point strictly inside, in lexicographic
    order, decided in exact integer arithmetic on the fp64 coordinates.  Returns the full (uncapped) list as an (m, 3) array."""
    Z = _as_ints(P)
    if _small(Z):
        Z = Z.astype(np.int64)                      # |coordinate| < 2**13: the determinant stays below 2**60
    n = len(Z)
    out = []
    ls = np.arange(n)
    for i in range(n - 2):
        jj, kk = np.triu_indices(n, 1)
        sel = jj > i
        jj, kk = jj[sel], kk[sel]
        o = _orient(Z, i, jj, kk)
        nz = np.nonzero(o != 0)[0]
        jj, kk, o = jj[nz], kk[nz], o[nz]
        d = _incircle(Z, i, jj[:, None], kk[:, None], ls[None, :])
        inside = (np.sign(o)[:, None] * np.sign(d)) > 0       # a, b, c themselves give 0
        for t in np.nonzero(~inside.any(axis=1))[0]:
            out.append((i, int(jj[t]), int(kk[t])))
    return np.array(sorted(out), np.int64).reshape(-1, 3)


def general_position(P):
    """True iff, for EVERY four of the points, the in-circle determinant the oracle would evaluate (fp64, on the index-sorted tuple)
    is non-zero and has the sign of the exact determinant, and every three have a non-zero orientation with the fp64 sign.  The
    fp64 value is certified by Shewchuk's static error bound where that suffices ((10 + 96 eps) eps times the permanent for the
    in-circle form, (3 + 16 eps) eps for the orientation) and by exact integers where it does not."""
    P = np.asarray(P, np.float64)
    n = len(P)
    Z = None
    t = np.array(list(combinations(range(n), 3)), np.int64)
    a, b, c = P[t[:, 0]], P[t[:, 1]], P[t[:, 2]]
    l, r = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]), (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])
    o = l - r
    for s in np.nonzero(~(np.abs(o) > (3 + 16 * _EPS) * _EPS * (np.abs(l) + np.abs(r))))[0]:
        Z = _as_ints(P) if Z is None else Z
        e = _orient(Z, *t[s])
        if e == 0 or (e > 0) != (o[s] > 0):
            return False
    q = np.array(list(combinations(range(n), 4)), np.int64)
    for lo in range(0, len(q), 1 << 20):
        w, x, y, z = (P[q[lo:lo + (1 << 20), m]] for m in range(4))
        adx, ady, bdx, bdy, cdx, cdy = w[:, 0] - z[:, 0], w[:, 1] - z[:, 1], x[:, 0] - z[:, 0], x[:, 1] - z[:, 1], y[:, 0] - z[:, 0], y[:, 1] - z[:, 1]
        al, bl, cl = adx * adx + ady * ady, bdx * bdx + bdy * bdy, cdx * cdx + cdy * cdy
        d = (al * (bdx * cdy - bdy * cdx) - bl * (adx * cdy - ady * cdx)) + cl * (adx * bdy - ady * bdx)
        perm = (np.abs(bdx * cdy) + np.abs(bdy * cdx)) * al + (np.abs(adx * cdy) + np.abs(ady * cdx)) * bl + (np.abs(adx * bdy) + np.abs(ady * bdx)) * cl
        for s in np.nonzero(~(np.abs(d) > (10 + 96 * _EPS) * _EPS * perm))[0]:
            Z = _as_ints(P) if Z is None else Z
            e = _incircle(Z, *q[lo + s])
            if e == 0 or (e > 0) != (d[s] > 0):
                return False
    return True


def scipy_delaunay(P):
    """scipy's (Qhull's) triangulation as sorted triples in lexicographic order; meaningful only in general position"""
    from scipy.spatial import Delaunay
    s = np.sort(Delaunay(np.asarray(P, np.float64)).simplices.astype(np.int64), axis=1)
    return s[np.lexsort((s[:, 2], s[:, 1], s[:, 0]))]


def hull_size(P):
    from scipy.spatial import ConvexHull
    return len(ConvexHull(np.asarray(P, np.float64)).vertices)


def tri_area2(P, tris):
    """sum over the triangles of |doubled area|"""
    P = np.asarray(P, np.float64)
    a, b, c = P[tris[:, 0]], P[tris[:, 1]], P[tris[:, 2]]
    return np.abs((b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])).sum()


# ---- one face ----------------------------------------------------------------------------------------------------------------------
def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _cross(u, v):
    return np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]])


def _cross2(ax, ay, bx, by):
    return ax * by - ay * bx


def _bary(X, P0, P1, P2, A):
    b0 = _cross2(P1[0] - X[0], P1[1] - X[1], P2[0] - X[0], P2[1] - X[1]) / A
    b1 = _cross2(P2[0] - X[0], P2[1] - X[1], P0[0] - X[0], P0[1] - X[1]) / A
    return b0, b1, (1.0 - b0) - b1


def face_points(src_xyz, src_rgb, vert_xyz, vert_uv, vert_rgb, fv, nbr_idx):
    """(ids, P (np, 2), UV (np, 2), RGB (np, 3)) of a well-formed face: corners first, then the kept points by ascending index"""
    n = src_xyz.shape[1]
    ids = np.unique(np.asarray(nbr_idx, np.uint32)[list(fv)].ravel())
    ids = ids[ids < n]
    c = [np.array([np.float64(vert_xyz[a, v]) for a in range(3)]) for v in fv]
    uv = [np.array(vert_uv[v], np.float64) for v in fv]
    P, UV, RGB = [], [uv[0], uv[1], uv[2]], [np.clip(np.asarray(vert_rgb[v], np.int64), 0, 255) for v in fv]
    with np.errstate(all="ignore"):
        a, b = c[1] - c[0], c[2] - c[0]
        nrm = _cross(a, b)
        la = np.sqrt(_dot(a, a))
        e1 = a / la
        t = _cross(nrm, e1)
        lt = np.sqrt(_dot(t, t))
        e2 = t / lt
        P = [np.array([0.0, 0.0]), np.array([_dot(a, e1), _dot(a, e2)]), np.array([_dot(b, e1), _dot(b, e2)])]
        ok = la > 0 and lt > 0 and np.isfinite(la) and np.isfinite(lt)
        A = _cross2(P[1][0], P[1][1], P[2][0], P[2][1]) if ok else 0.0
        if ok and A != 0 and np.isfinite(A):
            for i in ids:
                d = np.array([np.float64(src_xyz[a_, i]) for a_ in range(3)]) - c[0]
                X = np.array([_dot(d, e1), _dot(d, e2)])
                b0, b1, b2 = _bary(X, P[0], P[1], P[2], A)
                if not (b0 >= 0 and b1 >= 0 and b2 >= 0):
                    continue
                if any(X[0] == Q[0] and X[1] == Q[1] for Q in P):
                    continue
                P.append(X)
                UV.append((b0 * uv[0] + b1 * uv[1]) + b2 * uv[2])
                RGB.append(np.asarray(src_rgb[i], np.int64))
    return ids, np.array(P), np.array(UV), np.array(RGB)


def bake(src_xyz, src_rgb, vert_xyz, vert_uv, vert_rgb, faces, nbr_idx, R, triangulate):
    """The (R, R, 4) BGRA atlas.  triangulate(P) -> (m, 3) sorted triples in lexicographic order (scipy_delaunay or exact_delaunay)."""
    src_xyz = np.asarray(src_xyz, np.float64); vert_xyz = np.asarray(vert_xyz, np.float64)
    nv = vert_xyz.shape[1]
    tex = np.zeros((R, R, 4), np.uint8)
    for fv in np.asarray(faces).reshape(-1, 3):
        if any(v < 0 or v >= nv for v in fv):
            continue
        _, P, UV, RGB = face_points(src_xyz, src_rgb, vert_xyz, vert_uv, vert_rgb, fv, nbr_idx)
        tris = np.array([[0, 1, 2]]) if len(P) == 3 else triangulate(P)[:MAXTRI]
        for t in tris:
            draw(tex, UV[t, 0], UV[t, 1], RGB[t], R)
    return tex
