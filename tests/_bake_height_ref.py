"""The height map of DESIGN.md section 8 ("Height map"), restated from its table in numpy float64 (numpy rounds every operation on
its own; the kernel is compiled with contraction off):

  kept points, triangles, coverage   _bake_ref's: face_points, the caller's triangulation, and draw() decides which pixels a triangle covers
                                     (taken as _bake_normal_ref.draw_normals takes them).  Which source point a kept point is comes out
                                     of face_points through an index-coded colour
  face normal                        a = c1 - c0, b = c2 - c0, n = a x b;  ln = sqrt((nx nx + ny ny) + nz nz);  e3 = n / ln
  a kept point's height              corner: 0;  interior point: h = (dx e3x + dy e3y) + dz e3z with d = source point - c0;  0 for every
                                     interior point unless 0 < ln < inf
  per covered pixel                  b from the rasteriser's formulas;  m = (b0 h0 + b1 h1) + b2 h2;  m not finite: byte = 128;  otherwise
                                     t = m / H;  u = t * 127.5 + 127.5;  byte = (int)min(max(u + 0.5, 0), 255)
  pixel                              BGRA bytes {byte, byte, byte, 255}; a later (face, triangle) overwrites an earlier one; untouched pixels are 0
  max_abs_height                     max |h| over the interior kept points with a finite h, over all well-formed faces; 0 when there is none
"""
import numpy as np

import _bake_normal_ref as NR
import _bake_ref as B


def encode(m, H):
    """(...) float64 mixes -> (..., 4) uint8 BGRA pixels"""
    m = np.asarray(m, np.float64)
    with np.errstate(all="ignore"):
        t = m / np.float64(H)
        u = t * 127.5 + 127.5
        r = np.minimum(np.maximum(u + 0.5, 0.0), 255.0)
        byte = np.where(np.isfinite(m), r, 128.0).astype(np.int64).astype(np.uint8)
    out = np.empty(m.shape + (4,), np.uint8)
    out[..., 0] = byte; out[..., 1] = byte; out[..., 2] = byte; out[..., 3] = 255
    return out


def face_heights(src_xyz, vert_xyz, vert_uv, fv, nbr_idx):
    """(P, UV, H, ids) of a well-formed face: _bake_ref.face_points' kept points with their heights (corners first: 0) and the interior
    points' source indices"""
    n = src_xyz.shape[1]
    _, P, UV, code = B.face_points(src_xyz, NR.index_colours(n), vert_xyz, vert_uv, np.zeros((vert_xyz.shape[1], 3), np.int64), fv, nbr_idx)
    ids = code[3:, 0] + (code[3:, 1] << 8) + (code[3:, 2] << 16)
    c = [np.array([np.float64(vert_xyz[a, v]) for a in range(3)]) for v in fv]
    H = np.zeros(len(P))
    with np.errstate(all="ignore"):
        a, b = c[1] - c[0], c[2] - c[0]
        nx, ny, nz = a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]
        ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
        if ln > 0 and np.isfinite(ln):
            e3x, e3y, e3z = nx / ln, ny / ln, nz / ln
            for s, i in enumerate(ids):
                dx, dy, dz = (np.float64(src_xyz[q, i]) - c[0][q] for q in range(3))
                H[3 + s] = (dx * e3x + dy * e3y) + dz * e3z
    return P, UV, H, ids


def draw_heights(tex, cov, U, V, h, R, H, mix=None):
    """One triangle into tex (and its raw mixes into `mix`, an (R, R) float64 plane, when given).  The covered pixels are
    _bake_ref.draw's (drawn into the scratch atlas `cov`, all zero on entry and on exit); their barycentrics follow from the
    rasteriser's formulas at (x, y) = (column, min(R - row, R - 1))."""
    B.draw(cov, U, V, np.zeros((3, 3)), R)
    rows, cols = np.nonzero(cov[:, :, 3])
    if not len(rows):
        return
    cov[rows, cols] = 0
    with np.errstate(all="ignore"):
        px, py, qx, qy, rx, ry = (np.float64(v) * R for v in (U[0], V[0], U[1], V[1], U[2], V[2]))
        A = (qx - px) * (ry - py) - (qy - py) * (rx - px)
        x = cols.astype(np.float64); y = np.minimum(R - rows, R - 1).astype(np.float64)
        b0 = ((qx - x) * (ry - y) - (qy - y) * (rx - x)) / A
        b1 = ((rx - x) * (py - y) - (ry - y) * (px - x)) / A
        b2 = (1.0 - b0) - b1
        m = (b0 * h[0] + b1 * h[1]) + b2 * h[2]
    tex[rows, cols] = encode(m, H)
    if mix is not None:
        mix[rows, cols] = m


def bake(src_xyz, vert_xyz, vert_uv, faces, nbr_idx, R, H, triangulate, mix=None):
    """((R, R, 4) BGRA height map, max_abs_height) for height_range H"""
    src_xyz = np.asarray(src_xyz, np.float64); vert_xyz = np.asarray(vert_xyz, np.float64)
    nv = vert_xyz.shape[1]
    tex = np.zeros((R, R, 4), np.uint8); cov = np.zeros((R, R, 4), np.uint8)
    top = 0.0
    for fv in np.asarray(faces).reshape(-1, 3):
        if any(v < 0 or v >= nv for v in fv):
            continue
        P, UV, h, _ = face_heights(src_xyz, vert_xyz, vert_uv, fv, nbr_idx)
        fin = np.abs(h[3:][np.isfinite(h[3:])])
        if len(fin):
            top = max(top, float(fin.max()))
        tris = np.array([[0, 1, 2]]) if len(P) == 3 else triangulate(P)[:B.MAXTRI]
        for t in tris:
            draw_heights(tex, cov, UV[t, 0], UV[t, 1], h[t], R, H, mix)
    return tex, top
