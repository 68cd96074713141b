"""The object-space normal map of DESIGN.md section 8 ("Normal map"), restated from its table in numpy float64 (numpy rounds every
operation on its own; the kernel is compiled with contraction off):

  kept points, triangles, coverage   _bake_ref's: face_points, the caller's triangulation, and draw() decides which pixels a triangle covers
  a kept point's normal              corner: the mesh vertex's normal (double); interior point: the source point's normal as the GPU holds
                                     it (float32, widened) -- NOT normalised.  Which source point a kept point is comes out of face_points
                                     through an index-coded colour
  per covered pixel                  b from the rasteriser's formulas;  m_c = (b0 n0_c + b1 n1_c) + b2 n2_c;  l = sqrt((mx mx + my my) + mz mz);
                                     u = m / l if 0 < l < inf else (0, 0, 1);  t_c = u_c * 127.5 + 127.5;  byte_c = clamp((int)(t_c + 0.5), 0, 255)
  pixel                              BGRA bytes {z, y, x, 255}; a later (face, triangle) overwrites an earlier one; untouched pixels are 0
"""
import numpy as np

import _bake_ref as B


def encode(m):
    """(..., 3) float64 mixes -> (..., 4) uint8 BGRA pixels"""
    m = np.asarray(m, np.float64)
    with np.errstate(all="ignore"):
        mx, my, mz = m[..., 0], m[..., 1], m[..., 2]
        l = np.sqrt((mx * mx + my * my) + mz * mz)
        ok = (l > 0) & np.isfinite(l)
        out = np.zeros(m.shape[:-1] + (4,), np.uint8)
        for c in range(3):
            u = np.where(ok, m[..., c] / l, 1.0 if c == 2 else 0.0)
            t = u * 127.5 + 127.5
            out[..., 2 - c] = np.clip((t + 0.5).astype(np.int64), 0, 255).astype(np.uint8)
    out[..., 3] = 255
    return out


def index_colours(n):
    """colours that spell the point's index (n < 2**24): what face_points hands back for a kept interior point"""
    assert n < (1 << 24)
    i = np.arange(n, dtype=np.int64)
    return np.stack([i & 255, (i >> 8) & 255, (i >> 16) & 255], axis=1)


def face_normals(src_xyz, src_nrm, vert_xyz, vert_uv, vert_nrm, fv, nbr_idx):
    """(P, UV, N) of a well-formed face: _bake_ref.face_points' kept points with their normals (corners first)"""
    n = src_xyz.shape[1]
    _, P, UV, code = B.face_points(src_xyz, index_colours(n), vert_xyz, vert_uv, np.zeros((vert_xyz.shape[1], 3), np.int64), fv, nbr_idx)
    ids = code[3:, 0] + (code[3:, 1] << 8) + (code[3:, 2] << 16)
    N = np.concatenate([np.asarray(vert_nrm, np.float64)[list(fv)], np.asarray(src_nrm, np.float64).reshape(-1, 3)[ids]])
    return P, UV, N


def draw_normals(tex, cov, U, V, N, R):
    """One triangle into tex.  The covered pixels are _bake_ref.draw's (drawn into the scratch atlas `cov`, all zero on entry and on
    exit); their barycentrics follow from the rasteriser's formulas at (x, y) = (column, min(R - row, R - 1))."""
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
        m = np.stack([(b0 * N[0][c] + b1 * N[1][c]) + b2 * N[2][c] for c in range(3)], axis=1)
    tex[rows, cols] = encode(m)


def bake(src_xyz, src_nrm, vert_xyz, vert_uv, vert_nrm, faces, nbr_idx, R, triangulate):
    """The (R, R, 4) BGRA normal map.  src_nrm (n, 3): the cloud's normals as the GPU holds them; vert_nrm (nv, 3) float64."""
    src_xyz = np.asarray(src_xyz, np.float64); vert_xyz = np.asarray(vert_xyz, np.float64)
    nv = vert_xyz.shape[1]
    tex = np.zeros((R, R, 4), np.uint8); cov = np.zeros((R, R, 4), np.uint8)
    for fv in np.asarray(faces).reshape(-1, 3):
        if any(v < 0 or v >= nv for v in fv):
            continue
        P, UV, N = face_normals(src_xyz, src_nrm, vert_xyz, vert_uv, vert_nrm, fv, nbr_idx)
        tris = np.array([[0, 1, 2]]) if len(P) == 3 else triangulate(P)[:B.MAXTRI]
        for t in tris:
            draw_normals(tex, cov, UV[t, 0], UV[t, 1], N[t], R)
    return tex


def faces_in_general_position(src_xyz, vert_xyz, vert_uv, faces, nbr_idx):
    """True iff every well-formed face that gets triangulated (more than its three corners kept) passes _bake_ref.general_position:
    the exact and the fp64 predicates then agree, and exact_delaunay is the kernel's triangulation"""
    src_xyz = np.asarray(src_xyz, np.float64); vert_xyz = np.asarray(vert_xyz, np.float64)
    nv = vert_xyz.shape[1]
    for fv in np.asarray(faces).reshape(-1, 3):
        if any(v < 0 or v >= nv for v in fv):
            continue
        _, P, _, _ = B.face_points(src_xyz, index_colours(src_xyz.shape[1]), vert_xyz, vert_uv, np.zeros((nv, 3), np.int64), fv, nbr_idx)
        if len(P) > 3 and not B.general_position(P):
            return False
    return True
