"""The height-map reference (tests/_bake_height_ref.py) held to closed forms: what the GPU suite compares pt_bake_maps_h against must
itself be right.  No GPU."""
from fractions import Fraction

import numpy as np

import _bake_height_ref as HR
import _bake_ref as B
from _bake_cases import LATTICE, UNIT, _Mesh, _interior, _lattice_xyz, make_face_cases

ROWS = {r["name"]: r for r in make_face_cases()}
UV_UNIT = np.array([[0.125, 0.125], [0.875, 0.125], [0.125, 0.875]])       # U = 0.125 + 0.75 x, V = 0.125 + 0.75 y: dyadic, exact


def one_face(points, k=32, corners=UNIT, uv=UV_UNIT, order=(0, 1, 2)):
    m = _Mesh(k, 1)
    m.face(corners, m.cloud(points), uv=uv, order=order)
    return m.row("t", (64,), ("f64",), "exact", None)


def bake(row, R, H, mix=None):
    return HR.bake(row["src"], row["verts"], row["uv"], row["faces"], row["lists"], R, H, B.exact_delaunay, mix)


def grey(tex):
    """the height bytes of the covered pixels; checks the pixel layout on the way"""
    cov = tex[:, :, 3] == 255
    assert not tex[~cov].any() and (tex[cov][:, 0] == tex[cov][:, 1]).all() and (tex[cov][:, 0] == tex[cov][:, 2]).all()
    return tex[cov][:, 0]


def test_encoding_end_points():
    got = HR.encode(np.array([0.0, -0.0, 2.0, -2.0, 1.0, -1.0, 5.0, -5.0, np.inf, -np.inf, np.nan]), 2.0)[:, 0]
    assert got.tolist() == [128, 128, 255, 0, 191, 64, 255, 0, 128, 128, 128]          # 127.5 * 0.5 + 128 = 191.75; 127.5 * -0.5 + 128 = 64.25


def test_cloud_in_the_face_plane_is_128():
    row = one_face(_lattice_xyz(LATTICE[:40]))
    tex, top = bake(row, 64, 0.37)
    g = grey(tex)
    assert len(g) > 500 and (g == 128).all() and top == 0.0


def test_one_interior_point_is_a_tent():
    """one point at height h0 over barycentrics p of the face: the mix at a pixel with face barycentrics l is h0 min(l_i / p_i), whichever
    of the three sub-triangles drew it.  Exact rationals; a pixel off the face's edges is compared unless its exact u + 0.5 lies within 1e-9 of an integer."""
    h0, H, R = 0.3, 0.4, 64
    row = one_face(np.array([[0.25, 0.5, h0]]))
    tex, top = bake(row, R, H)
    assert top == h0
    rows, cols = np.nonzero(tex[:, :, 3])
    p = (Fraction(1, 4), Fraction(1, 4), Fraction(1, 2))                       # of the point (0.25, 0.5): l0 = 1 - x - y, l1 = x, l2 = y
    checked = 0
    for r, c in zip(rows, cols):
        x = (Fraction(int(c), R) - Fraction(1, 8)) / Fraction(3, 4); y = (Fraction(int(R - r), R) - Fraction(1, 8)) / Fraction(3, 4)
        l = (1 - x - y, x, y)
        assert min(l) >= 0
        m = Fraction(h0) * min(l[i] / p[i] for i in range(3))
        u = m / Fraction(H) * Fraction(255, 2) + 128
        if m == 0:                                                           # a face edge: a mix of a few ulps is absorbed by 127.5 + .
            assert tex[r, c, 0] == 128, (r, c)
        elif abs(u - round(u)) < Fraction(1, 10 ** 9):
            continue
        else:
            assert int(tex[r, c, 0]) == min(max(int(u), 0), 255), (r, c)
        checked += 1
    assert checked > 0.95 * len(rows) and len(rows) > 1000
    assert tex[:, :, 0].max() > 215                                          # the apex: 0.75 * 127.5 + 128 = 223.6


def test_scaling_by_two_leaves_the_bytes():
    rng = np.random.default_rng(3)
    corners = UNIT @ np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]]).T + np.array([3.0, -2.0, 5.0])
    pts = _interior(rng, 14, corners, lift=0.2)
    a = one_face(pts, corners=corners); b = one_face(2.0 * pts, corners=2.0 * corners)
    ta, ma = bake(a, 96, 0.25); tb, mb = bake(b, 96, 0.5)
    assert np.array_equal(ta, tb) and mb == 2.0 * ma and ma > 0
    assert len(np.unique(grey(ta))) > 20


def test_reversed_winding_negates_every_height():
    rng = np.random.default_rng(4)
    corners = UNIT @ np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]]).T
    pts = _interior(rng, 20, corners, lift=0.3, margin=0.05)
    fwd = one_face(pts, corners=corners); rev = one_face(pts, corners=corners, order=(0, 2, 1))
    hf = HR.face_heights(fwd["src"], fwd["verts"], fwd["uv"], fwd["faces"][0], fwd["lists"])
    hr = HR.face_heights(rev["src"], rev["verts"], rev["uv"], rev["faces"][0], rev["lists"])
    assert len(hf[2]) == 23 and np.array_equal(hf[3], hr[3])
    assert np.array_equal(hr[2], -hf[2]) and (hf[2][3:] > 0).any() and (hf[2][3:] < 0).any()
    # the sign: the face's winding faces +z for UNIT in order (0, 1, 2)
    up = one_face(np.array([[0.25, 0.25, 0.5]]))
    assert HR.face_heights(up["src"], up["verts"], up["uv"], up["faces"][0], up["lists"])[2][3] == 0.5


def test_small_range_saturates():
    rng = np.random.default_rng(5)
    pts = _interior(rng, 16, lift=0.5)
    row = one_face(pts)
    R, H = 96, 1e-6
    mix = np.zeros((R, R))
    tex, top = bake(row, R, H, mix)
    cov = tex[:, :, 3] == 255
    g = tex[:, :, 0]
    assert top > 0.1
    assert (g[cov & (mix >= H)] == 255).all() and (g[cov & (mix <= -H)] == 0).all()
    assert (cov & (mix >= H)).sum() > 100 and (cov & (mix <= -H)).sum() > 100
    between = cov & (np.abs(mix) < H)
    assert set(np.unique(g[cov & ~between]).tolist()) == {0, 255} and between.sum() < 0.1 * cov.sum()


def test_degenerate_frames_have_height_zero():
    row = ROWS["verts_bad"]
    for f in range(1, 7):
        P, UV, h, ids = HR.face_heights(row["src"], row["verts"], row["uv"], row["faces"][f], row["lists"])
        assert len(P) == 3 and not h.any() and len(ids) == 0
    tex, top = HR.bake(row["src"], row["verts"], row["uv"], row["faces"][1:7], row["lists"], 128, 0.01, B.scipy_delaunay)
    assert (grey(tex) == 128).all() and top == 0.0
    tex, top = HR.bake(row["src"], row["verts"], row["uv"], row["faces"], row["lists"], 128, 0.01, B.scipy_delaunay)
    assert top > 0 and len(np.unique(grey(tex))) > 3


def test_coverage_is_the_colour_reference_s():
    for name in ("mirrored_uv", "sliver", "stacked", "uv_edge", "uv_bad"):
        row = ROWS[name]
        R = row["R"][0]
        tri = B.scipy_delaunay if row["tri"] == "scipy" else B.exact_delaunay
        tex, _ = HR.bake(row["src"], row["verts"], row["uv"], row["faces"], row["lists"], R, 0.05, tri)
        col = B.bake(row["src"], row["rgb"], row["verts"], row["uv"], np.clip(row["vrgb"], 0, 255), row["faces"], row["lists"], R, tri)
        assert np.array_equal(tex[:, :, 3], col[:, :, 3]) and (tex[:, :, 3] == 255).any()
