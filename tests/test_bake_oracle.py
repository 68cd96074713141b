"""CPU checks of the texture-bake oracle (oracle/pt_oracle.c: pto_bake_texture, pto_dilate_pad) -- the build's definition of
the reference's per-face bake (src/pointsTransfer.cpp:462-581, :66-107) and edge padding (:593-611) -- against independent
restatements: a numpy rasteriser for the no-neighbour case, scipy.ndimage for the dilation, and, on the rows of
_bake_cases.make_face_cases(), tests/_bake_ref.py -- DESIGN.md section 8 restated in numpy:
  * rows in general position (every in-circle determinant verified non-zero and of the fp64 sign in exact arithmetic, no face left
    out): the oracle's triangle SET equals scipy.spatial.Delaunay's, the areas add up to the face's, the count is 2 np - 2 - hull;
  * lattice rows (co-circular, collinear, coincident points): the oracle's triangle LIST equals exhaustive empty-circle with exact
    integer predicates, entry for entry, including which triples the 255 cap drops;
  * every row: the whole atlas of _bake_ref.bake equals the oracle's byte for byte, and the row's reach holds on the face report;
  * a triangle far outside the int range in UV returns at once (child process under a time limit)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _bake_ref as B
from _bake_cases import ROW_NAMES, cloud_as, face_reports, make_case, make_face_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = {r["name"]: r for r in make_face_cases()}


def _numpy_draw(tex, U, V, col, R):
    """reference draw_triangle (:66-107) in numpy, same operation order as the oracle"""
    p = np.array([U[0] * R, V[0] * R]); q = np.array([U[1] * R, V[1] * R]); r = np.array([U[2] * R, V[2] * R])
    A = (q[0] - p[0]) * (r[1] - p[1]) - (q[1] - p[1]) * (r[0] - p[0])
    if A == 0:
        return
    i0 = max(int(np.floor(min(p[0], q[0], r[0]))), 0); i1 = min(int(np.floor(max(p[0], q[0], r[0]))), R - 1)
    j0 = max(int(np.floor(min(p[1], q[1], r[1]))), 1); j1 = min(int(np.floor(max(p[1], q[1], r[1]))), R)
    for i in range(i0, i1 + 1):
        for j in range(j0, j1 + 1):
            x, y = float(min(i, R - 1)), float(min(j, R - 1))
            b0 = ((q[0] - x) * (r[1] - y) - (q[1] - y) * (r[0] - x)) / A
            b1 = ((r[0] - x) * (p[1] - y) - (r[1] - y) * (p[0] - x)) / A
            b2 = (1.0 - b0) - b1
            if b0 >= 0 and b1 >= 0 and b2 >= 0:
                for c in range(3):
                    f = np.float32((b0 * float(col[0][c]) + b1 * float(col[1][c])) + b2 * float(col[2][c]))
                    tex[R - j, i, 2 - c] = np.uint8(min(max(f, np.float32(0)), np.float32(255)))
                tex[R - j, i, 3] = 255


def test_bake_without_neighbours_is_the_plain_rasteriser(oracle):
    src, rgb, verts, uv, vrgb, faces = make_case(3, n=50, grid=3)
    R = 96
    none = np.full((verts.shape[1], 4), 0xFFFFFFFF, np.uint32)
    got = oracle.bake_texture(src, rgb, verts, uv, vrgb, faces, none, R)
    want = np.zeros((R, R, 4), np.uint8)
    for f in faces:
        _numpy_draw(want, uv[f, 0], uv[f, 1], vrgb[f], R)
    assert np.array_equal(got, want)


def test_bake_covers_the_face_and_uses_cloud_colours(oracle):
    """With neighbours, the sub-triangles tile each face: whatever the plain face rasterisation covers stays covered, except
    pixel centres that sit exactly on an edge (barycentric rounding, as in the reference) -- and the colours now come from the cloud."""
    src, rgb, verts, uv, vrgb, faces = make_case(4, n=4000, grid=4)
    uv = uv * np.array([0.987, 0.981]) + np.array([0.0031, 0.0057])      # keep mesh edges (the diagonals too) off the pixel centres
    R = 256
    idx, _ = oracle.knn_bruteforce(src, verts, 20)
    none = np.full_like(idx, 0xFFFFFFFF)
    plain = oracle.bake_texture(src, rgb, verts, uv, vrgb, faces, none, R)
    baked = oracle.bake_texture(src, rgb, verts, uv, vrgb, faces, idx, R)
    lost = (plain[:, :, 3] == 255) & (baked[:, :, 3] != 255)
    assert (plain[:, :, 3] == 255).sum() > 40000 and lost.sum() <= 4
    assert (baked[:, :, 3] == 255).sum() <= (plain[:, :, 3] == 255).sum()          # interior points never reach outside their face
    assert (baked[:, :, :3] != plain[:, :, :3]).any(axis=2).mean() > 0.3
    # idempotent and order-defined: baking twice gives the same bytes
    assert np.array_equal(baked, oracle.bake_texture(src, rgb, verts, uv, vrgb, faces, idx, R))


def test_bake_degenerate_inputs(oracle):
    """duplicate cloud points, cloud points exactly on mesh vertices, zero-area faces, out-of-range indices, UVs outside [0, 1]"""
    src, rgb, verts, uv, vrgb, faces = make_case(5, n=3000, grid=3, degenerate=True)
    idx, _ = oracle.knn_bruteforce(src, verts, 20)
    idx[3, :5] = 0xFFFFFFFF
    uv2 = uv * 1.3 - 0.15                          # part of the atlas outside the texture: those pixels are skipped
    faces = np.vstack([faces, [[0, 1, 9999]]]).astype(np.int32)      # malformed face: skipped
    tex = oracle.bake_texture(src, rgb, verts, uv2, vrgb, faces, idx, 128)
    assert tex.shape == (128, 128, 4) and set(np.unique(tex[:, :, 3])) <= {0, 255}
    assert (tex[:, :, 3] == 255).mean() > 0.5


def test_dilate_pad_against_scipy(oracle):
    from scipy import ndimage
    rng = np.random.default_rng(6)
    R = 97
    tex = np.zeros((R, R, 4), np.uint8)
    m = rng.random((R, R)) < 0.02
    tex[m, :3] = rng.integers(0, 256, size=(int(m.sum()), 3), dtype=np.uint8)
    tex[m, 3] = 255
    tex[5, 5] = (10, 20, 30, 128)                   # a partly transparent pixel: the mask is bitwise, the add saturates
    for ks in (1, 3, 25):
        got = oracle.dilate_pad(tex, ks)
        dil = np.stack([ndimage.maximum_filter(tex[:, :, c], size=ks, mode="constant", cval=0) for c in range(4)], axis=2)
        mask = (~tex[:, :, 3])[:, :, None]
        want = np.minimum(tex.astype(np.int32) + (dil & mask).astype(np.int32), 255).astype(np.uint8)
        assert np.array_equal(got, want), ks


# ---- the rows of _bake_cases.make_face_cases(): reach, triangulation against scipy / exact predicates, whole atlas against _bake_ref ----
def test_vector_rasteriser_equals_the_scalar_one():
    """_bake_ref.draw is _numpy_draw over the bounding box at once: same bytes, triangles partly and wholly outside included"""
    rng = np.random.default_rng(70)
    for R in (1, 7, 40):
        a = np.zeros((R, R, 4), np.uint8); b = np.zeros((R, R, 4), np.uint8)
        for _ in range(12):
            U = rng.random(3) * 1.6 - 0.3; V = rng.random(3) * 1.6 - 0.3
            col = rng.integers(0, 256, size=(3, 3))
            _numpy_draw(a, U, V, col, R); B.draw(b, U, V, col, R)
        assert np.array_equal(a, b) and (R < 40 or (a[:, :, 3] == 255).any())


def _oracle_atlas(oracle, row, src, R):
    return oracle.bake_texture(src, row["rgb"], row["verts"], row["uv"], np.clip(row["vrgb"], 0, 255).astype(np.uint8), row["faces"], row["lists"], R)


@pytest.mark.parametrize("name", ROW_NAMES)
def test_face_row_reach_triangulation_and_atlas(oracle, name):
    row = ROWS[name]
    skipped = 0
    for ctype in row["types"]:
        src = cloud_as(row, ctype)
        reps = face_reports(oracle, row, ctype)
        row["reach"](reps)
        for f, r in enumerate(reps):
            if not r["valid"] or r["np"] == 3:
                assert r["ntri_all"] == 0
                continue
            P, T = r["xy"], r["tris"]
            if row["tri"] == "scipy":
                if not B.general_position(P):
                    skipped += 1
                    continue
                want = B.scipy_delaunay(P)
                assert r["ntri_all"] == len(T) == 2 * r["np"] - 2 - B.hull_size(P), (name, ctype, f)
                assert set(map(tuple, T)) == set(map(tuple, want)), (name, ctype, f)
                face2 = abs((P[1, 0] - P[0, 0]) * (P[2, 1] - P[0, 1]) - (P[1, 1] - P[0, 1]) * (P[2, 0] - P[0, 0]))
                assert abs(B.tri_area2(P, T) - face2) <= 1e-12 * face2, (name, ctype, f)
                assert np.array_equal(T, want)                       # and the oracle's order is the lexicographic one
            else:
                want = B.exact_delaunay(P)
                assert r["ntri_all"] == len(want), (name, ctype, f, r["ntri_all"], len(want))
                assert np.array_equal(T, want[:B.MAXTRI]), (name, ctype, f)
        tri = B.scipy_delaunay if row["tri"] == "scipy" else B.exact_delaunay
        for R in row["R"]:
            got = _oracle_atlas(oracle, row, src, R)
            want = B.bake(src, row["rgb"], row["verts"], row["uv"], row["vrgb"], row["faces"], row["lists"], R, tri)
            assert np.array_equal(got, want), "%s %s R=%d: %d pixels differ" % (name, ctype, R, (got != want).any(axis=2).sum())
    assert skipped == 0, "%s: %d faces are not in verified general position" % (name, skipped)


def test_triangle_far_outside_the_int_range_returns():
    """all three U R >= 2**31: the bounding box is rejected in double before any cast (it used to make the column loop run 2**31 times)"""
    code = ("import numpy as np\nfrom oracle import oracle\n"
            "verts = np.array([[0, 1, 0], [0, 0, 1], [0, 0, 0]], float)\n"
            "none = np.full((3, 4), 0xFFFFFFFF, np.uint32)\n"
            "for uv in ([[1e10, 0.1], [1e10 + 1, 0.2], [1e10, 0.9]], [[0.1, -1e10], [0.2, -1e10 - 1], [0.9, -1e10]], [[4e7, 4e7], [4e7 + 1, 4e7], [4e7, 4e7 + 1]]):\n"
            "    tex = oracle.bake_texture(np.zeros((3, 4)), np.zeros((4, 3), np.uint8), verts, np.array(uv), np.full((3, 3), 200, np.uint8), np.array([[0, 1, 2]], np.int32), none, 64)\n"
            "    assert not tex.any()\n"
            "print('returned')\n")
    try:
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=60)
    except subprocess.TimeoutExpired:
        pytest.fail("pto_draw_triangle did not return within 60 s on a triangle beyond the int range")
    assert r.returncode == 0 and "returned" in r.stdout, r.stderr
