"""The normal-map reference (tests/_bake_normal_ref.py) on closed forms -- no GPU: what the GPU suite (tests/test_gpu_bake_maps.py) is
held to must itself be right where the answer is known without it."""
from fractions import Fraction

import numpy as np
import pytest

import _bake_normal_ref as NR
import _bake_ref as B
from _bake_cases import UNIT, _interior

R = 64
UV = np.array([[0.1, 0.1], [0.9, 0.15], [0.2, 0.85]])
AXES = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
IRRATIONAL = [(1, 2, 3), (-3, 1, 2), (2, -5, 1), (1, 1, 1), (-1, -2, -2.5)]


def _face(n_interior, seed=1):
    rng = np.random.default_rng(seed)
    pts = _interior(rng, n_interior) if n_interior else np.zeros((1, 3)) + 5.0
    lists = np.full((3, 32), B.NOIDX, np.uint32)
    if n_interior:
        lists.ravel()[:n_interior] = np.arange(n_interior)
    return np.ascontiguousarray(pts.T), np.ascontiguousarray(UNIT.T), np.array([[0, 1, 2]], np.int32), lists


def _bake(src, src_nrm, verts, vert_nrm, faces, lists):
    return NR.bake(src, src_nrm, verts, UV, vert_nrm, faces, lists, R, B.exact_delaunay)


def _expected_byte(v):
    """encode() of a direction by hand, and how far each t + 0.5 is from the next integer (the room rounding errors have)"""
    v = np.asarray(v, np.float64)
    t = v / np.sqrt((v * v).sum()) * 127.5 + 127.5 + 0.5
    room = np.minimum(t - np.floor(t), np.ceil(t) - t)
    return np.array([int(t[2]), int(t[1]), int(t[0]), 255], np.uint8), room.min()


@pytest.mark.parametrize("n", AXES + IRRATIONAL)
def test_one_direction_everywhere(n):
    src, verts, faces, lists = _face(20)
    unit = np.asarray(n, np.float64) / np.linalg.norm(n)
    want, room = _expected_byte(n)
    # the mix of three equal unit vectors is the vector up to a few ulp; a byte can only flip if t + 0.5 is that close to an integer
    assert tuple(n) in AXES or room > 1e-9
    tex = _bake(src, np.tile(unit, (20, 1)), verts, np.tile(unit, (3, 1)), faces, lists)
    covered = tex[:, :, 3] == 255
    assert covered.sum() > 500 and np.array_equal(np.unique(tex[covered], axis=0), want[None, :])
    assert not tex[~covered].any()


def test_axis_encodings_are_exact():
    assert [tuple(NR.encode(np.float64(a))) for a in AXES] == [(128, 128, 255, 255), (128, 128, 0, 255), (128, 255, 128, 255), (128, 0, 128, 255),
                                                               (255, 128, 128, 255), (0, 128, 128, 255)]


def test_zero_and_non_finite_normals_point_up():
    src, verts, faces, lists = _face(12)
    tex = _bake(src, np.zeros((12, 3)), verts, np.zeros((3, 3)), faces, lists)
    covered = tex[:, :, 3] == 255
    assert covered.any() and (tex[covered][:, [2, 1, 0, 3]] == (128, 128, 255, 255)).all()        # R, G, B, A: straight up
    for bad in (np.nan, np.inf, 1e200):                       # NaN, infinite, and finite values whose squares overflow
        assert tuple(NR.encode(np.array([bad, 1.0, 0.0]))) == (255, 128, 128, 255)                 # B, G, R, A as stored


def test_endpoint_scale():
    src, verts, faces, lists = _face(15, seed=3)
    rng = np.random.default_rng(4)
    sn, vn = rng.standard_normal((15, 3)), rng.standard_normal((3, 3))
    base = _bake(src, sn, verts, vn, faces, lists)
    # a common factor scales m and l alike: u moves by an ulp or two, a byte only where t + 0.5 sits that close to an integer (none here)
    assert np.array_equal(_bake(src, 7.0 * sn, verts, 7.0 * vn, faces, lists), base)
    vn2 = vn.copy(); vn2[0] *= 7.0                            # one endpoint alone: its normal now outweighs the others
    assert (_bake(src, sn, verts, vn2, faces, lists) != base).any(axis=2).sum() > 20


def test_coverage_equals_the_colour_reference():
    src, verts, faces, lists = _face(40, seed=5)
    rng = np.random.default_rng(6)
    tex = _bake(src, rng.standard_normal((40, 3)), verts, rng.standard_normal((3, 3)), faces, lists)
    col = B.bake(src, rng.integers(0, 256, (40, 3)), verts, UV, rng.integers(0, 256, (3, 3)), faces, lists, R, B.exact_delaunay)
    assert np.array_equal(tex[:, :, 3], col[:, :, 3]) and (tex[:, :, 3] == 255).sum() > 500


def test_linear_field_against_exact_barycentrics():
    """no interior points, corner normals e_x, e_y, e_z: the mix IS the barycentric triple, here computed in exact rationals"""
    src, verts, faces, lists = _face(0)
    tex = _bake(src, np.zeros((1, 3)), verts, np.eye(3), faces, lists)
    P = [(Fraction(float(u)) * R, Fraction(float(v)) * R) for u, v in UV]
    A = (P[1][0] - P[0][0]) * (P[2][1] - P[0][1]) - (P[1][1] - P[0][1]) * (P[2][0] - P[0][0])
    checked = 0
    for i, j in [(20, 20), (30, 15), (15, 40), (40, 25), (12, 12), (25, 30), (50, 12), (18, 50)]:
        b0 = ((P[1][0] - i) * (P[2][1] - j) - (P[1][1] - j) * (P[2][0] - i)) / A
        b1 = ((P[2][0] - i) * (P[0][1] - j) - (P[2][1] - j) * (P[0][0] - i)) / A
        b2 = 1 - b0 - b1
        if min(b0, b1, b2) <= 0:
            assert tex[R - j, i, 3] == 0 or min(b0, b1, b2) > -1e-12
            continue
        b = np.array([float(b0), float(b1), float(b2)])
        want, room = _expected_byte(b)
        assert room > 1e-9                                    # (else pick another pixel: the byte would hang on the last ulp)
        assert np.array_equal(tex[R - j, i], want), (i, j)
        checked += 1
    assert checked >= 5
