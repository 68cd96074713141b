"""CPU: pins tests/_attr_ref.py -- the plain fp64 / longdouble reference of the attribute stage -- before the GPU suite
(tests/test_gpu_attr_reference.py) holds the kernels to it: against the oracle on the GPU suite's own inputs, against closed forms, and
against a numpy restatement of the kernel's one-pass shifted moment sums (the cancellation claim of pca_one in csrc/pt_attr.hip)."""
import numpy as np
import pytest

import _attr_cases as cases
import _attr_ref as R

NOIDX = R.NOIDX


def shifted_moments_normal(idx, xyz64):
    """pca_one's sums restated in numpy fp64, neighbour by neighbour in list order: moments about the FIRST valid neighbour, then
    cov = Sum(d d^T) - Sum(d) Sum(d)^T / ke, handed to eigh (not to a Jacobi sweep).  Returns the unoriented normal (m, 3)."""
    xyz64 = np.asarray(xyz64, np.float64)
    n = xyz64.shape[1]
    idx = np.asarray(idx, np.uint32)
    m, k = idx.shape
    pts = np.ascontiguousarray(xyz64.T)
    o = np.zeros((m, 3)); sd = np.zeros((m, 3)); cv = np.zeros((m, 3, 3)); ke = np.zeros(m, np.int64)
    for j in range(k):
        id_ = idx[:, j]
        ok = (id_ != NOIDX) & (id_ < n)
        p = pts[np.where(ok, id_, 0)]
        first = ok & (ke == 0)
        o[first] = p[first]
        d = np.where(ok[:, None], p - o, 0.0)
        sd += d
        cv += d[:, :, None] * d[:, None, :]
        ke += ok
    cv -= sd[:, :, None] * sd[:, None, :] / np.maximum(ke, 1)[:, None, None]
    return np.linalg.eigh(cv)[1][:, :, 0], ke


# ---- pca_ref against the oracle, on the inputs of the GPU suite ------------------------------------------------------------------
ORACLE_CASES = [(c, "f32", k) for c in ("surface", "volume") for k in cases.KS] + \
               [(c, "f16", k) for c in ("surface", "volume") for k in (3, 5, 16, 31, 32)] + \
               [(c, "f64", k) for c in ("surface", "volume") for k in (3, 8, 13, 32)] + [("far", "f64", 8), ("far", "f64", 20)]


@pytest.mark.parametrize("name,dtype,k", ORACLE_CASES, ids=["%s-%s-k%d" % c for c in ORACLE_CASES])
@pytest.mark.parametrize("normals", [True, False], ids=["nrm", "nonrm"])
def test_pca_ref_matches_oracle(oracle, name, dtype, k, normals):
    """The oracle (two-pass fp64 sums, cyclic Jacobi) within pca_bound of the reference (longdouble centring, LAPACK eigh) on every
    comparable row.  The share of comparable rows is a condition of the inputs: >= 0.99 (fp16 rounding makes a few collinear triples on
    the surface at k = 3)."""
    xyz, nrm = cases.cloud(name, dtype)
    x64 = xyz.astype(np.float64)
    idx, _ = cases.lists(name, dtype, k)
    got, _ = oracle.pca_normals(idx, x64, nrm if normals else None)
    R.check_pca(got, idx, x64, nrm if normals else None, "oracle %s %s" % (name, dtype))


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_pca_ref_matches_oracle_missing_entries(oracle, dtype):
    """the lists with NOIDX entries, ids >= n and 0..3 survivors: the oracle skips what the kernels skip, and rows with fewer than three
    neighbours are (0, 0, 1)"""
    xyz, nrm = cases.cloud("surface", dtype)
    x64 = xyz.astype(np.float64)
    idx = cases.knock_out(cases.lists("surface", dtype, 20)[0], x64.shape[1])
    got, _ = oracle.pca_normals(idx, x64, nrm)
    f = R.check_pca(got, idx, x64, nrm, "oracle knocked-out %s" % dtype, min_share=0.95)
    assert f["few"] >= 30


# ---- pca_ref against closed forms -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b,c", [(0.3, 0.1, 0.0), (-1.0, 0.75, -2.5), (5.0, -3.0, 0.125), (0.0, 0.0, 0.0)])
def test_pca_ref_plane(a, b, c):
    """points on z = a + b x + c y give (-b, -c, 1) / |.| (oriented +z without stored normals, and against a stored normal)"""
    rng = np.random.default_rng(1)
    p = rng.random((3, 400))
    p[2] = a + b * p[0] + c * p[1]
    idx = np.stack([rng.choice(400, 12, replace=False) for _ in range(64)]).astype(np.uint32)
    want = np.array([-b, -c, 1.0]) / np.sqrt(b * b + c * c + 1.0)
    got, lam, ke = R.pca_ref(idx, p)
    assert (ke == 12).all()
    # z is rounded to fp64 after the plane is evaluated: the points leave the plane by one ulp of |z|, eps |z| / spread as an angle
    assert np.abs(got - want).max() <= 1e-13
    down = np.tile(np.float32([0, 0, -1]), (400, 1))
    got, _, _ = R.pca_ref(idx, p, down)
    assert np.abs(got + want).max() <= 1e-13


@pytest.mark.parametrize("radius", [1.0, 10.0, 1e3])
def test_pca_ref_sphere(radius):
    """a patch of radius h around the pole of a sphere of radius R: the radial direction within O(h^2 / R^2).  The patch is sampled
    symmetrically (rings of 8), so that the tangential asymmetry terms of odd order vanish and the bound is the curvature term alone."""
    h = 0.05 * radius
    pole = np.array([0.3, -0.5, 0.8]); pole /= np.linalg.norm(pole)
    e1 = np.cross(pole, [0, 0, 1.0]); e1 /= np.linalg.norm(e1)
    e2 = np.cross(pole, e1)
    pts = []
    for r in (0.35, 0.7, 1.0):
        for q in range(8):
            t = h * r * (np.cos(2 * np.pi * q / 8) * e1 + np.sin(2 * np.pi * q / 8) * e2)
            v = radius * pole + t
            pts.append(v / np.linalg.norm(v) * radius)
    p = np.array(pts).T + np.array([[2.0], [3.0], [-1.0]]) * radius
    idx = np.arange(24, dtype=np.uint32)[None, :]
    outward = np.tile(pole.astype(np.float32), (24, 1))
    got, lam, ke = R.pca_ref(idx, p, outward)
    err = np.linalg.norm(np.cross(got[0], pole))
    print("sphere R=%g: sin(angle to the radial direction) %.3g, (h/R)^2 = %.3g" % (radius, err, (h / radius) ** 2))
    assert err <= (h / radius) ** 2 and got[0] @ pole > 0
    # an asymmetric patch tilts the fitted plane at first order in h / R times the asymmetry; still O(h / R)^2 for a mild one
    got2, _, _ = R.pca_ref(idx[:, :20], p, outward)
    assert np.linalg.norm(np.cross(got2[0], pole)) <= 4 * (h / radius) ** 2


def test_pca_ref_few_neighbours_and_bound():
    p = np.random.default_rng(2).random((3, 10))
    idx = np.array([[0, 1, NOIDX, NOIDX], [NOIDX] * 4, [0, 1, 10, 0xFFFFFFFE], [0, 1, 2, NOIDX], [3, 4, 5, 6]], np.uint32)
    got, lam, ke = R.pca_ref(idx, p)
    assert ke.tolist() == [2, 0, 2, 3, 4]
    assert np.array_equal(got[:3], np.tile([0.0, 0.0, 1.0], (3, 1)))
    assert np.abs(np.linalg.norm(got, axis=1) - 1).max() < 1e-15 and (got[3:, 2] >= 0).all()
    # the bound: 2 (k+2)^2 eps trace / gap + 2^-22; infinite without a gap
    assert R.pca_bound(16, np.array([1.0, 2.0, 3.0])) == pytest.approx(2 * 18 ** 2 * 2.0 ** -52 * 6.0 + 2.0 ** -22, rel=1e-15)
    assert np.isinf(R.pca_bound(16, np.array([[1.0, 1.0, 3.0]]))).all()


# ---- blend_ref against the oracle ----------------------------------------------------------------------------------------------
def _within_before_store(got32, ref64, tol):
    """`got32` is the fp32 store of a value within tol of ref64: rounding is monotonic, so it lies between the stores of the two ends"""
    lo = (ref64 - tol).astype(np.float32); hi = (ref64 + tol).astype(np.float32)
    return (got32 >= lo) & (got32 <= hi)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 3, 5, 8, 13, 20, 31, 32])
def test_blend_ref_matches_oracle(oracle, k, mode):
    """oracle.blend (fp64 sums, stored to fp32) against blend_ref (longdouble) within 1e-12 of the value before the store, relative to
    the full scale of the output (255 for colours; 1 for normals, which are unit vectors or -- below the 1e-12 length -- shorter).
    fp64 sums of k <= 32 terms err by k 2^-53 ~ 4e-15 of that scale, so 1e-12 holds with two orders to spare."""
    idx, d2, rgb, nrm = cases.blend_case(k)
    gc, gn = oracle.blend(idx, d2, rgb, nrm, mode)
    rc, rn = R.blend_ref(idx, d2, rgb, nrm, mode)
    assert _within_before_store(gc, rc, 255e-12).all()
    assert _within_before_store(gn, rn, 1e-12).all()
    empty = ~((idx != NOIDX) & (idx < len(rgb))).any(axis=1)
    assert empty.any() and not gc[empty].any() and not gn[empty].any() and not rc[empty].any() and not rn[empty].any()


# ---- the kernel's one-pass shifted sums, without a GPU -------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0.0, 1e3, 1e6])
@pytest.mark.parametrize("name,k", [("surface", 3), ("surface", 16), ("surface", 32), ("volume", 5), ("volume", 20)])
def test_shifted_one_pass_moments_do_not_cancel(name, k, offset):
    """pca_one forms moments about the first neighbour in one pass and subtracts Sum(d) Sum(d)^T / ke.  Restated in numpy fp64 and fed
    to eigh, that agrees with the longdouble two-pass reference within the Davis-Kahan term of pca_bound wherever the cloud lies: the
    shift point is a neighbour, so the sums hold no term larger than (k + 1) trace."""
    xyz, _ = cases.cloud(name, "f32")
    x64 = xyz.astype(np.float64) + offset * np.array([[1.0], [-2.0], [3.0]])
    idx, _ = cases.lists(name, "f32", k)          # the same neighbourhoods at every offset
    got, ke = shifted_moments_normal(idx, x64)
    want, lam, ke_ref = R.pca_ref(idx, x64)
    assert np.array_equal(ke, ke_ref)
    cmp_ = R.comparable(lam)
    assert cmp_.mean() >= 0.99
    s = R.sin_angle(got, want)[cmp_]
    cond = (lam.sum(axis=1) / (lam[:, 1] - lam[:, 0]))[cmp_]
    print("%s k=%d offset %g: max sin / (eps trace / gap) = %.3g" % (name, k, offset, (s / (R.EPS64 * cond)).max()))
    assert (s <= R.pca_bound(k, lam)[cmp_] - 2.0 ** -22).all()


def test_shifted_one_pass_moments_missing_entries():
    xyz, _ = cases.cloud("surface", "f64")
    idx = cases.knock_out(cases.lists("surface", "f64", 20)[0], xyz.shape[1])
    got, ke = shifted_moments_normal(idx, xyz)
    want, lam, ke_ref = R.pca_ref(idx, xyz)
    assert np.array_equal(ke, ke_ref)
    cmp_ = R.comparable(lam) & (ke >= 3)
    assert (R.sin_angle(got, want)[cmp_] <= R.pca_bound(20, lam)[cmp_] - 2.0 ** -22).all()
