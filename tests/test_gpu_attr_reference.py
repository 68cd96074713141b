"""GPU suite of the attribute stage (csrc/pt_attr.hip: pca_pa_kernel, pca_kernel<double>, blend_kernel, blend_keep_kernel) against the
plain fp64 / longdouble reference of tests/_attr_ref.py, which tests/test_attr_ref.py pins on the CPU.

Neighbour lists are the oracle's brute force or hand-built, so no search kernel stands between a test and the attribute kernels.
PCA bar: every row finite and of unit length within 1e-6; rows with fewer than three neighbours exactly (0, 0, 1); every row with
l1 - l0 > 1e-6 trace within pca_bound (derived in _attr_ref.py) of the reference and in its half-space.
Blend bar: the project's 1e-5 (colour / 255, normal components)."""
import numpy as np
import pytest

import _attr_cases as cases
import _attr_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-5
NOIDX = R.NOIDX


@pytest.fixture(scope="module")
def pt(pkg):
    p = pkg.PointsTransfer(device=0)
    yield p
    p.close()


@pytest.fixture(scope="module")
def pt_capped(pkg):
    p = pkg.PointsTransfer(device=0, max_dist=1e3)          # blends take the lists they are given: the cap only selects the keep-empty kernels
    yield p
    p.close()


def _build(p, xyz, nrm):
    """stored normals or no attribute table at all (the has_attr == 0 branch of the kernels)"""
    p.build(xyz, None, nrm)


# ---- the PCA matrix -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normals", [True, False], ids=["nrm", "nonrm"])
@pytest.mark.parametrize("k", cases.KS)
@pytest.mark.parametrize("dtype", ["f32", "f64", "f16"])
@pytest.mark.parametrize("name", ["surface", "volume"])
def test_pca_matrix(pt, name, dtype, k, normals):
    """fp32 and fp16 clouds run pca_pa_kernel over the packed table, fp64 clouds pca_kernel<double>; k = 1, 2 end in the ke < 3 branch,
    k not a multiple of four in the tail guard of the four-at-a-time gather, k = 32 is PT_MAX_K.  The share of comparable rows
    (>= 0.99) is a condition on the inputs, checked on the CPU for these clouds (tests/test_attr_ref.py)."""
    xyz, nrm = cases.cloud(name, dtype)
    nrm = nrm if normals else None
    _build(pt, xyz, nrm)
    idx, _ = cases.lists(name, dtype, k)
    got = pt.pca_normals(idx)
    R.check_pca(got, idx, xyz.astype(np.float64), nrm, "%s %s" % (name, dtype))


@pytest.mark.parametrize("k", [8, 20])
def test_pca_f64_far_from_origin(pt, k):
    """the surface scaled by 1e-3 at (1e6, -2e6, 3e6): neighbour offsets of 1e-5 on coordinates of 1e6.  The reference reads the same
    fp64 values, so the offset costs it nothing; a kernel that centred in fp32, or summed unshifted moments, is off by far more than
    the bound"""
    xyz, nrm = cases.cloud("far", "f64")
    _build(pt, xyz, nrm)
    idx, _ = cases.lists("far", "f64", k)
    R.check_pca(pt.pca_normals(idx), idx, xyz, nrm, "far f64")


def test_pca_dev_matches_host_entry(pt):
    """pt_pca_normals_dev on device buffers: the same answer as the host entry point, bit for bit, and within the bound"""
    import torch
    xyz, nrm = cases.cloud("surface", "f32")
    _build(pt, xyz, nrm)
    idx, _ = cases.lists("surface", "f32", 13)
    host = pt.pca_normals(idx)
    di = torch.from_numpy(idx.view(np.int32)).cuda()
    out = torch.full((idx.shape[0], 3), float("nan"), device="cuda", dtype=torch.float32)
    pt.pca_normals_dev(di, idx.shape[0], 13, out)
    pt.synchronize(); torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), host.view(np.uint32))
    R.check_pca(got, idx, xyz.astype(np.float64), nrm, "dev entry")


# ---- missing entries --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normals", [True, False], ids=["nrm", "nonrm"])
@pytest.mark.parametrize("dtype", ["f32", "f64", "f16"])
def test_pca_missing_entries(pt, dtype, normals):
    """An exact k = 20 list with NOIDX entries at random, ids n and 0xFFFFFFFE (both read record 0 and are skipped), rows of exactly
    0, 1, 2 and 3 survivors, and rows whose first valid neighbour -- the origin of the shifted sums -- is not the first of its group of
    four.  Rows below three neighbours are exactly (0, 0, 1).  Three-point rows are mostly near-collinear on no one's account, hence
    the lower share."""
    xyz, nrm = cases.cloud("surface", dtype)
    nrm = nrm if normals else None
    _build(pt, xyz, nrm)
    idx = cases.knock_out(cases.lists("surface", dtype, 20)[0], xyz.shape[1])
    valid = (idx != NOIDX) & (idx < xyz.shape[1])
    assert all((valid.sum(axis=1) == s).sum() >= 10 for s in (0, 1, 2, 3))
    assert (idx == xyz.shape[1]).any() and (idx == 0xFFFFFFFE).any()
    assert (~valid[40:140, 0]).sum() >= 60 and valid[100:120, 3].all()
    f = R.check_pca(pt.pca_normals(idx), idx, xyz.astype(np.float64), nrm, "knocked-out %s" % dtype, min_share=0.95)
    assert f["few"] >= 30


# ---- a context with a max_dist cap -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_pca_capped_context(pkg, dtype):
    """Lists as a capped query returns them (short and empty rows): PCA equals the reference on those very lists.  include/pt_api.h:
    a row with fewer than three neighbours -- an empty one included -- gets (0, 0, 1) under a cap as without one (unlike the capped
    blends, which leave empty rows unwritten)."""
    xyz, nrm = cases.cloud("surface", dtype)
    tgt = np.array(xyz[:, :cases.M], copy=True)
    lift = np.linspace(0.0, 0.03, cases.M).astype(xyz.dtype)
    tgt[2] += lift                                            # targets leave the surface: from full lists to none within reach
    r = 0.012
    with pkg.PointsTransfer(device=0, max_dist=r) as p:
        _build(p, xyz, nrm)
        idx, d2 = p.query(tgt, 16)
        cnt = (idx != NOIDX).sum(axis=1)
        assert (cnt == 16).sum() > 50 and (cnt == 0).sum() > 50 and ((cnt > 0) & (cnt < 3)).sum() > 5 and ((cnt >= 3) & (cnt < 16)).sum() > 50, np.bincount(cnt, minlength=17)
        assert (d2[idx != NOIDX] <= r * r).all()
        got = np.full((cases.M, 3), np.nan, np.float32)
        got[:] = p.pca_normals(idx)
    f = R.check_pca(got, idx, xyz.astype(np.float64), nrm, "capped %s" % dtype, min_share=0.95)
    assert np.array_equal(got[cnt == 0], np.tile(np.float32([0, 0, 1]), (int((cnt == 0).sum()), 1)))


# ---- degenerate neighbourhoods ---------------------------------------------------------------------------------------------------
def _degenerate_cloud():
    """Hand-built, every coordinate a small multiple of 2^-5 (exact in fp16, fp32 and fp64).  Returns (xyz (3, n) float64, dict of
    id ranges)."""
    parts, where = [], {}

    def add(name, pts):
        start = sum(len(q) for q in parts)
        parts.append(np.asarray(pts, np.float64))
        where[name] = np.arange(start, start + len(pts), dtype=np.uint32)

    s = 2.0 ** -5
    add("same", np.tile([[3 * s, 5 * s, 7 * s]], (32, 1)))
    add("line", np.array([[8, 8, 8]]) * s + np.arange(-16, 16)[:, None] * np.array([[1, 2, -1]]) * s)
    g = np.array([(i, j) for i in range(6) for j in range(6)][:32], np.float64)
    add("plane_z", np.stack([g[:, 0] * s, g[:, 1] * s, np.full(32, 9 * s)], axis=1))
    add("plane_111", np.stack([g[:, 0] * s, g[:, 1] * s, (20 - g[:, 0] - g[:, 1]) * s], axis=1))
    add("triangle", np.eye(3))
    return np.ascontiguousarray(np.concatenate(parts).T), where


@pytest.mark.parametrize("k", [3, 5, 8, 13, 32])
@pytest.mark.parametrize("dtype", ["f32", "f64", "f16"])
def test_pca_degenerate_rows(pt, dtype, k):
    """k copies of one point (zero covariance), k points on a line (two zero eigenvalues), k lattice points on the planes z = c and
    x + y + z = c (l0 zero or one ulp), an equilateral triangle.  Planes and triangle: within the bound.  Line and identical points:
    finite and of unit length; the line's answer perpendicular to the line within the bound taken with the gap l2 - l1."""
    x64, where = _degenerate_cloud()
    xyz = x64.astype(cases.DTYPES[dtype])
    assert np.array_equal(xyz.astype(np.float64), x64)
    _build(pt, xyz, None)
    rng = np.random.default_rng(k)
    rows, kind = [], []
    for name in ("same", "line", "plane_z", "plane_111"):
        for _ in range(8):
            rows.append(rng.choice(where[name], k, replace=False)); kind.append(name)
    rows.append(np.concatenate([where["triangle"], np.full(k - 3, NOIDX, np.uint32)])); kind.append("triangle")
    rows.append(np.full(k, where["same"][0], np.uint32)); kind.append("same")            # one id, k times
    idx = np.array(rows, np.uint32)
    kind = np.array(kind)
    got = pt.pca_normals(idx).astype(np.float64)
    assert np.isfinite(got).all() and np.abs(np.linalg.norm(got, axis=1) - 1).max() <= 1e-6
    want, lam, ke = R.pca_ref(idx, x64)
    flat = np.isin(kind, ["plane_z", "plane_111", "triangle"])
    assert R.comparable(lam)[flat].all()
    s = R.sin_angle(got, want)
    assert (s[flat] <= R.pca_bound(k, lam)[flat]).all(), (s[flat] / R.pca_bound(k, lam)[flat]).max()
    assert ((got * want).sum(axis=1)[flat] > 0).all()
    assert np.abs(np.abs(got[kind == "plane_z"]) - [0, 0, 1]).max() <= 2.0 ** -22
    assert np.abs(got[kind == "plane_111"] - 1 / np.sqrt(3)).max() <= 2 * R.pca_bound(k, lam)[kind == "plane_111"].max()
    line = kind == "line"
    along = np.array([1.0, 2.0, -1.0]) / np.sqrt(6.0)
    top_gap = lam[line, 2] - lam[line, 1]
    bound = 2.0 * (k + 2) ** 2 * R.EPS64 * lam[line].sum(axis=1) / top_gap + 2.0 ** -22
    assert (np.abs(got[line] @ along) <= bound).all(), np.abs(got[line] @ along).max()


# ---- the sign boundary -----------------------------------------------------------------------------------------------------------
def test_pca_sign_boundary(pt):
    """ref == 0: stored normals that sum to exactly zero over the neighbours (pairs of +-v), and -- without stored normals -- a plane
    that holds the z axis direction (n_z = 0).  Either orientation of the reference normal is right; the line must be within the
    bound.  With a sum of +-1e-3 n the orientation is decided and must follow it."""
    rng = np.random.default_rng(9)
    n = 4096
    p = rng.random((3, n)).astype(np.float32)
    p[2] = (0.2 + 0.5 * p[0] - 0.25 * p[1]).astype(np.float32)
    plane_n = np.array([-0.5, 0.25, 1.0]) / np.linalg.norm([-0.5, 0.25, 1.0])
    idx = np.stack([rng.choice(n, 8, replace=False) for _ in range(256)]).astype(np.uint32)
    for dtype in (np.float32, np.float64):
        xyz = p.astype(dtype)
        x64 = xyz.astype(np.float64)
        # every row: slots (0,1), (2,3), (4,5) carry +-v; slot 6 carries `tip`; slot 7 a zero normal.  A point may sit in several
        # rows, so each case gets its own table, built row by row over disjoint ids
        rows = idx[:n // 8].copy()
        rows[:] = rng.permutation(n)[:rows.size].reshape(rows.shape).astype(np.uint32)
        for tip, either in ((0.0, True), (1e-3, False), (-1e-3, False)):
            nrm = np.zeros((n, 3), np.float32)
            v = rng.standard_normal((rows.shape[0], 3, 3)).astype(np.float32)
            for q in range(3):
                nrm[rows[:, 2 * q]] = v[:, q]; nrm[rows[:, 2 * q + 1]] = -v[:, q]
            nrm[rows[:, 6]] = (tip * plane_n).astype(np.float32)
            pt.build(xyz, None, nrm)
            got = pt.pca_normals(rows)
            R.check_pca(got, rows, x64, nrm, "sum of normals %g n" % tip, either_sign=either)
            if not either:
                assert (np.sign(got.astype(np.float64) @ plane_n) == np.sign(tip)).all()
        # no attribute table, points exactly on the vertical plane x + 2 y = 1.5 (lattice coordinates): the true n_z is zero, the
        # computed one zero or rounding noise of either sign
        q = np.empty((3, n))
        q[1] = rng.integers(0, 64, n) / 64.0
        q[2] = rng.integers(0, 1024, n) / 1024.0
        q[0] = 1.5 - 2 * q[1]
        xv = q.astype(dtype)
        assert np.array_equal(xv.astype(np.float64), q)
        _build(pt, xv, None)
        got = pt.pca_normals(idx)
        R.check_pca(got, idx, q, None, "vertical plane", either_sign=True)
        assert np.abs(got[:, 2]).max() <= R.pca_bound(8, R.pca_ref(idx, q)[1]).max()
        # a tilted plane without normals: +z decides
        _build(pt, xyz, None)
        got = pt.pca_normals(idx)
        R.check_pca(got, idx, x64, None, "tilted plane, no normals")
        assert (got[:, 2] > 0).all()


# ---- the cached {position, attributes} table ------------------------------------------------------------------------------------
def test_pca_table_follows_the_resident_cloud(pkg):
    """One context, PCA after every change of the cloud or of its attributes.  The fp32 path packs a table on its first call after an
    upload and reuses it; a table that outlived its cloud would answer with the old cloud's normals and a success code.  Cloud B is
    cloud A rotated by 40 degrees, the second attribute set of B is the first negated: a stale table is off by tens of degrees, or
    by the sign."""
    a32, nrm_a = cases.cloud("surface", "f32")
    rot = cases.rotation(40.0)
    b64 = np.ascontiguousarray(rot @ cases.cloud("surface", "f64")[0])
    b32 = b64.astype(np.float32)
    nrm_b = np.ascontiguousarray((nrm_a.astype(np.float64) @ rot.T).astype(np.float32))
    idx, _ = cases.lists("surface", "f32", 16)          # one list throughout: B keeps A's numbering, and PCA takes any list
    idx = np.ascontiguousarray(idx[:1000])
    a16 = a32.astype(np.float16)

    def check(p, xyz, nrm, what):
        for rep in range(2):                             # the second call reuses what the first one packed
            R.check_pca(p.pca_normals(idx), idx, xyz.astype(np.float64), nrm, "%s (call %d)" % (what, rep))

    with pkg.PointsTransfer(device=0) as p:
        p.build(a32, None, nrm_a); check(p, a32, nrm_a, "1: cloud A")
        p.build(b32, None, nrm_b); check(p, b32, nrm_b, "2: cloud B, same n")
        p.set_attributes(None, -nrm_b); check(p, b32, -nrm_b, "3: new attributes on B")
        p.build(a16); check(p, a16, None, "4: fp16 cloud, no attributes")
        p.build(b64, None, nrm_b); check(p, b64, nrm_b, "5: fp64 cloud")
        p.build(a32, None, nrm_a); check(p, a32, nrm_a, "6: cloud A again")
        p.rebuild(); check(p, a32, nrm_a, "6b: after a rebuild of the grid")
        p.set_attributes_range(0, None, -nrm_a, a32.shape[1]); check(p, a32, -nrm_a, "7: attributes by range")
    # the stale answers would indeed fail: A's normals against B's cloud
    with pytest.raises(AssertionError):
        R.check_pca(R.pca_ref(idx, a32.astype(np.float64), nrm_a)[0].astype(np.float32), idx, b32.astype(np.float64), nrm_b, "stale table")


def test_pca_refuses_a_slab(pkg):
    xyz, _ = cases.cloud("volume", "f32")
    half = np.flatnonzero(xyz[0] < 0.5).astype(np.uint32)
    with pkg.PointsTransfer(device=0) as p:
        p.build(np.ascontiguousarray(xyz[:, half]), gidx=half)
        with pytest.raises(pkg.PtError) as e:
            p.pca_normals(np.zeros((4, 8), np.uint32))
        assert e.value.code == pkg.capi.ERR_UNSUPPORTED


# ---- the blend matrix ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capped", [False, True], ids=["uncapped", "capped"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 3, 5, 8, 13, 20, 31, 32])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_blend_matrix(pt, pt_capped, dtype, k, mode, capped):
    """Standalone pt_blend on hand-built lists (cases.blend_case: exact d2 = 0 hits beside neighbours 1e6 times farther, opposite
    normals that cancel, NOIDX at head / middle / tail, ids >= n_attr, empty rows) against blend_ref.  Rows without a valid entry: zeros
    in an uncapped context; in a capped one a row of NOIDX keeps the caller's rgb_out and nrm_out bit for bit."""
    p = pt_capped if capped else pt
    idx, d2, rgb, nrm = cases.blend_case(k)
    n = len(rgb)
    xyz = np.random.default_rng(4).random((3, n)).astype(cases.DTYPES[dtype])
    p.build(xyz, rgb, nrm)
    rng = np.random.default_rng(k)
    sc = (rng.random((len(idx), 3)) * 255).astype(np.float32); sn = rng.standard_normal((len(idx), 3)).astype(np.float32)
    gc, gn = p.blend(idx, d2, mode, rgb_out=sc.copy(), nrm_out=sn.copy())
    rc, rn = R.blend_ref(idx, d2, rgb, nrm, mode)
    valid = (idx != NOIDX) & (idx < n)
    untouched = capped & (idx == NOIDX).all(axis=1)
    assert (untouched.sum() >= 64 if capped else not untouched.any()) and (~valid.any(axis=1)).sum() >= 128
    w = ~untouched
    ec = np.abs(gc[w] - rc[w]).max() / 255.0; en = np.abs(gn[w] - rn[w]).max()
    print("blend %s k=%d mode %d %s: colour err %.3g normal err %.3g" % (dtype, k, mode, "capped" if capped else "uncapped", ec, en))
    assert ec <= TOL and en <= TOL
    assert np.array_equal(gc[untouched].view(np.uint32), sc[untouched].view(np.uint32))
    assert np.array_equal(gn[untouched].view(np.uint32), sn[untouched].view(np.uint32))
    if k >= 2:                                                  # the cancelling rows stayed unnormalised
        assert np.abs(gn[128:192]).max() <= 1e-9 and np.abs(rn[128:192]).max() <= 1e-12
