"""GPU suite of pt_remove_outliers (include/pt_api.h): the statistical and the radius filter on a resident cloud, and its compaction.

Expected values: tests/_outlier_ref.py on the oracle's brute-force lists of the cloud against itself (tests/_outlier_cases.py), so the
search routes, the score kernel, the reductions and the mask are held to lists and sums no kernel of this library produced.  Bounds:
  scores     relative 1e-12: fewer than 32 additions, a square root and a division are at most about 35 * 2^-53 = 4e-15 apart from the
             exactly rounded reference, and the lists themselves are bit-exact;
  threshold  |T - T_ref| <= 1e-9 T_ref: the reductions add n = 5e4 positive terms, worst case n * 2^-53 = 6e-12;
  mask       equal to the reference's outside the band |s - T_ref| <= 1e-9 T_ref, which may hold at most 0.1 % of N -- with these inputs
             it holds no point (tests/test_outlier_ref.py asserts that), so every point is compared;
  radius     no floating-point sum: mask and scores EQUAL the reference's;
  apply      everything afterwards is bit-identical to a fresh context built from the host-compacted arrays."""
import functools

import numpy as np
import pytest

import _attr_cases as cases
import _outlier_cases as OC
import _outlier_ref as R
from _bake_cases import make_case

pytestmark = pytest.mark.gpu

NOIDX = R.NOIDX
N, M = OC.N, cases.M
TORCH_T = {"f32": "float32", "f16": "float16", "f64": "float64"}


def _code(pkg, fn):
    with pytest.raises(pkg.PtError) as e:
        fn()
    return e.value.code


def _targets(xyz):
    return np.ascontiguousarray(xyz[:, :M] + xyz.dtype.type(0.002))


def check_statistical(what, keep, s, info, idx, d2, alpha, max_dist=None):
    rs, rkeep, (nf, mu, sd, T) = R.statistical(idx, d2, alpha, max_dist)
    fin = np.isfinite(rs)
    assert np.array_equal(np.isfinite(s), fin), what + ": the +inf scores differ"
    err, pos = np.abs(s[fin] - rs[fin]), rs[fin] > 0              # (a duplicate's score may be exactly 0: then both are)
    rel = err[pos] / rs[fin][pos]
    print("%s: score rel err %.3g, T %.17g (ref %.17g, rel %.3g), mean rel %.3g, stddev rel %.3g, kept %d" % (
        what, rel.max(), info["threshold"], T, abs(info["threshold"] - T) / T, abs(info["mean"] - mu) / mu, abs(info["stddev"] - sd) / sd, info["n_kept"]))
    assert (err <= 1e-12 * rs[fin]).all(), what
    assert abs(info["threshold"] - T) <= 1e-9 * T and abs(info["mean"] - mu) <= 1e-9 * mu and abs(info["stddev"] - sd) <= 1e-9 * sd, what
    inband = R.band(rs, T, OC.BAND)
    assert inband.sum() <= N // 1000, what
    assert np.array_equal(keep[~inband], rkeep[~inband]), "%s: %d points on the wrong side of T" % (what, (keep[~inband] != rkeep[~inband]).sum())
    assert info["n_before"] == s.shape[0] and info["n_kept"] == int(keep.sum()) and info["n_scored"] == nf, what
    assert np.array_equal(keep, s <= info["threshold"]), what + ": the mask is not `score <= threshold` of the call's own values"
    return rkeep


# ---- 1. the matrix ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,alpha", OC.ALPHAS)
@pytest.mark.parametrize("dtype", OC.DTYPES)
@pytest.mark.parametrize("name", OC.NAMES)
def test_matrix_statistical(pkg, name, dtype, k, alpha):
    xyz, rgb, nrm, _ = OC.cloud(name, dtype)
    idx, d2 = OC.self_lists(name, dtype, k)
    tgt = _targets(xyz)
    with pkg.PointsTransfer(device=0, k_hint=k) as p:
        p.build(xyz, rgb, nrm)
        before = p.query(tgt, 8)
        keep, s, info = p.remove_outliers(k, alpha, apply=False)
        st = p.stats()
        after = p.query(tgt, 8)
        n_after = p.num_source
    assert keep.dtype == np.bool_ and keep.shape == (N,) and s.dtype == np.float64 and s.shape == (N,)
    assert st["n_outlier_chunks"] == 1 and st["ms_outliers"] > 0
    check_statistical("%s %s k=%d alpha=%g" % (name, dtype, k, alpha), keep, s, info, idx, d2, alpha)
    assert n_after == N and np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]), "apply=False changed the cloud"


# ---- 2. radius ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 8, 31])
@pytest.mark.parametrize("dtype", OC.DTYPES)
@pytest.mark.parametrize("name", OC.NAMES)
def test_radius(pkg, name, dtype, m):
    xyz, rgb, nrm, _ = OC.cloud(name, dtype)
    idx, d2 = OC.self_lists(name, dtype, m + 1)
    r = OC.radius_for(name, dtype)
    rs, rkeep = R.radius(idx, d2, r)
    tgt = _targets(xyz)
    with pkg.PointsTransfer(device=0, k_hint=8) as p:
        p.build(xyz, rgb, nrm)
        keep, s, info = p.remove_outliers(radius=r, min_neighbors=m, apply=False)
        assert np.array_equal(keep, rkeep) and np.array_equal(s, rs)
        assert info == dict(n_before=N, n_kept=int(rkeep.sum()), n_scored=N, mean=0.0, stddev=0.0, threshold=float(m))
        assert 0 < info["n_kept"] < N
        # a context capped at 3 r: the call searches under reach r, and the cap is 3 r again afterwards -- also after a failing call
        p.max_dist = 3 * r
        q0 = p.query(tgt, 20)
        assert ((q0[1] > r * r) & (q0[0] != NOIDX)).any() and (q0[0] == NOIDX).any()
        keep3, s3, _ = p.remove_outliers(radius=r, min_neighbors=m, apply=False)
        assert np.array_equal(keep3, rkeep) and np.array_equal(s3, rs)
        q1 = p.query(tgt, 20)
        assert _code(pkg, lambda: p.remove_outliers(radius=r * 1e-7, min_neighbors=31, apply=True)) == pkg.capi.ERR_ARG
        q2 = p.query(tgt, 20)
        for q in (q1, q2):
            assert np.array_equal(q[0], q0[0]) and np.array_equal(q[1], q0[1]), "max_dist was not restored"
        # a cap below r: reach min(r, max_dist)
        p.max_dist = 0.5 * r
        keepc, sc, _ = p.remove_outliers(radius=r, min_neighbors=m, apply=False)
        rsc, rkeepc = R.radius(idx, d2, r, max_dist=0.5 * r)
        assert np.array_equal(keepc, rkeepc) and np.array_equal(sc, rsc)


def test_python_arguments(pkg):
    xyz = OC.cloud("volume", "f32")[0]
    with pkg.PointsTransfer(device=0) as p:
        p.build(xyz)
        with pytest.raises(ValueError):
            p.remove_outliers(radius=0.1)
        with pytest.raises(ValueError):
            p.remove_outliers(min_neighbors=4)
    assert (pkg.capi.OUTLIER_STATISTICAL, pkg.capi.OUTLIER_RADIUS) == (0, 1)


# ---- 3. chunks and routes -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _one_chunk_default(name, dtype, k):
    import __graft_entry__ as g
    pkg = g.load_package()
    with pkg.PointsTransfer(device=0, k_hint=k) as p:
        p.build(OC.cloud(name, dtype)[0])
        return p.remove_outliers(k, 2.0, apply=False), p.remove_outliers(radius=OC.radius_for(name, dtype), min_neighbors=8, apply=False)


@pytest.mark.parametrize("route", ["default", "tile0", "wave_force", "tile0_wave_force"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("name", OC.NAMES)
def test_chunks_and_routes_are_bit_identical(pkg, name, dtype, route):
    """13 chunks of 4096 against one chunk: scores (as 64-bit words), mask, mean, stddev and threshold bit for bit, with the tile kernel,
    without it, with a wave per leftover target and with a wave per target"""
    k = 16
    xyz = OC.cloud(name, dtype)[0]
    base, base_rad = _one_chunk_default(name, dtype, k)
    r = OC.radius_for(name, dtype)
    with pkg.PointsTransfer(device=0, k_hint=k) as p:
        if route.startswith("tile0"):
            p.set_param("tile", 0)
        if route.endswith("wave_force"):
            p.set_param("wave_force", 1)
        p.build(xyz)
        one = p.remove_outliers(k, 2.0, apply=False)
        s1 = p.stats()
        p.set_param("normals_chunk", 4096)
        many = p.remove_outliers(k, 2.0, apply=False)
        s2 = p.stats()
        many_rad = p.remove_outliers(radius=r, min_neighbors=8, apply=False)
    print("%s %s %s: routes %d (one chunk) %d (last of %d chunks)" % (name, dtype, route, s1["query_route"], s2["query_route"], s2["n_outlier_chunks"]))
    assert s1["n_outlier_chunks"] == 1 and s2["n_outlier_chunks"] >= 12
    for st in (s1, s2):
        if route.startswith("tile0"):
            assert not st["query_route"] & pkg.capi.ROUTE_TILE
        elif name == "volume":
            assert st["query_route"] & pkg.capi.ROUTE_TILE
        if route == "tile0_wave_force":
            assert st["query_route"] & (pkg.capi.ROUTE_WAVE | pkg.capi.ROUTE_WAVE_HIER)
    for got, what in ((many, "13 chunks"), (base, "the default route")):
        assert np.array_equal(one[1].view(np.uint64), got[1].view(np.uint64)), "scores differ from " + what
        assert np.array_equal(one[0], got[0]), "mask differs from " + what
        for f in ("mean", "stddev", "threshold"):
            assert np.float64(one[2][f]).view(np.uint64) == np.float64(got[2][f]).view(np.uint64), "%s differs from %s" % (f, what)
        assert one[2] == got[2]
    assert np.array_equal(many_rad[0], base_rad[0]) and np.array_equal(many_rad[1], base_rad[1]) and many_rad[2] == base_rad[2]


# ---- 4. apply -----------------------------------------------------------------------------------------------------------------------
def _records(pkg, verts, vrgb, uv):
    a = np.zeros(verts.shape[1], dtype=pkg.POINT_DTYPE)
    a["ver"] = np.ascontiguousarray(verts.T); a["color"] = vrgb.astype(np.int32); a["U"] = uv[:, 0]; a["V"] = uv[:, 1]; a["normal"] = (0.0, 0.0, 1.0)
    return a


def _resident_xyz(pkg, p, dtype):
    import torch
    out = torch.empty((3, p.num_source), dtype=getattr(torch, TORCH_T[dtype]), device="cuda")
    t = p.resident_source_xyz_dev(out)
    p.synchronize(); torch.cuda.synchronize()
    assert t == {"f32": pkg.capi.F32, "f16": pkg.capi.F16, "f64": pkg.capi.F64}[dtype]
    return out.cpu().numpy()


def _consumers(pkg, p, tgt, second):
    """everything the compacted cloud is asked afterwards; `second`: the arguments of a second remove_outliers (apply=False)"""
    import torch
    C = pkg.capi
    out = [p.query(tgt, 8), p.query(tgt, 20)]
    dev = torch.from_numpy(tgt).cuda()
    p.set_targets(dev, xyz_type={np.float32: C.F32, np.float16: C.F16, np.float64: C.F64}[tgt.dtype.type])
    m = tgt.shape[1]
    i = torch.empty((m, 8), dtype=torch.int32, device="cuda"); d = torch.empty((m, 8), dtype=torch.float64, device="cuda")
    c = torch.zeros((m, 3), dtype=torch.float32, device="cuda"); nn = torch.zeros((m, 3), dtype=torch.float32, device="cuda")
    p.query_blend_resident_dev(8, C.BLEND_INV_D2, i, d, c, nn)
    p.synchronize(); torch.cuda.synchronize()
    out.append((i.cpu().numpy(), d.cpu().numpy(), c.cpu().numpy().view(np.uint32), nn.cpu().numpy().view(np.uint32)))
    out.append(p.remove_outliers(apply=False, **second)[:2])
    out.append((p.estimate_normals(16).view(np.uint32),))           # (last: it rewrites the table's normals)
    return out


@pytest.mark.parametrize("mode", ["statistical", "radius"])
@pytest.mark.parametrize("dtype", OC.DTYPES)
def test_apply_equals_a_fresh_build_of_the_kept_points(pkg, dtype, mode):
    name, k = "surface", 16
    xyz, rgb, nrm, _ = OC.cloud(name, dtype)
    r = OC.radius_for(name, dtype)
    args = dict(k=k, alpha=2.0) if mode == "statistical" else dict(radius=r, min_neighbors=8)
    second = dict(k=8, alpha=1.0) if mode == "statistical" else dict(radius=r, min_neighbors=12)
    tgt = _targets(xyz)
    with pkg.PointsTransfer(device=0, k_hint=k) as p:
        p.build(xyz, rgb, nrm)
        keep, s, info = p.remove_outliers(**args)
        assert 0 < info["n_kept"] < N and info["n_kept"] == keep.sum()
        assert p.num_source == info["n_kept"] and p.stats()["n_source"] == info["n_kept"]
        xk = np.ascontiguousarray(xyz[:, keep])
        assert np.array_equal(_resident_xyz(pkg, p, dtype).view(xyz.dtype.str.replace("f", "u")), xk.view(xyz.dtype.str.replace("f", "u")))
        got = _consumers(pkg, p, tgt, second)
    with pkg.PointsTransfer(device=0, k_hint=k) as f:
        f.build(xk, rgb[keep], nrm[keep])
        want = _consumers(pkg, f, tgt, second)
    for g_, w_, what in zip(got, want, ("k = 8 query", "k = 20 query", "query + blend", "a second remove_outliers", "estimate_normals")):
        for a_, b_ in zip(g_, w_):
            assert a_.shape == b_.shape and np.array_equal(a_, b_), "%s differs from the fresh context's" % what
    assert got[0][0].max() < info["n_kept"]

    # a cloud built WITHOUT attributes filters and queries the same way
    with pkg.PointsTransfer(device=0, k_hint=k) as p:
        p.build(xyz)
        keep2, s2, info2 = p.remove_outliers(**args)
        q = p.query(tgt, 8)
        n2 = p.num_source
    assert np.array_equal(keep2, keep) and np.array_equal(s2.view(np.uint64), s.view(np.uint64)) and info2 == info and n2 == info["n_kept"]
    assert np.array_equal(q[0], got[0][0]) and np.array_equal(q[1], got[0][1])


@pytest.mark.parametrize("dtype", OC.DTYPES)
def test_apply_then_bake_maps(pkg, dtype):
    """a small bake case with strays injected: colour atlas and normal map after the filter equal those of a fresh context"""
    k, res = 8, 128
    src, rgb, verts, uv, vrgb, faces = make_case(31, n=6000, grid=5)
    rng = np.random.default_rng(23)
    src = np.array(src, copy=True)
    src[:, rng.choice(src.shape[1], 60, replace=False)] = (rng.random((60, 3)) * 3 - 1).T
    xyz = np.ascontiguousarray(src.astype(cases.DTYPES[dtype]))
    nrm = rng.standard_normal((xyz.shape[1], 3)).astype(np.float32)
    vrec = _records(pkg, verts, vrgb, uv)
    vxyz = np.ascontiguousarray(verts.astype(xyz.dtype))

    def bake(p):
        vidx = p.query(vxyz, k, want_d2=False)
        return (vidx,) + p.bake_maps(vrec, faces, vidx, res)

    with pkg.PointsTransfer(device=0, k_hint=k) as p:
        p.build(xyz, rgb, nrm)
        keep, _, info = p.remove_outliers(12, 2.0)
        got = bake(p)
    assert 20 <= xyz.shape[1] - info["n_kept"] <= 200
    with pkg.PointsTransfer(device=0, k_hint=k) as f:
        f.build(np.ascontiguousarray(xyz[:, keep]), rgb[keep], nrm[keep])
        want = bake(f)
    for g_, w_, what in zip(got, want, ("vertex lists", "colour atlas", "normal map")):
        assert np.array_equal(g_, w_), what + " differs from the fresh context's"
    assert (got[1][:, :, 3] == 255).mean() > 0.5


# ---- 5. a capped context ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", OC.NAMES)
def test_capped_context(pkg, name):
    k = 16
    xyz, rgb, nrm, stray = OC.cloud(name, "f32")
    idx, d2 = OC.self_lists(name, "f32", k)
    with pkg.PointsTransfer(device=0, k_hint=k, max_dist=OC.CAP) as p:
        p.build(xyz, rgb, nrm)
        keep, s, info = p.remove_outliers(k, 2.0, apply=False)
        p.set_param("normals_chunk", 4096)
        again = p.remove_outliers(k, 2.0, apply=False)
        keep_big, s_big, info_big = p.remove_outliers(k, 1e6, apply=False)
    check_statistical("capped " + name, keep, s, info, idx, d2, 2.0, max_dist=OC.CAP)
    alone = np.isinf(s)
    assert 400 <= alone.sum() <= OC.N_STRAY and np.isin(np.flatnonzero(alone), stray).all()
    assert info["n_scored"] == N - alone.sum() and not keep[alone].any()
    assert np.array_equal(again[1].view(np.uint64), s.view(np.uint64)) and np.array_equal(again[0], keep) and again[2] == info
    # at any alpha the isolated points leave -- and with a huge alpha nobody else does
    assert np.array_equal(keep_big, ~alone) and info_big["n_scored"] == info["n_scored"] and info_big["n_kept"] == N - alone.sum()


# ---- 6. edges and errors ------------------------------------------------------------------------------------------------------------
def test_state_arguments_and_edges(pkg):
    C = pkg.capi
    xyz, rgb, nrm, _ = OC.cloud("surface", "f32")
    tgt = _targets(xyz)
    nan, inf = float("nan"), float("inf")
    with pkg.PointsTransfer(device=0, k_hint=16) as p:
        assert _code(pkg, lambda: p.remove_outliers(16, 2.0)) == C.ERR_STATE                          # before a build
        p.build(xyz, rgb, nrm)
        q0 = p.query(tgt, 8)
        for bad_k in (1, 33, 0, -1):
            assert _code(pkg, lambda: p.remove_outliers(bad_k, 2.0)) == C.ERR_ARG
        for bad_alpha in (-0.5, nan, inf, -inf):
            assert _code(pkg, lambda: p.remove_outliers(16, bad_alpha)) == C.ERR_ARG
        for bad_m in (0, 32, -1):
            assert _code(pkg, lambda: p.remove_outliers(radius=0.05, min_neighbors=bad_m)) == C.ERR_ARG
        for bad_r in (0.0, -1.0, nan, inf):
            assert _code(pkg, lambda: p.remove_outliers(radius=bad_r, min_neighbors=4)) == C.ERR_ARG
        assert p._L.pt_remove_outliers(p._h, 2, 16, 2.0, 0, None, None, 0, None) == C.ERR_ARG         # unknown mode
        # every output is optional
        assert p._L.pt_remove_outliers(p._h, C.OUTLIER_STATISTICAL, 16, 2.0, 0, None, None, 0, None) == C.OK
        # a radius nobody has a neighbour within: everything would go -- refused, and the cloud still answers as before
        assert _code(pkg, lambda: p.remove_outliers(radius=1e-9, min_neighbors=1, apply=True)) == C.ERR_ARG
        assert "every point" in p._L.pt_last_error(p._h).decode()
        q1 = p.query(tgt, 8)
        assert p.num_source == N and np.array_equal(q0[0], q1[0]) and np.array_equal(q0[1], q1[1])
        # a threshold nobody is over: PT_OK, mask of ones, nothing rebuilt
        keep, s, info = p.remove_outliers(16, 1e6, apply=True)
        assert keep.all() and info["n_kept"] == N and s.max() <= info["threshold"] and p.num_source == N
        q2 = p.query(tgt, 8)
        assert np.array_equal(q0[0], q2[0]) and np.array_equal(q0[1], q2[1])
        # an attribute table of another length: the compaction has no meaning for it
        p.set_attributes(np.zeros((N + 5, 3), np.uint8), np.zeros((N + 5, 3), np.float32))
        assert _code(pkg, lambda: p.remove_outliers(16, 2.0)) == C.ERR_STATE
    with pkg.PointsTransfer(device=0) as s_:                                                          # a slab context
        s_.build(xyz, gidx=np.arange(N, dtype=np.uint32))
        assert _code(pkg, lambda: s_.remove_outliers(16, 2.0)) == C.ERR_UNSUPPORTED
    with pkg.PointsTransfer(device=0) as e:                                                           # an empty cloud
        e.build(np.zeros((3, 0), np.float32))
        keep, s, info = e.remove_outliers(16, 2.0)
        assert keep.shape == (0,) and s.shape == (0,) and not any(info.values()) and e.stats()["n_outlier_chunks"] == 0


# ---- 7. "sync" 0 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_enqueue_only_mode(pkg, dtype):
    import torch
    k = 16
    xyz, rgb, nrm, _ = OC.cloud("surface", dtype)
    tgt = _targets(xyz)
    xtype = pkg.capi.F32 if dtype == "f32" else pkg.capi.F64
    with pkg.PointsTransfer(device=0, k_hint=k) as p:
        p.build(xyz, rgb, nrm)
        keep1, s1, info1 = p.remove_outliers(k, 2.0, apply=False)
    with pkg.PointsTransfer(device=0, k_hint=k) as p:
        p.build(xyz, rgb, nrm)
        p.set_param("sync", 0)
        kd = torch.full((N,), 7, dtype=torch.uint8, device="cuda"); sd = torch.full((N,), -1.0, dtype=torch.float64, device="cuda")
        info0 = p.remove_outliers_dev(kd, sd, k, 2.0, apply=False)
        p.synchronize(); torch.cuda.synchronize()
        assert info0 == info1
        assert np.array_equal(kd.cpu().numpy(), keep1.astype(np.uint8)) and np.array_equal(sd.cpu().numpy().view(np.uint64), s1.view(np.uint64))
        # apply, and a query enqueued straight behind it
        info2 = p.remove_outliers_dev(kd, None, k, 2.0, apply=True)
        td = torch.from_numpy(tgt).cuda()
        i = torch.empty((M, 8), dtype=torch.int32, device="cuda"); d = torch.empty((M, 8), dtype=torch.float64, device="cuda")
        p.query_dev(td, xtype, M, 8, i, d)
        p.synchronize(); torch.cuda.synchronize()
        assert info2 == info1 and p.num_source == info1["n_kept"]
    with pkg.PointsTransfer(device=0, k_hint=k) as f:
        f.build(np.ascontiguousarray(xyz[:, keep1]), rgb[keep1], nrm[keep1])
        want = f.query(tgt, 8)
    assert np.array_equal(i.cpu().numpy().view(np.uint32), want[0]) and np.array_equal(d.cpu().numpy(), want[1])
