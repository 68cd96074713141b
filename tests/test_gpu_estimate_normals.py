"""GPU suite of pt_estimate_normals (include/pt_api.h): the normals of a resident cloud from every point's own neighbour list.

Expected lists: the oracle's brute force of the cloud against itself (all N rows), so the search routes, the chunk-as-targets copy and
the self-PCA kernel are held together to lists no kernel of this library produced.  PCA bar: tests/_attr_ref.py's check_pca (unit
length within 1e-6, exactly (0, 0, 1) below three entries, every comparable row within pca_bound) with either_sign=True; the
orientation rule is checked on its own, on the rows where |dot| > 1e-6 |ref| (or |ref - p|).  The shares asserted below (comparable
>= 0.99, decided >= 0.98 for +z and >= 0.9999 for the far viewpoints) are conditions on the INPUT clouds, taken from the reference."""
import functools

import numpy as np
import pytest

import _attr_cases as cases
import _attr_ref as R
from _bake_cases import make_case

pytestmark = pytest.mark.gpu

NOIDX = R.NOIDX
KS = (3, 5, 8, 13, 16, 20, 32)
UP, DOWN = (0.5, 0.5, 10.0), (0.5, 0.5, -10.0)


@functools.lru_cache(maxsize=None)
def self_lists32(name, dtype):
    """the exact 32 nearest neighbours, (d2, id) order, of EVERY point of the cloud among the cloud's points"""
    from oracle import oracle as O
    x64 = cases.cloud(name, dtype)[0].astype(np.float64)
    return O.knn_bruteforce(x64, x64, 32)


def self_lists(name, dtype, k):
    idx, d2 = self_lists32(name, dtype)
    return np.ascontiguousarray(idx[:, :k]), np.ascontiguousarray(d2[:, :k])


def check_orientation(got, idx, x64, ref, viewpoint, what, min_decided):
    """got . d >= 0 with d = ref (axis) or ref - p (viewpoint), on the comparable rows where the reference normal's |dot| with d / |d|
    exceeds 1e-6.  Returns the mask of those rows."""
    want, lam, ke = R.pca_ref(idx, x64, None)
    d = np.asarray(ref, np.float64)[None, :] - (x64.T if viewpoint else 0.0)
    d = np.broadcast_to(d, want.shape) / np.linalg.norm(np.broadcast_to(d, want.shape), axis=1, keepdims=True)
    decided = (ke >= 3) & R.comparable(lam) & (np.abs((want * d).sum(axis=1)) > 1e-6)
    share = decided[ke >= 3].mean() if (ke >= 3).any() else 1.0
    dots = (got.astype(np.float64) * d).sum(axis=1)
    print("%s: decided %.5f, wrong side %d" % (what, share, int((dots[decided] <= 0).sum())))
    assert share >= min_decided, "%s: only %.5f of the rows have a decided orientation" % (what, share)
    assert (dots[decided] > 0).all(), "%s: %d rows point away from the reference" % (what, int((dots[decided] <= 0).sum()))
    return decided


def _code(pkg, fn):
    with pytest.raises(pkg.PtError) as e:
        fn()
    return e.value.code


# ---- 1. the matrix ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dtype", ["f32", "f16", "f64"])
@pytest.mark.parametrize("name", ["surface", "volume"])
def test_matrix_plus_z(pkg, name, dtype, k):
    xyz, _ = cases.cloud(name, dtype)
    x64 = xyz.astype(np.float64)
    idx, _ = self_lists(name, dtype, k)
    with pkg.PointsTransfer(device=0, k_hint=k) as p:
        p.build(xyz)
        got = p.estimate_normals(k)
        st = p.stats()
    assert got.shape == (cases.N, 3) and got.dtype == np.float32
    assert st["n_normal_chunks"] == 1 and st["ms_normals"] > 0
    what = "%s %s k=%d" % (name, dtype, k)
    R.check_pca(got, idx, x64, None, what, either_sign=True)
    check_orientation(got, idx, x64, (0.0, 0.0, 1.0), False, what, 0.98)


# ---- 2. orientation -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16", "f64"])
def test_viewpoint_and_axis(pkg, dtype):
    k = 16
    xyz, _ = cases.cloud("surface", dtype)
    x64 = xyz.astype(np.float64)
    idx, _ = self_lists("surface", dtype, k)
    with pkg.PointsTransfer(device=0, k_hint=k) as p:
        p.build(xyz)
        up = p.estimate_normals(k, viewpoint=UP)
        down = p.estimate_normals(k, viewpoint=DOWN)
        plus = p.estimate_normals(k)
        minus = p.estimate_normals(k, axis=(0.0, 0.0, -1.0))
        with pytest.raises(ValueError):
            p.estimate_normals(k, viewpoint=UP, axis=(0, 0, 1))
    for got, what in ((up, "up"), (down, "down")):
        R.check_pca(got, idx, x64, None, "viewpoint %s %s" % (what, dtype), either_sign=True)
    du = check_orientation(up, idx, x64, UP, True, "viewpoint up " + dtype, 0.9999)
    dd = check_orientation(down, idx, x64, DOWN, True, "viewpoint down " + dtype, 0.9999)
    both = du & dd
    assert np.array_equal(up[both], -down[both]), "the two viewpoints' results are not exact negatives of each other"
    check_orientation(minus, idx, x64, (0.0, 0.0, -1.0), False, "axis -z " + dtype, 0.98)
    flip = plus[:, 2] != 0                                      # (n_z == 0 exactly: both calls keep the sign as computed)
    assert flip.mean() > 0.98
    assert np.array_equal(minus[flip], -plus[flip]) and np.array_equal(minus[~flip], plus[~flip])


# ---- 3. chunks and routes -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _one_chunk_default(name, dtype, k):
    import __graft_entry__ as g
    pkg = g.load_package()
    with pkg.PointsTransfer(device=0, k_hint=k) as p:
        p.build(cases.cloud(name, dtype)[0])
        return p.estimate_normals(k)


@pytest.mark.parametrize("route", ["default", "tile0", "wave_force", "tile0_wave_force"])
@pytest.mark.parametrize("dtype", ["f32", "f16", "f64"])
@pytest.mark.parametrize("name", ["surface", "volume"])
def test_chunks_and_routes_are_bit_identical(pkg, name, dtype, route):
    """13 chunks of 4096 against one chunk, bit for bit, with the tile kernel, without it (group kernel), with a wave per leftover
    target and with a wave per target: every search route feeds the pass the same lists"""
    k = 16
    xyz, _ = cases.cloud(name, dtype)
    base = _one_chunk_default(name, dtype, k)
    with pkg.PointsTransfer(device=0, k_hint=k) as p:
        if route.startswith("tile0"):
            p.set_param("tile", 0)
        if route.endswith("wave_force"):
            p.set_param("wave_force", 1)
        p.build(xyz)
        one = p.estimate_normals(k)
        s1 = p.stats()
        p.set_param("normals_chunk", 4096)
        many = p.estimate_normals(k)
        s2 = p.stats()
        assert _code(pkg, lambda: p.set_param("normals_chunk", 1023)) == pkg.capi.ERR_ARG
    print("%s %s %s: routes %d (one chunk) %d (last of %d chunks)" % (name, dtype, route, s1["query_route"], s2["query_route"], s2["n_normal_chunks"]))
    assert s1["n_normal_chunks"] == 1 and s2["n_normal_chunks"] >= 12
    for st in (s1, s2):
        if route.startswith("tile0"):
            assert not st["query_route"] & pkg.capi.ROUTE_TILE
        elif name == "volume":                                  # (a uniform cloud: nothing keeps the tile kernel from it)
            assert st["query_route"] & pkg.capi.ROUTE_TILE
        if route == "tile0_wave_force":                         # (every target gets a wave; with the tile kernel only its leftovers do)
            assert st["query_route"] & (pkg.capi.ROUTE_WAVE | pkg.capi.ROUTE_WAVE_HIER)
        if route == "tile0" and name == "volume":
            assert st["query_route"] & (pkg.capi.ROUTE_GROUP | pkg.capi.ROUTE_GROUP_HIER)
    assert np.array_equal(one.view(np.uint32), many.view(np.uint32)), "%d rows differ between 1 and %d chunks" % (
        (one.view(np.uint32) != many.view(np.uint32)).any(axis=1).sum(), s2["n_normal_chunks"])
    assert np.array_equal(one.view(np.uint32), base.view(np.uint32)), "route %s changes the result" % route


# ---- 4. the table is written -------------------------------------------------------------------------------------------------------
def _records(pkg, verts, vrgb, uv, vnrm):
    a = np.zeros(verts.shape[1], dtype=pkg.POINT_DTYPE)
    a["ver"] = np.ascontiguousarray(verts.T); a["color"] = vrgb.astype(np.int32); a["U"] = uv[:, 0]; a["V"] = uv[:, 1]; a["normal"] = vnrm
    return a


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_table_is_written_and_colours_kept(pkg, dtype):
    """query + blend and the normal map after estimate_normals equal, bit for bit, those of a context built with the returned array as
    its normals (and the same colours): the stored normals ARE the returned ones, and the colours survived the call"""
    k, res = 8, 128
    src, rgb, verts, uv, vrgb, faces = make_case(31, n=6000, grid=5)
    xyz = np.ascontiguousarray(src.astype(cases.DTYPES[dtype]))
    vrec = _records(pkg, verts, vrgb, uv, np.tile([0.0, 0.0, 1.0], (verts.shape[1], 1)))
    tgt = np.ascontiguousarray(xyz[:, ::7] + xyz.dtype.type(0.003))
    vxyz = np.ascontiguousarray(verts.astype(xyz.dtype))

    def consumers(p):
        idx, d2 = p.query(tgt, k)
        c, nn = p.blend(idx, d2, mode=pkg.BLEND_INV_D2)
        vidx = p.query(vxyz, k, want_d2=False)                  # (planar, in the cloud's own type: pt_query_aos is for fp64 clouds)
        col, nmap = p.bake_maps(vrec, faces, vidx, res)
        return idx, c, nn, col, nmap

    with pkg.PointsTransfer(device=0, k_hint=k) as a:
        a.build(xyz, rgb, None)
        est = a.estimate_normals(12, viewpoint=(0.5, 0.5, 5.0))
        got = consumers(a)
    with pkg.PointsTransfer(device=0, k_hint=k) as b:
        b.build(xyz, rgb, est)
        want = consumers(b)
    with pkg.PointsTransfer(device=0, k_hint=k) as z:
        z.build(xyz, rgb, None)
        flat = consumers(z)
    for g_, w_, what in zip(got, want, ("lists", "blended colour", "blended normal", "colour atlas", "normal map")):
        assert np.array_equal(g_, w_), what + " differs from the context built with the returned normals"
    assert np.abs(np.linalg.norm(got[2], axis=1) - 1).max() < 1e-5 and not flat[2].any()       # blended normals: unit now, zero before
    covered = got[4][:, :, 3] == 255
    assert covered.mean() > 0.5 and not np.array_equal(got[4], flat[4])
    assert np.array_equal(got[1], flat[1]) and np.array_equal(got[3], flat[3])                 # colours: as without the call

    # a cloud built without ANY attributes gets a table with zero colours
    with pkg.PointsTransfer(device=0, k_hint=k) as n:
        n.build(xyz)
        est2 = n.estimate_normals(12, viewpoint=(0.5, 0.5, 5.0))
        idx, d2 = n.query(tgt, k)
        c, nn = n.blend(idx, d2, mode=pkg.BLEND_INV_D2)
    assert np.array_equal(est2, est) and not c.any() and np.array_equal(nn, got[2])


# ---- 5. a capped context ------------------------------------------------------------------------------------------------------------
def test_capped_context(pkg):
    k, r = 16, 0.008
    xyz, _ = cases.cloud("surface", "f32")
    x64 = xyz.astype(np.float64)
    idx, d2 = self_lists("surface", "f32", k)
    idx = np.where(d2 <= r * r, idx, np.uint32(NOIDX)).astype(np.uint32)
    cnt = (idx != NOIDX).sum(axis=1)
    assert (cnt < 3).sum() >= 30 and (cnt == k).sum() >= 1000 and ((cnt >= 3) & (cnt < k)).sum() >= 1000, np.bincount(cnt, minlength=k + 1)
    with pkg.PointsTransfer(device=0, k_hint=k, max_dist=r) as p:
        p.build(xyz)
        got = p.estimate_normals(k)
        p.set_param("normals_chunk", 4096)
        again = p.estimate_normals(k)
    f = R.check_pca(got, idx, x64, None, "capped", min_share=0.95, either_sign=True)
    assert f["few"] == int((cnt < 3).sum())
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
    check_orientation(got, idx, x64, (0.0, 0.0, 1.0), False, "capped", 0.9)


# ---- 6. state and arguments ---------------------------------------------------------------------------------------------------------
def test_state_and_arguments(pkg):
    import torch
    C = pkg.capi
    k = 13
    xyz, _ = cases.cloud("surface", "f32")
    x64 = xyz.astype(np.float64)
    with pkg.PointsTransfer(device=0, k_hint=k) as p:
        assert _code(pkg, lambda: p.estimate_normals(k)) == C.ERR_STATE                       # before a build
        p.build(xyz)
        for bad in (2, 33, 0, -1):
            assert _code(pkg, lambda: p.estimate_normals(bad)) == C.ERR_ARG
        assert _code(pkg, lambda: p.estimate_normals(k, viewpoint=(0.0, float("nan"), 1.0))) == C.ERR_ARG
        assert _code(pkg, lambda: p.estimate_normals(k, axis=(0.0, float("inf"), 1.0))) == C.ERR_ARG
        assert _code(pkg, lambda: p.estimate_normals(k, axis=(0.0, 0.0, 0.0))) == C.ERR_ARG
        assert p._L.pt_estimate_normals(p._h, k, C.ORIENT_VIEWPOINT, None, None, 0) == C.ERR_ARG      # a viewpoint is needed
        assert p._L.pt_estimate_normals(p._h, k, 2, None, None, 0) == C.ERR_ARG                       # unknown mode
        # resident targets survive the call
        tgt = torch.from_numpy(np.ascontiguousarray(xyz[:, :cases.M] + np.float32(0.002))).cuda()
        p.set_targets(tgt, xyz_type=C.F32)
        i0 = torch.empty((cases.M, k), dtype=torch.int32, device="cuda")
        p.query_resident_dev(k, i0)
        first = p.estimate_normals(k)
        assert p.num_targets == cases.M
        i1 = torch.empty_like(i0)
        p.query_resident_dev(k, i1)
        p.synchronize(); torch.cuda.synchronize()
        assert torch.equal(i0, i1)
        # a second call reproduces the first; the device entry equals the host entry
        second = p.estimate_normals(k)
        assert np.array_equal(first.view(np.uint32), second.view(np.uint32))
        out = torch.full((cases.N, 3), float("nan"), device="cuda", dtype=torch.float32)
        p.estimate_normals_dev(k, out)
        p.synchronize(); torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), first.view(np.uint32))
        p.estimate_normals_dev(k, None)                                                       # into the table only
        # pt_pca_normals afterwards orients by the new table
        idx, _ = cases.lists("surface", "f32", k)
        R.check_pca(p.pca_normals(idx), idx, x64, first, "pca after estimate")
        flipped = p.estimate_normals(k, axis=(0.0, 0.0, -1.0))
        R.check_pca(p.pca_normals(idx), idx, x64, flipped, "pca after flipped estimate")
    with pkg.PointsTransfer(device=0) as s:                                                   # a slab context
        s.build(xyz, gidx=np.arange(cases.N, dtype=np.uint32))
        assert _code(pkg, lambda: s.estimate_normals(k)) == C.ERR_UNSUPPORTED
    with pkg.PointsTransfer(device=0) as e:                                                   # an empty cloud
        e.build(np.zeros((3, 0), np.float32))
        assert e.estimate_normals(k).shape == (0, 3) and e.stats()["n_normal_chunks"] == 0


# ---- 7. exact planes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 8, 16])
@pytest.mark.parametrize("dtype", ["f32", "f16", "f64"])
def test_lattice_planes(pkg, oracle, dtype, k):
    """10 x 10 lattice points (multiples of 2^-5: exact in every type) on z = c and on x + y + z = c, each its own cloud"""
    s = 2.0 ** -5
    g = np.array([(i, j) for i in range(10) for j in range(10)], np.float64)
    planes = {"z": np.stack([g[:, 0] * s, g[:, 1] * s, np.full(100, 9 * s)]),
              "111": np.stack([g[:, 0] * s, g[:, 1] * s, (30 - g[:, 0] - g[:, 1]) * s])}
    for name, x64 in planes.items():
        x64 = np.ascontiguousarray(x64)
        xyz = x64.astype(cases.DTYPES[dtype])
        assert np.array_equal(xyz.astype(np.float64), x64)
        idx, _ = oracle.knn_bruteforce(x64, x64, k)
        with pkg.PointsTransfer(device=0, k_hint=k) as p:
            p.build(xyz)
            got = p.estimate_normals(k).astype(np.float64)
        want, lam, ke = R.pca_ref(idx, x64)
        assert (ke == k).all() and R.comparable(lam).all()
        bound = R.pca_bound(k, lam)
        assert (R.sin_angle(got, want) <= bound).all()
        if name == "z":
            assert np.abs(got - [0, 0, 1]).max() <= 2.0 ** -22
        else:
            assert np.abs(got - 1 / np.sqrt(3)).max() <= 2 * bound.max()
