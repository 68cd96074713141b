"""GPU suite of pt_voxel_downsample (include/pt_api.h): voxel-grid downsampling of a resident cloud.

Expected values: tests/_voxel_ref.py (numpy fp64, a stable lexsort, explicit loops for the blocked sums) on the clouds of
tests/_voxel_cases.py.  The definition fixes every rounding and every order of addition, so EVERY comparison here is bit-exact: voxel
numbers, counts, centroids in the stored width, colours, normals, and everything a context answers after apply against a fresh context
built from the reference's arrays.  No tolerance is involved."""
import math

import numpy as np
import pytest

import _attr_cases as cases
import _voxel_cases as VC
import _voxel_ref as R

pytestmark = pytest.mark.gpu

N, M = VC.N, cases.M
TORCH_T = {"f32": "float32", "f16": "float16", "f64": "float64"}
IDS = ["%s-%s-%g" % c for c in VC.MATRIX]


def _code(pkg, fn):
    with pytest.raises(pkg.PtError) as e:
        fn()
    return e.value.code


def _targets(xyz):
    return np.ascontiguousarray(xyz[:, :M] + xyz.dtype.type(0.002))


def _same(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _resident_xyz(pkg, p, dtype):
    import torch
    out = torch.empty((3, p.num_source), dtype=getattr(torch, TORCH_T[dtype]), device="cuda")
    t = p.resident_source_xyz_dev(out)
    p.synchronize(); torch.cuda.synchronize()
    assert t == {"f32": pkg.capi.F32, "f16": pkg.capi.F16, "f64": pkg.capi.F64}[dtype]
    return out.cpu().numpy()


def _check_outputs(what, got, ref, n):
    voxel_of, counts, info = got
    assert voxel_of.dtype == np.uint32 and voxel_of.shape == (n,) and counts.dtype == np.uint32, what
    assert info["n_before"] == n and info["n_voxels"] == ref["n_voxels"] and info["max_count"] == ref["max_count"], (what, info)
    assert info["dims"] == ref["dims"] and info["origin"] == ref["origin"], (what, info)
    assert np.array_equal(counts, ref["counts"]), what + ": counts"
    assert np.array_equal(voxel_of, ref["voxel_of"]), what + ": voxel_of"


# ---- 1. the matrix, apply = 0 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype,v", VC.MATRIX, ids=IDS)
def test_matrix(pkg, name, dtype, v):
    xyz, rgb, nrm = VC.cloud(name, dtype)
    ref = VC.ref(name, dtype, v)
    tgt = _targets(xyz)
    with pkg.PointsTransfer(device=0, k_hint=8) as p:
        p.build(xyz, rgb, nrm)
        before = p.query(tgt, 8)
        got = p.voxel_downsample(v, apply=False)
        st = p.stats()
        after = p.query(tgt, 8)
        n_after = p.num_source
    _check_outputs("%s %s v=%g" % (name, dtype, v), got, ref, N)
    assert got[2]["voxel"] == v
    assert st["n_voxel_passes"] == math.ceil(sum(ref["bits"]) / 8) == ref["passes"] and st["ms_voxel"] > 0
    assert n_after == N and _same(before, after), "apply=False changed the cloud"


# ---- 2. apply -----------------------------------------------------------------------------------------------------------------------
def _consumers(p, tgt):
    q8, q20 = p.query(tgt, 8), p.query(tgt, 20)
    c, nn = p.blend(q8[0], q8[1], mode=1)
    return [q8, q20, (_bits(c), _bits(nn))]


@pytest.mark.parametrize("name,dtype,v", VC.MATRIX, ids=IDS)
def test_apply_equals_a_fresh_build_of_the_reference_points(pkg, name, dtype, v):
    xyz, rgb, nrm = VC.cloud(name, dtype)
    ref = VC.ref(name, dtype, v)
    nv = ref["n_voxels"]
    tgt = _targets(xyz)
    with pkg.PointsTransfer(device=0, k_hint=8) as p:
        p.build(xyz, rgb, nrm)
        got = p.voxel_downsample(v)
        _check_outputs("%s %s v=%g" % (name, dtype, v), got, ref, N)
        assert p.num_source == nv and p.stats()["n_source"] == nv
        res = _resident_xyz(pkg, p, dtype)
        assert res.dtype == xyz.dtype and np.array_equal(_bits(res), _bits(ref["xyz"])), "centroids differ from the reference"
        # the table through the public interface: every centroid's nearest point is itself (or the first centroid at the same position).
        # A mean blend over that one entry returns its colour as it is; it divides the normal by its length (include/pt_api.h), so the
        # stored, NOT renormalised normal is read with the weighted blend at weight 1, which returns the record's floats unchanged
        idx, d2 = p.query(ref["xyz"], 1)
        _, first = np.unique(ref["xyz"].astype(np.float64).T, axis=0, return_inverse=True)
        lowest = np.full(first.max() + 1, nv, np.int64)
        np.minimum.at(lowest, first.ravel(), np.arange(nv))
        want = lowest[first.ravel()]
        assert np.array_equal(idx[:, 0], want) and (d2 == 0).all()
        c, _ = p.blend(idx, d2, mode=0)
        cw, nn = p.blend_weighted(idx, np.ones((nv, 1)))
        assert np.array_equal(c, ref["rgb"][want].astype(np.float32)) and np.array_equal(cw, c), "colours differ from the reference"
        assert np.array_equal(_bits(nn), _bits(ref["nrm"][want])), "normals differ from the reference"
        got_c = _consumers(p, tgt)
        again = p.voxel_downsample(v, origin=got[2]["origin"], apply=False)[2]
        assert again["n_voxels"] == nv and again["n_before"] == nv
    with pkg.PointsTransfer(device=0, k_hint=8) as f:
        f.build(ref["xyz"], ref["rgb"], ref["nrm"])
        want_c = _consumers(f, tgt)
    for g_, w_, what in zip(got_c, want_c, ("k = 8 query", "k = 20 query", "blend")):
        assert _same(g_, w_), "%s differs from the fresh context's" % what


# ---- 3. without an attribute table --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", VC.DTYPES)
def test_without_attributes(pkg, dtype):
    xyz = VC.cloud("surface", dtype)[0]
    ref = VC.ref("surface", dtype, 0.05)
    tgt = _targets(xyz)
    with pkg.PointsTransfer(device=0, k_hint=16) as p:
        p.build(xyz)
        _check_outputs("no attributes " + dtype, p.voxel_downsample(0.05), ref, N)
        assert np.array_equal(_bits(_resident_xyz(pkg, p, dtype)), _bits(ref["xyz"]))
        q = p.query(tgt, 8)
        nrm = p.estimate_normals(16)
    with pkg.PointsTransfer(device=0, k_hint=16) as f:
        f.build(ref["xyz"])
        assert _same(q, f.query(tgt, 8))
        assert np.array_equal(_bits(nrm), _bits(f.estimate_normals(16)))
    assert nrm.shape == (ref["n_voxels"], 3)


# ---- 4. caller origin and bad arguments ---------------------------------------------------------------------------------------------
def test_caller_origin_and_arguments(pkg):
    C = pkg.capi
    xyz, rgb, nrm = VC.cloud("volume", "f32")
    tgt = _targets(xyz)
    nan, inf = float("nan"), float("inf")
    lo = xyz.astype(np.float64).min(axis=1)
    origin = (float(lo[0]) - 0.013, float(lo[1]) - 0.5, float(lo[2]) - 0.0371)
    ref = VC.ref("volume", "f32", 0.05, origin)
    assert ref["n_voxels"] != VC.ref("volume", "f32", 0.05)["n_voxels"]                 # the origin matters
    with pkg.PointsTransfer(device=0, k_hint=8) as p:
        p.build(xyz, rgb, nrm)
        q0 = p.query(tgt, 8)
        got = p.voxel_downsample(0.05, origin=origin, apply=False)
        _check_outputs("caller origin", got, ref, N)
        above = [float(x) for x in lo]
        above[1] = float(np.nextafter(lo[1], np.inf))                                   # above the lowest point of one axis
        bad = [lambda: p.voxel_downsample(0.05, origin=above), lambda: p.voxel_downsample(0.05, origin=(0.5, 0.5, 0.5))]
        bad += [lambda v=v: p.voxel_downsample(v) for v in (0.0, -0.05, nan, inf, -inf)]
        bad += [lambda o=o: p.voxel_downsample(0.05, origin=o) for o in ((nan, 0.0, 0.0), (0.0, inf, 0.0), (0.0, 0.0, -inf))]
        bad += [lambda: p.voxel_downsample(1e-6), lambda: p.voxel_downsample(3.0 / 2 ** 21 * 0.99)]       # an index reaches 2^21
        for fn in bad:
            assert _code(pkg, fn) == C.ERR_ARG
            assert p.num_source == N
        assert _same(q0, p.query(tgt, 8)), "a refused call changed the cloud"
        with pytest.raises(ValueError):
            p.voxel_downsample(0.05, origin=(0.0, 0.0))
        # the largest grid that is allowed: all indices below 2^21 (the strays span just under 3 units)
        ext = float((xyz.astype(np.float64).max(axis=1) - lo).max())
        v_ok = ext / (2 ** 21 - 1)
        r_ok = R.downsample(xyz, v_ok)
        _check_outputs("2^21 - 1", p.voxel_downsample(v_ok, apply=False), r_ok, N)
        assert max(r_ok["dims"]) > 2 ** 21 - 8
        # every output is optional
        assert p._L.pt_voxel_downsample(p._h, 0.05, None, 0, None, None, 0, None) == C.OK


# ---- 5. state errors ----------------------------------------------------------------------------------------------------------------
def test_state_errors_and_the_empty_cloud(pkg):
    C = pkg.capi
    xyz, rgb, nrm = VC.cloud("surface", "f32")
    with pkg.PointsTransfer(device=0) as p:
        assert p._L.pt_voxel_downsample(p._h, 0.05, None, 1, None, None, 0, None) == C.ERR_STATE      # before a build
        p.build(xyz, rgb, nrm)
        p.set_attributes(np.zeros((N + 5, 3), np.uint8), np.zeros((N + 5, 3), np.float32))              # a table of another length
        assert _code(pkg, lambda: p.voxel_downsample(0.05)) == C.ERR_STATE
    with pkg.PointsTransfer(device=0) as s_:
        s_.build(xyz, gidx=np.arange(N, dtype=np.uint32))
        assert _code(pkg, lambda: s_.voxel_downsample(0.05)) == C.ERR_UNSUPPORTED
    with pkg.PointsTransfer(device=0) as e:
        e.build(np.zeros((3, 0), np.float32))
        voxel_of, counts, info = e.voxel_downsample(0.05)
        assert voxel_of.shape == (0,) and counts.shape == (0,) and e.stats()["n_voxel_passes"] == 0
        assert info["n_before"] == 0 and info["n_voxels"] == 0 and info["max_count"] == 0 and info["dims"] == [0, 0, 0]


# ---- 6. sizes around the tile and the block -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", [0.5, 10.0])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4097])
def test_sizes(pkg, n, v):
    xyz, rgb, nrm = VC.cloud("volume", "f32")
    x, c, m = np.ascontiguousarray(xyz[:, :n]), rgb[:n], nrm[:n]
    ref = R.downsample(x, v, None, c, m)
    with pkg.PointsTransfer(device=0) as p:
        p.build(x, c, m)
        _check_outputs("n=%d v=%g" % (n, v), p.voxel_downsample(v), ref, n)
        assert np.array_equal(_bits(_resident_xyz(pkg, p, "f32")), _bits(ref["xyz"]))
        idx, d2 = p.query(ref["xyz"], 1)
        cc, _ = p.blend(idx, d2, mode=0)
        _, nn = p.blend_weighted(idx, np.ones((ref["n_voxels"], 1)))          # (the stored normal: the mean blend would normalise it)
    assert np.array_equal(idx[:, 0], np.arange(ref["n_voxels"]))
    assert np.array_equal(cc, ref["rgb"].astype(np.float32)) and np.array_equal(_bits(nn), _bits(ref["nrm"]))
    if v == 10.0:
        assert ref["n_voxels"] == 1 and ref["max_count"] == n


# ---- 7. determinism and the stream --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_determinism_and_enqueue_only_mode(pkg, dtype):
    import torch
    v = 0.5
    xyz, rgb, nrm = VC.cloud("surface", dtype)
    ref = VC.ref("surface", dtype, v)
    nv = ref["n_voxels"]
    tgt = _targets(xyz)
    runs = []
    for _ in range(2):
        with pkg.PointsTransfer(device=0, k_hint=8) as p:
            p.build(xyz, rgb, nrm)
            voxel_of, counts, info = p.voxel_downsample(v)
            runs.append((voxel_of, counts, _bits(_resident_xyz(pkg, p, dtype))) + tuple(_consumers(p, tgt)[2]))
    assert _same(runs[0], runs[1]), "two runs differ"
    with pkg.PointsTransfer(device=0, k_hint=8) as p:
        p.build(xyz, rgb, nrm)
        p.set_param("sync", 0)
        vd = torch.full((N,), 7, dtype=torch.int32, device="cuda"); cd = torch.full((N,), 7, dtype=torch.int32, device="cuda")
        info0 = p.voxel_downsample_dev(vd, cd, v, apply=False)
        p.synchronize(); torch.cuda.synchronize()
        assert info0 == info and p.num_source == N
        assert np.array_equal(vd.cpu().numpy().view(np.uint32), runs[0][0]) and np.array_equal(cd.cpu().numpy().view(np.uint32)[:nv], runs[0][1])
        assert (cd.cpu().numpy()[nv:] == 7).all(), "count_out was written past n_voxels"
        # apply, and a query enqueued straight behind it on torch's stream
        info1 = p.voxel_downsample_dev(vd, None, v, apply=True)
        td = torch.from_numpy(tgt).cuda()
        i = torch.empty((M, 8), dtype=torch.int32, device="cuda"); d = torch.empty((M, 8), dtype=torch.float64, device="cuda")
        p.query_dev(td, pkg.capi.F32 if dtype == "f32" else pkg.capi.F64, M, 8, i, d)
        p.synchronize(); torch.cuda.synchronize()
        assert info1 == info and p.num_source == nv
        assert np.array_equal(_bits(_resident_xyz(pkg, p, dtype)), runs[0][2])
    with pkg.PointsTransfer(device=0, k_hint=8) as f:
        f.build(ref["xyz"], ref["rgb"], ref["nrm"])
        want = f.query(tgt, 8)
    assert np.array_equal(i.cpu().numpy().view(np.uint32), want[0]) and np.array_equal(d.cpu().numpy(), want[1])


# ---- 8. the clean-up pipeline -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", VC.DTYPES)
def test_pipeline(pkg, dtype):
    xyz, rgb, nrm = VC.cloud("surface", dtype)
    ref = VC.ref("surface", dtype, 0.05)

    def rest(p):
        keep, scores, info = p.remove_outliers(16, 2.0)
        normals = p.estimate_normals(16)
        return keep, _bits(scores), _bits(normals), np.array([info["n_kept"], p.num_source])

    with pkg.PointsTransfer(device=0, k_hint=16) as p:
        p.build(xyz, rgb, nrm)
        p.voxel_downsample(0.05)
        got = rest(p)
    with pkg.PointsTransfer(device=0, k_hint=16) as f:
        f.build(ref["xyz"], ref["rgb"], ref["nrm"])
        want = rest(f)
    assert _same(got, want), "the pipeline on the thinned cloud differs from a fresh context's"
    assert 0 < got[3][0] < ref["n_voxels"]
