"""GPU suite of the enqueue-only mode (pt_set_param "sync" 0) and of the caller-stream plumbing (pt_set_stream, "own_stream").

1. every _dev entry point under "sync" 0 and ONE host wait equals the reference; host-array entry points under "sync" 0 leave their
   inputs free and their outputs complete on return;
2. the routes only "sync" 0 takes -- the 8-lane group kernel over the tile kernel's leftover list, the blend pass over that list, the
   immediate read-back of the retry count -- are proven by pt_stats and answer like the oracle;
3. calls queue behind a slow producer on the caller's stream: the inputs are zeros until a torch.cuda._sleep on a side stream has run,
   so a launch on any other stream cannot match;
4. a switch of streams with work in flight orders the new stream behind the old one (include/pt_api.h at pt_set_stream).

Lists are compared with oracle.knn_bruteforce bit for bit (capped: truncated at d2 <= r*r), blends with _capped.check_blend (1e-5), PCA
and estimated normals with tests/_attr_ref.py on the clouds and under the shares tests/test_gpu_attr_reference.py and
tests/test_gpu_estimate_normals.py hold them to.  The only comparison of the library with itself is "sync" 0 == "sync" 1 in section 2,
on top of the oracle check.  The clouds are test_gpu_tile_variants.py's: exact duplicates, targets on source points, 2.5 % of the targets
outside the bounding box (the tile kernel always hands those over), a dense clump (the retry launch)."""
import ctypes as C
import math

import numpy as np
import pytest

import _attr_cases as cases
import _attr_ref as R
import _tile_variants as TV
from _capped import NOIDX, check_blend, check_exact, truncate
from test_gpu_tile_variants import KMAX, _make_cloud

pytestmark = pytest.mark.gpu

KS = (1, 8, 13, 16, 17, 20, 24, 25, 32)         # both sides of the k > 16 switch, every k bucket (8, 16, 20, 24, 32)
NP_TYPE = {"f32": np.float32, "f64": np.float64, "f16": np.float16}
G_MERGE = 3
# torch.cuda._sleep(SLEEP_CYCLES): the slow producer of sections 3 and 4.  The counter behind _sleep runs at about 2 GHz on the MI355X
# (20 000 000 cycles were measured at 9.4 and 11.0 ms, this value at 63.9 ms); test_sleep_is_long_enough measures it again.
SLEEP_CYCLES = 150_000_000


def _xt(pkg, dtype):
    return {"f32": pkg.F32, "f64": pkg.F64, "f16": pkg.F16}[dtype]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _lists(m, k):
    import torch
    return torch.zeros((m, k), dtype=torch.int32, device="cuda"), torch.zeros((m, k), dtype=torch.float64, device="cuda")


def _np_lists(i_, d_):
    return i_.cpu().numpy().view(np.uint32), d_.cpu().numpy()


def _sentinels(m):
    sc = np.full((m, 3), np.nan, np.float32); sc[1::2] = -7.0          # what an empty row must keep
    sn = np.full((m, 3), 3.0, np.float32)
    return sc, sn


@pytest.fixture(scope="module")
def clouds(oracle):
    """(dtype, scenario) -> dict(src, tgt, rgb, nrm, idx, d2, part_idx, part_d2): the oracle's 32 nearest, taken once (a k-list is its
    first k columns), and the 32 nearest within each third of the cloud (points i with i % 3 == s, global indices): what
    pt_merge_candidates_dev is given.  fp16 clouds are handed to the oracle as the values they hold."""
    cache = {}

    def get(dtype, scenario):
        key = (dtype, scenario)
        if key not in cache:
            src, tgt = _make_cloud(NP_TYPE[dtype], scenario)
            n = src.shape[1]
            s64, t64 = src.astype(np.float64), tgt.astype(np.float64)
            wi, wd = oracle.knn_bruteforce(s64, t64, KMAX)
            parts = [oracle.knn_bruteforce(np.ascontiguousarray(s64[:, s::G_MERGE]), t64, KMAX, gidx=np.arange(s, n, G_MERGE, dtype=np.uint32))
                     for s in range(G_MERGE)]
            cache[key] = dict(src=src, tgt=tgt, rgb=oracle.synth_rgb(0x7A, n), nrm=oracle.synth_nrm(0x7A, n), idx=wi, d2=wd,
                              part_idx=np.stack([p[0] for p in parts]), part_d2=np.stack([p[1] for p in parts]))
        return cache[key]
    return get


# ---- 1. every _dev entry point under "sync" 0 ----------------------------------------------------------------------------------------
def _slab_need_ref(tgt, d2, k, bounds, my, r):
    """numpy restatement of pt_slab_need_dev (as tests/test_gpu_max_dist.py states it): a target's reach is min(k-th d2, r * r)"""
    g = len(bounds) - 1
    reach = np.minimum(d2[:, k - 1], r * r if r is not None else np.inf)
    cx = tgt[0].astype(np.float64)
    want = np.zeros((g, tgt.shape[1]), np.uint8)
    for s in range(g):
        if s == my:
            continue
        lo, hi = bounds[s], bounds[s + 1]
        gap = np.where(cx < lo, lo - cx, np.where(cx >= hi, cx - hi, 0.0))
        want[s] = (gap * gap * (1.0 - 1e-12) <= reach)
    return want, reach


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dtype", ["f32", "f64", "f16"])
def test_dev_entry_points_only_enqueue(pkg, oracle, clouds, dtype, k):
    """One context with "sync" 0; every _dev entry point is called, later calls consuming the DEVICE outputs of earlier ones (the blends
    and the slab tests read the lists the first query is still writing), then one pt_synchronize, then everything is compared.  Without
    a cap, under a small one (the 0.3 quantile of the nearest neighbour's distance: most rows stay empty) and under one of about the
    median k-th distance: capped lists are the truncated oracle lists, capped blends leave empty rows as the sentinels.  fp16: the queries and
    blends (pt_slab_need_dev / pt_pack_requests_dev take fp32 and fp64 only)."""
    import torch
    c = clouds(dtype, "clumped")
    src, tgt, rgb, nrm = c["src"], c["tgt"], c["rgb"], c["nrm"]
    n, m = src.shape[1], tgt.shape[1]
    xt = _xt(pkg, dtype)
    wi, wd = c["idx"][:, :k].copy(), c["d2"][:, :k].copy()
    rng = np.random.default_rng(0xA5 + k)
    w = rng.random((m, k))
    bounds = [-math.inf] + [float(v) for v in np.quantile(src[0].astype(np.float64), np.arange(1, 4) / 4)] + [math.inf]
    my = 1
    sc, sn = _sentinels(m)
    with pkg.PointsTransfer(device=0, k_hint=k) as p:
        p.set_param("sync", 0)
        p.build(src, rgb, nrm)
        x = _dev(tgt)
        p.set_targets(x, xyz_type=xt)
        small = math.sqrt(float(np.quantile(wd[:, 0], 0.3)))
        for r in (None, small, math.sqrt(float(np.median(wd[:, k - 1])))):
            p.max_dist = r
            what = "sync 0 %s k=%d r=%r" % (dtype, k, r)
            want = truncate(wi, wd, r) if r is not None else (wi, wd)
            R2 = r * r if r is not None else np.inf
            out = {}
            # -- enqueue ----------------------------------------------------------------------------------------------------------------
            i1, d1 = _lists(m, k); p.query_resident_dev(k, i1, d1)
            i2, d2 = _lists(m, k); p.query_dev(x, xt, m, k, i2, d2)
            bnd = wd[:, k - 1].copy(); bnd[::2] *= 0.5                  # every other row's bound halved: those rows come back shorter
            i3, d3 = _lists(m, k); p.query_bounded_dev(x, xt, _dev(bnd), m, k, i3, d3)
            for mode in (pkg.BLEND_MEAN, pkg.BLEND_INV_D2):
                fi, fd = _lists(m, k); fc, fn = _dev(sc), _dev(sn)
                p.query_blend_resident_dev(k, mode, fi, fd, fc, fn)
                bc, bn = _dev(sc), _dev(sn)
                p.blend_dev(i1, d1, m, k, mode, bc, bn)                  # (reads the lists the first query writes)
                out[mode] = (fi, fd, fc, fn, bc, bn)
            wc, wn = _dev(sc), _dev(sn)
            p.blend_weighted_dev(_dev(want[0].view(np.int32)), _dev(w), m, k, wc, wn)
            pi, pd = truncate(c["part_idx"][:, :, :k], c["part_d2"][:, :, :k], r) if r is not None else (c["part_idx"][:, :, :k], c["part_d2"][:, :, :k])
            mi, md = _lists(m, k)
            p.merge_candidates_dev(_dev(pi.view(np.int32)), _dev(pd), G_MERGE, m, k, mi, md)
            if dtype != "f16":
                need = torch.zeros((4, m), dtype=torch.uint8, device="cuda")
                p.slab_need_dev(x, xt, d1, m, k, 0, bounds, my, need)
                sel = torch.zeros(m, dtype=torch.int32, device="cuda"); pkt = torch.zeros((m, 5), dtype=torch.float64, device="cuda")
                cnt = p.pack_requests_dev(x, xt, d1, m, k, 0, bounds, my, sel, pkt)
            ids = torch.full((m,), -1, dtype=torch.int32, device="cuda"); p.resident_target_ids_dev(ids)
            back = torch.zeros_like(x) if dtype != "f16" else torch.zeros((3, m), dtype=torch.float32, device="cuda")
            p.resident_target_xyz_dev(back)
            # -- one wait, then read -------------------------------------------------------------------------------------------------
            p.synchronize()
            check_exact(_np_lists(i1, d1), want, what + " query_resident")
            check_exact(_np_lists(i2, d2), want, what + " query_soa(on_device)")
            keep = wd <= np.minimum(bnd, R2)[:, None]
            check_exact(_np_lists(i3, d3), (np.where(keep, wi, np.uint32(NOIDX)), np.where(keep, wd, np.inf)), what + " query_bounded_dev")
            for mode, (fi, fd, fc, fn, bc, bn) in out.items():
                check_exact(_np_lists(fi, fd), want, what + " fused lists mode %d" % mode)
                empty = check_blend(fc.cpu().numpy(), fn.cpu().numpy(), want[0], want[1], rgb, nrm, mode, sc, sn, oracle, what + " fused blend mode %d" % mode)
                assert empty == 0 if r is None else (empty > 0 or r != small), what + ": %d rows without a neighbour" % empty
                check_blend(bc.cpu().numpy(), bn.cpu().numpy(), want[0], want[1], rgb, nrm, mode, sc, sn, oracle, what + " blend_dev mode %d" % mode)
            rc, rn = oracle.blend_weighted(want[0], w, rgb, nrm)
            assert np.array_equal(wc.cpu().numpy(), rc) and np.array_equal(wn.cpu().numpy(), rn), what + " blend_weighted_dev"
            check_exact(_np_lists(mi, md), want, what + " merge_candidates_dev")
            if dtype != "f16":
                wneed, reach = _slab_need_ref(tgt, want[1], k, bounds, my, r)
                assert np.array_equal(need.cpu().numpy(), wneed), what + " slab_need_dev"
                rows = np.nonzero(wneed.any(axis=0))[0]
                assert 0 < len(rows) < m and cnt == len(rows), what + " pack_requests_dev: %d packets, %d rows need another slab" % (cnt, len(rows))
                got_rows = sel[:cnt].cpu().numpy()
                o = np.argsort(got_rows)
                pk = pkt[:cnt].cpu().numpy()[o]
                assert np.array_equal(got_rows[o], rows), what + " pack_requests_dev: selected rows"
                assert np.array_equal(pk[:, :3], tgt[:, rows].T.astype(np.float64)) and np.array_equal(pk[:, 3], reach[rows]), what + " packets"
                masks = (wneed[:, rows].astype(np.uint64) << np.arange(4, dtype=np.uint64)[:, None]).sum(axis=0)
                assert np.array_equal(pk[:, 4].astype(np.uint64), masks), what + " packet masks"
            assert np.array_equal(ids.cpu().numpy(), np.arange(m, dtype=np.int32)), what + " resident_target_ids"
            assert np.array_equal(back.cpu().numpy(), tgt.astype(np.float32) if dtype == "f16" else tgt), what + " resident_target_xyz"


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dtype", ["f32", "f64", "f16"])
def test_pca_normals_dev_only_enqueues(pkg, dtype, k):
    """pt_pca_normals_dev under "sync" 0 on the surface cloud of the attribute reference tests (>= 0.99 of its rows comparable), the first
    call building the packed table of fp32 / fp16 clouds in the same enqueue; and the host entry point with its input overwritten"""
    import torch
    xyz, nrm = cases.cloud("surface", dtype)
    idx, _ = cases.lists("surface", dtype, k)
    with pkg.PointsTransfer(device=0) as p:
        p.set_param("sync", 0)
        p.build(xyz, None, nrm)
        outs = [torch.full((cases.M, 3), float("nan"), device="cuda", dtype=torch.float32) for _ in range(2)]
        di = _dev(idx.view(np.int32))
        for o in outs:
            p.pca_normals_dev(di, cases.M, k, o)
        p.synchronize()
        host_in = idx.copy()
        host = p.pca_normals(host_in)
        host_in[:] = 7
    for what, got in (("first call", outs[0].cpu().numpy()), ("second call", outs[1].cpu().numpy()), ("host entry", host)):
        R.check_pca(got, idx, xyz.astype(np.float64), nrm, "sync 0 pca %s %s k=%d" % (what, dtype, k))


@pytest.mark.parametrize("k", [16, 17, 32])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_pca_normals_dev_capped_only_enqueues(pkg, oracle, dtype, k):
    """the capped context of test_gpu_attr_reference.py (targets leaving the surface, r = 0.012, share >= 0.95; there k = 16) under
    "sync" 0, on both sides of the k > 16 switch and at PT_MAX_K: the capped query's device lists go straight into pt_pca_normals_dev;
    the lists are the truncated oracle lists.  (Within r = 0.012 the surface holds about 23 points: full rows are rare above k = 16.)"""
    import torch
    r = 0.012
    xyz, nrm = cases.cloud("surface", dtype)
    tgt = np.array(xyz[:, :cases.M], copy=True)
    tgt[2] += np.linspace(0.0, 0.03, cases.M).astype(xyz.dtype)
    want = truncate(*oracle.knn_bruteforce(xyz.astype(np.float64), tgt.astype(np.float64), k), r)
    cnt = (want[0] != NOIDX).sum(axis=1)
    assert ((cnt == k).sum() > 50 or k > 16) and (cnt == 0).sum() > 50 and ((cnt >= 3) & (cnt < k)).sum() > 50
    with pkg.PointsTransfer(device=0, max_dist=r) as p:
        p.set_param("sync", 0)
        p.build(xyz, None, nrm)
        i_, d_ = _lists(cases.M, k)
        out = torch.full((cases.M, 3), float("nan"), device="cuda", dtype=torch.float32)
        p.query_dev(_dev(tgt), _xt(pkg, dtype), cases.M, k, i_, d_)
        p.pca_normals_dev(i_, cases.M, k, out)
        p.synchronize()
    check_exact(_np_lists(i_, d_), want, "sync 0 capped lists %s k=%d" % (dtype, k))
    R.check_pca(out.cpu().numpy(), want[0], xyz.astype(np.float64), nrm, "sync 0 capped pca %s k=%d" % (dtype, k), min_share=0.95)


@pytest.mark.parametrize("k", [k for k in KS if k >= 3])
@pytest.mark.parametrize("dtype", ["f32", "f16", "f64"])
def test_estimate_normals_dev_only_enqueues(pkg, dtype, k):
    """pt_estimate_normals with a device nrm_out and 13 chunks of 4096 under "sync" 0: every chunk's search and PCA is queued behind the
    previous one's, reusing the same list buffer; one wait; test_gpu_estimate_normals.py's bars (its clouds, its shares).  Every k of
    the matrix the call admits (k = 1 is PT_ERR_ARG: it needs three neighbours): each chunk's search routes on k > 16 like any query."""
    import torch
    from test_gpu_estimate_normals import check_orientation, self_lists
    xyz, _ = cases.cloud("surface", dtype)
    x64 = xyz.astype(np.float64)
    idx, _ = self_lists("surface", dtype, k)
    with pkg.PointsTransfer(device=0, k_hint=k) as p:
        p.set_param("sync", 0)
        p.set_param("normals_chunk", 4096)
        p.build(xyz)
        out = torch.full((cases.N, 3), float("nan"), device="cuda", dtype=torch.float32)
        p.estimate_normals_dev(k, out)
        p.synchronize()
        st = p.stats()
    assert st["n_normal_chunks"] >= 12
    got = out.cpu().numpy()
    what = "sync 0 estimate_normals %s k=%d" % (dtype, k)
    R.check_pca(got, idx, x64, None, what, either_sign=True)
    check_orientation(got, idx, x64, (0.0, 0.0, 1.0), False, what, 0.98)


@pytest.mark.parametrize("k", [16, 17, 25])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_estimate_normals_dev_capped_only_enqueues(pkg, dtype, k):
    """... and under the cap of test_gpu_estimate_normals.py's capped context (r = 0.008, shares >= 0.95 and 0.9; there fp32, k = 16),
    on both sides of the k > 16 switch and in the widest k bucket"""
    import torch
    from test_gpu_estimate_normals import check_orientation, self_lists
    r = 0.008
    xyz, _ = cases.cloud("surface", dtype)
    x64 = xyz.astype(np.float64)
    idx, d2 = self_lists("surface", dtype, k)
    idx = np.where(d2 <= r * r, idx, np.uint32(NOIDX)).astype(np.uint32)
    with pkg.PointsTransfer(device=0, k_hint=k, max_dist=r) as p:
        p.set_param("sync", 0)
        p.set_param("normals_chunk", 4096)
        p.build(xyz)
        out = torch.full((cases.N, 3), float("nan"), device="cuda", dtype=torch.float32)
        p.estimate_normals_dev(k, out)
        p.synchronize()
    got = out.cpu().numpy()
    what = "sync 0 capped estimate_normals %s k=%d" % (dtype, k)
    f = R.check_pca(got, idx, x64, None, what, min_share=0.95, either_sign=True)
    assert f["few"] == int(((idx != NOIDX).sum(axis=1) < 3).sum())
    check_orientation(got, idx, x64, (0.0, 0.0, 1.0), False, what, 0.9)


@pytest.mark.parametrize("dtype", ["f32", "f64", "f16"])
def test_host_entry_points_under_sync_0(pkg, oracle, clouds, dtype):
    """build, set_attributes, set_attributes_range, set_targets, query and blend on host arrays under "sync" 0: every input is overwritten
    with garbage the moment its call returns, every output is compared without any further wait"""
    c = clouds(dtype, "clumped")
    k = 13
    n, m = c["src"].shape[1], c["tgt"].shape[1]
    want = (c["idx"][:, :k].copy(), c["d2"][:, :k].copy())
    z = np.zeros((m, 3), np.float32)                            # (no cap: no row is empty, nothing is compared with these)

    def spoil(*arrays):
        for a in arrays:
            a[...] = 77
    with pkg.PointsTransfer(device=0, k_hint=k) as p:
        p.set_param("sync", 0)
        src, rgb, nrm = c["src"].copy(), c["rgb"].copy(), c["nrm"].copy()
        p.build(src, rgb, nrm)
        spoil(src, rgb, nrm)
        tgt = c["tgt"].copy()
        got = p.query(tgt, k)
        spoil(tgt)
        check_exact(got, want, "host query %s" % dtype)
        for mode in (pkg.BLEND_MEAN, pkg.BLEND_INV_D2):
            i_, d_ = want[0].copy(), want[1].copy()
            gc, gn = p.blend(i_, d_, mode=mode)
            spoil(i_, d_)
            check_blend(gc, gn, want[0], want[1], c["rgb"], c["nrm"], mode, z, z, oracle, "host blend %s mode %d" % (dtype, mode))
        # a second table, uploaded whole and then in three ranges: the blends read the new records
        rgb2, nrm2 = oracle.synth_rgb(0x7B, n), oracle.synth_nrm(0x7B, n)
        a, b = rgb2.copy(), nrm2.copy()
        p.set_attributes(a, b)
        spoil(a, b)
        gc, gn = p.blend(want[0], want[1], mode=pkg.BLEND_INV_D2)
        check_blend(gc, gn, want[0], want[1], rgb2, nrm2, pkg.BLEND_INV_D2, z, z, oracle, "host blend after set_attributes %s" % dtype)
        for lo, hi in ((0, n // 3), (n // 3, n - 5), (n - 5, n)):
            a, b = c["rgb"][lo:hi].copy(), c["nrm"][lo:hi].copy()
            p.set_attributes_range(lo, a, b, n)
            spoil(a, b)
        gc, gn = p.blend(want[0], want[1], mode=pkg.BLEND_MEAN)
        check_blend(gc, gn, want[0], want[1], c["rgb"], c["nrm"], pkg.BLEND_MEAN, z, z, oracle, "host blend after set_attributes_range %s" % dtype)
        # host targets made resident, then searched by a _dev call with nothing in between
        tgt = c["tgt"].copy()
        p.set_targets(tgt)
        spoil(tgt)
        i_, d_ = _lists(m, k)
        p.query_resident_dev(k, i_, d_)
        p.synchronize()
        check_exact(_np_lists(i_, d_), want, "set_targets(host) + query_resident %s" % dtype)


# ---- 2. the routes only "sync" 0 takes -------------------------------------------------------------------------------------------------
SETUPS = {                                       # name -> (tile, tile_sparse, scenario)
    "tile2-clumped": (2, 0, "clumped"),
    "tile3-uniform": (3, 0, "uniform"),
    "tile3-sparse": (3, 1, "uniform"),
    "tile2-sparse": (2, 1, "clumped"),
}
ROUTE_KS = (8, 13, 16, 17, 24, 32)


def _row(k, tile, fused, f64):
    """the row of tests/_tile_variants.py whose instantiation answers k under pt_set_param("tile", tile), uncapped"""
    geometry = "large" if tile == 3 else ("small" if k <= 16 else "medium")
    K, cap, twg, wide, kc = TV.expected_route(k, geometry, "none")
    rows = [r for r in TV.ROWS if (r["K"], r["CAP"], r["TWG"], r["WIDE"], r["KC"]) == (K, cap, twg, wide, kc) and r["BLEND"] == fused and r["DBL"] == f64 and not r["BND"]]
    assert len(rows) == 1
    return rows[0]


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("setup", list(SETUPS))
def test_routes_of_sync_0(pkg, oracle, clouds, setup, dtype, fused):
    """Per k: (a) "sync" 1, "wave_min" 0 -- the same tile launch, the group kernel takes the leftovers: n_leftover > 0, and on the
    two-per-CU geometries (tile 2, k <= 24; k in 25..32 has none: csrc/pt_tile_route.h runs the wide geometry whatever is asked)
    tile_retry_blocks > 0 -- conditions on the clouds; (b) "sync" 1, default "wave_min": TILE | WAVE; (c) "sync" 0: TILE | GROUP at
    k <= 16 (+ BLEND_LIST when fused) and no wave bit, TILE | WAVE above.  tile_variant names the row's instantiation in all three
    (and its retry, read back at once under (c) at k <= 16, with the leftover count otherwise); lists and blends equal the oracle's in
    all three, and (c)'s lists equal (b)'s."""
    Cx = pkg.capi
    tile, sparse, scenario = SETUPS[setup]
    c = clouds(dtype, scenario)
    src, tgt, rgb, nrm = c["src"], c["tgt"], c["rgb"], c["nrm"]
    m = tgt.shape[1]
    sc, sn = _sentinels(m)
    WAVES, GROUPS = Cx.ROUTE_WAVE | Cx.ROUTE_WAVE_HIER, Cx.ROUTE_GROUP | Cx.ROUTE_GROUP_HIER
    for k in ROUTE_KS:
        row = _row(k, tile, fused, dtype == "f64")
        want = (c["idx"][:, :k].copy(), c["d2"][:, :k].copy())
        with pkg.PointsTransfer(device=0, k_hint=k) as p:
            p.set_param("tile", tile); p.set_param("tile_sparse", sparse)
            p.build(src, rgb, nrm)
            p.set_targets(tgt)

            def run(what):
                res = []
                for mode in ((pkg.BLEND_MEAN, pkg.BLEND_INV_D2) if fused else (None,)):
                    i_, d_ = _lists(m, k)
                    if mode is None:
                        p.query_resident_dev(k, i_, d_)
                    else:
                        c_, n_ = _dev(sc), _dev(sn)
                        p.query_blend_resident_dev(k, mode, i_, d_, c_, n_)
                    st = p.stats()                              # (the route is known when the call returns, whatever "sync" is)
                    p.synchronize()
                    got = _np_lists(i_, d_)
                    check_exact(got, want, what)
                    if mode is not None:
                        check_blend(c_.cpu().numpy(), n_.cpu().numpy(), want[0], want[1], rgb, nrm, mode, sc, sn, oracle, "%s mode %d" % (what, mode))
                    v = st["tile_variant"]
                    assert v[0] == TV.row_code(row, listed=bool(sparse)), "%s: the tile launch ran %s" % (what, TV.decode(v[0]))
                    if row["retry"]:
                        assert st["tile_retry_blocks"] > 0 and v[1] == TV.retry_code(row), "%s: retry %s over %d blocks" % (what, TV.decode(v[1]), st["tile_retry_blocks"])
                    else:
                        assert st["tile_retry_blocks"] == 0 and v[1] == 0, what
                    res.append((st, got))
                return res
            what = "%s %s k=%d %s" % (setup, dtype, k, "fused" if fused else "plain")
            p.set_param("sync", 1); p.set_param("wave_min", 0)
            for st, _ in run(what + " (a) sync 1 wave_min 0"):
                assert st["n_leftover"] > 0, what + ": the tile kernel handed nothing over"
                assert st["query_route"] == Cx.ROUTE_TILE | Cx.ROUTE_GROUP | (Cx.ROUTE_BLEND_LIST if fused else 0), (what, st["query_route"])
            p.set_param("wave_min", 1)
            pinned = run(what + " (b) sync 1")
            for st, _ in pinned:
                assert st["n_leftover"] > 0 and st["n_wave"] == st["n_leftover"], what
                assert st["query_route"] == Cx.ROUTE_TILE | Cx.ROUTE_WAVE, (what, st["query_route"])
            p.set_param("sync", 0)
            for (st, got), (_, ref) in zip(run(what + " (c) sync 0"), pinned):
                route = st["query_route"]
                if k <= 16:
                    assert route & Cx.ROUTE_TILE and route & Cx.ROUTE_GROUP and not route & WAVES, (what, route)
                    assert bool(route & Cx.ROUTE_BLEND_LIST) == fused, (what, route)
                else:
                    assert route == Cx.ROUTE_TILE | Cx.ROUTE_WAVE and not route & GROUPS, (what, route)
                assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), what + ": sync 0 and sync 1 lists differ"


@pytest.mark.parametrize("wave_min", [0, 1])
@pytest.mark.parametrize("tile", [0, 1])
def test_refined_cells_under_sync_0(pkg, oracle, tile, wave_min):
    """test_gpu_parity.py's refined blobs (a low "refine_threshold": nodes everywhere) under "sync" 0: the descending group kernel
    ("wave_min" 0) or the wave pair, unbounded and with every other row's bound halved, equal to brute force bit for bit"""
    from test_gpu_stress import _cloud
    Cx = pkg.capi
    k, thr = 8, 24
    rng = np.random.default_rng(77 + k)
    n, m = 60000, 3000
    src = _cloud(rng, "blobs", n); tgt = _cloud(rng, "blobs", m)
    tgt[:, :100] = tgt[:, :100] * np.float32(3.0) - np.float32(1.0)
    tgt[:, 100:400] = src[:, rng.integers(0, n, 300)]
    want = oracle.knn_bruteforce(src, tgt, k)
    with pkg.PointsTransfer(device=0, k_hint=k) as p:
        p.set_param("refine_threshold", thr); p.set_param("tile", tile); p.set_param("wave_min", wave_min)
        p.build(src)
        assert p.stats()["n_nodes"] > 0
        p.set_param("sync", 0)
        x = _dev(tgt)
        i_, d_ = _lists(m, k)
        p.query_dev(x, pkg.F32, m, k, i_, d_)
        route = p.stats()["query_route"]
        bnd = want[1][:, k - 1].copy(); bnd[::2] *= 0.5
        bi, bd = _lists(m, k)
        p.query_bounded_dev(x, pkg.F32, _dev(bnd), m, k, bi, bd)
        broute = p.stats()["query_route"]
        p.synchronize()
    for r_ in (route, broute):
        if wave_min:
            assert r_ & (Cx.ROUTE_WAVE | Cx.ROUTE_WAVE_HIER) and not r_ & (Cx.ROUTE_GROUP | Cx.ROUTE_GROUP_HIER), r_
        else:
            assert r_ & Cx.ROUTE_GROUP_HIER and not r_ & (Cx.ROUTE_WAVE | Cx.ROUTE_WAVE_HIER), r_
    check_exact(_np_lists(i_, d_), want, "refined, sync 0, tile %d wave_min %d" % (tile, wave_min))
    keep = want[1] <= bnd[:, None]
    check_exact(_np_lists(bi, bd), (np.where(keep, want[0], np.uint32(NOIDX)), np.where(keep, want[1], np.inf)), "refined bounded, sync 0")


# ---- 3. stream ordering ------------------------------------------------------------------------------------------------------------
def _slow_copy(S, pairs):
    """on stream S: a long sleep, then the copies dst <- real; returns the event recorded behind them.  Until it has run, every dst
    holds zeros"""
    import torch
    with torch.cuda.stream(S):
        torch.cuda._sleep(SLEEP_CYCLES)
        for dst, real in pairs:
            dst.copy_(real, non_blocking=True)
        E = torch.cuda.Event()
        E.record(S)
    return E


def test_sleep_is_long_enough():
    """torch.cuda._sleep(SLEEP_CYCLES), SLEEP_CYCLES = 150 000 000, must keep a stream busy for at least 50 ms -- hundreds of times the
    host time of an enqueue-only call (tens of microseconds per launch, a dozen launches).  Measured on the MI355X: 20 000 000 cycles
    took 9.4 and 11.0 ms (a counter of about 2 GHz), and this value 63.9 ms; the figure is printed."""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record(); torch.cuda._sleep(SLEEP_CYCLES); b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b)
    print("torch.cuda._sleep(%d): %.1f ms" % (SLEEP_CYCLES, ms))
    assert ms >= 50.0


@pytest.fixture(scope="module")
def _stream_ctx(pkg, clouds):
    """the uniform fp32 cloud, k = 8, on the route without any host read-back ("tile" 3 over all blocks, k <= 16): under "sync" 0 its
    queries only enqueue.  Every test warms its calls up with one synchronous round first, so that the round that counts allocates
    nothing (an allocation may wait for the device)."""
    c = clouds("f32", "uniform")
    p = pkg.PointsTransfer(device=0, k_hint=8)
    p.set_param("tile", 3); p.set_param("tile_sparse", 0)
    p.build(c["src"], c["rgb"], c["nrm"])
    yield p, c, 8
    p.close()


@pytest.fixture
def stream_case(_stream_ctx):
    """... handed to one test; whatever that test did or failed at, the shared context is back under "sync" 1 afterwards"""
    try:
        yield _stream_ctx
    finally:
        _stream_ctx[0].set_param("sync", 1)


ENTRIES = ["query_dev", "query_bounded_dev", "blend_dev", "merge_candidates_dev", "set_targets+query_resident_dev", "set_targets+query_blend_resident_dev"]


def _call_entry(pkg, oracle, p, c, k, entry, S, sync):
    """the five steps of section 3 for one entry point: zero-filled inputs, the slow producer and the call on S, a consumer on S, S
    alone synchronised, the consumer's clone compared.  Returns E.query() as read the moment the call returned (None: warm-up)."""
    import torch
    m = c["tgt"].shape[1]
    want = (c["idx"][:, :k].copy(), c["d2"][:, :k].copy())
    sc, sn = _sentinels(m)
    mode = pkg.BLEND_INV_D2
    bnd = want[1][:, k - 1].copy(); bnd[::2] *= 0.5
    real = {"x": _dev(c["tgt"]), "b": _dev(bnd), "i": _dev(want[0].view(np.int32)), "d": _dev(want[1]),
            "pi": _dev(c["part_idx"][:, :, :k].view(np.int32)), "pd": _dev(c["part_d2"][:, :, :k])}
    late = {key: torch.zeros_like(v) for key, v in real.items()}
    i_, d_ = _lists(m, k)
    c_, n_ = _dev(sc), _dev(sn)
    needs = {"query_dev": "x", "query_bounded_dev": "xb", "blend_dev": "id", "merge_candidates_dev": ("pi", "pd")}.get(entry, "x")
    torch.cuda.synchronize()
    p.set_param("sync", sync)
    E = _slow_copy(S, [(late[key], real[key]) for key in needs])
    with torch.cuda.stream(S):
        if entry == "query_dev":
            p.query_dev(late["x"], pkg.F32, m, k, i_, d_)
        elif entry == "query_bounded_dev":
            p.query_bounded_dev(late["x"], pkg.F32, late["b"], m, k, i_, d_)
        elif entry == "blend_dev":
            p.blend_dev(late["i"], late["d"], m, k, mode, c_, n_)
        elif entry == "merge_candidates_dev":
            p.merge_candidates_dev(late["pi"], late["pd"], G_MERGE, m, k, i_, d_)
        elif entry == "set_targets+query_resident_dev":
            p.set_targets(late["x"], xyz_type=pkg.F32)
            p.query_resident_dev(k, i_, d_)
        else:
            p.set_targets(late["x"], xyz_type=pkg.F32)
            p.query_blend_resident_dev(k, mode, i_, d_, c_, n_)
        done = E.query()
        got = [t.clone() for t in (i_, d_, c_, n_)]
    S.synchronize()
    gi, gd = _np_lists(got[0], got[1])
    what = "%s on a side stream, sync %d" % (entry, sync)
    if entry == "blend_dev":
        check_blend(got[2].cpu().numpy(), got[3].cpu().numpy(), want[0], want[1], c["rgb"], c["nrm"], mode, sc, sn, oracle, what)
    elif entry == "query_bounded_dev":
        keep = want[1] <= bnd[:, None]
        check_exact((gi, gd), (np.where(keep, want[0], np.uint32(NOIDX)), np.where(keep, want[1], np.inf)), what)
    else:
        check_exact((gi, gd), want, what)
        if entry.endswith("query_blend_resident_dev"):
            check_blend(got[2].cpu().numpy(), got[3].cpu().numpy(), want[0], want[1], c["rgb"], c["nrm"], mode, sc, sn, oracle, what)
    return done


@pytest.mark.parametrize("sync", [0, 1])
@pytest.mark.parametrize("entry", ENTRIES)
def test_calls_queue_behind_the_callers_stream(pkg, oracle, stream_case, entry, sync):
    """The inputs are zeros until torch.cuda._sleep(SLEEP_CYCLES = 150 000 000, 64 ms when measured; measured by test_sleep_is_long_enough) and the copies
    behind it have run on side stream S; the call is made under S.  A launch on any other stream reads zeros.  Under "sync" 0 the
    producer's event must still be pending when the call returns: the call enqueued behind a producer that was still running."""
    import torch
    p, c, k = stream_case
    S = torch.cuda.Stream()
    _call_entry(pkg, oracle, p, c, k, entry, S, 1)               # warm-up: every buffer of this call is allocated
    done = _call_entry(pkg, oracle, p, c, k, entry, S, sync)
    if sync == 0:
        assert done is False, "%s returned only after the producer had finished: it waited on the host" % entry


@pytest.mark.parametrize("sync", [0, 1])
def test_pca_queues_behind_the_callers_stream(pkg, sync):
    """pt_pca_normals_dev the same way, on the attribute reference's surface cloud"""
    import torch
    k = 13
    xyz, nrm = cases.cloud("surface", "f32")
    idx, _ = cases.lists("surface", "f32", k)
    S = torch.cuda.Stream()
    with pkg.PointsTransfer(device=0) as p:
        p.build(xyz, None, nrm)
        real = _dev(idx.view(np.int32))
        for warm in (True, False):
            late = torch.zeros_like(real)
            out = torch.full((cases.M, 3), float("nan"), device="cuda", dtype=torch.float32)
            torch.cuda.synchronize()
            p.set_param("sync", 1 if warm else sync)
            E = _slow_copy(S, [(late, real)])
            with torch.cuda.stream(S):
                p.pca_normals_dev(late, cases.M, k, out)
                done = E.query()
                got = out.clone()
            S.synchronize()
            R.check_pca(got.cpu().numpy(), idx, xyz.astype(np.float64), nrm, "pca on a side stream, sync %d" % sync)
        if sync == 0:
            assert done is False, "pt_pca_normals_dev waited on the host"


def _raw_query(p, x, xt, m, k, i_, d_):
    """pt_query_soa(on_device) without the wrapper's adoption of torch's current stream"""
    p._chk(p._L.pt_query_soa(p._h, C.c_void_p(x.data_ptr()), xt, m, k, 1, C.c_void_p(i_.data_ptr()), C.c_void_p(d_.data_ptr())))


@pytest.mark.parametrize("sync", [0, 1])
@pytest.mark.parametrize("which", ["null_stream", "own_stream"])
def test_null_and_own_stream(pkg, stream_case, which, sync):
    """pt_set_stream(NULL) -- HIP's default stream -- and "own_stream" 1: a _dev query, pt_synchronize, exact lists"""
    import torch
    p, c, k = stream_case
    m = c["tgt"].shape[1]
    x = _dev(c["tgt"])
    i_, d_ = _lists(m, k)
    torch.cuda.synchronize()                                     # (the context's own stream is non-blocking: the inputs must be there)
    if which == "null_stream":
        p.set_stream(0)
    else:
        p.set_param("own_stream", 1)
    p.set_param("sync", sync)
    _raw_query(p, x, pkg.F32, m, k, i_, d_)
    p.synchronize()
    check_exact(_np_lists(i_, d_), (c["idx"][:, :k], c["d2"][:, :k]), "%s sync %d" % (which, sync))


# ---- 4. switching streams with work in flight ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("second", ["set_stream", "own_stream", "set_targets"])
def test_stream_switch_with_work_in_flight(pkg, oracle, stream_case, second):
    """include/pt_api.h at pt_set_stream: under "sync" 0 the context makes the stream it is switched to wait for what it queued on the
    one it leaves.  Stream A is kept busy by a sleep, then given the first call; the second call DEPENDS on the first and goes to
    stream B (set_stream), or to the context's own stream; only that stream is synchronised.
      set_stream / own_stream: query_dev on A into X, blend_dev reading X on the new stream;
      set_targets: set_targets(device tensor) on A, query_resident_dev on B (the resident targets were zeros before)."""
    import torch
    p, c, k = stream_case
    m = c["tgt"].shape[1]
    want = (c["idx"][:, :k].copy(), c["d2"][:, :k].copy())
    sc, sn = _sentinels(m)
    mode = pkg.BLEND_INV_D2
    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    x = _dev(c["tgt"])
    for warm in (True, False):                                   # (warm-up, synchronous: nothing allocates in the round that counts)
        i_, d_ = _lists(m, k)
        c_, n_ = _dev(sc), _dev(sn)
        p.set_param("sync", 1)
        p.set_targets(torch.zeros_like(x), xyz_type=pkg.F32)
        torch.cuda.synchronize()
        p.set_param("sync", 1 if warm else 0)
        with torch.cuda.stream(A):
            torch.cuda._sleep(SLEEP_CYCLES)
            if second == "set_targets":
                p.set_targets(x, xyz_type=pkg.F32)
            else:
                p.query_dev(x, pkg.F32, m, k, i_, d_)
            E = torch.cuda.Event(); E.record(A)
        if second == "own_stream":
            p.set_param("own_stream", 1)
            p._chk(p._L.pt_blend_dev(p._h, C.c_void_p(i_.data_ptr()), C.c_void_p(d_.data_ptr()), m, k, mode, C.c_void_p(c_.data_ptr()), C.c_void_p(n_.data_ptr())))
            pending = not E.query()
            p.synchronize()
        else:
            with torch.cuda.stream(B):
                if second == "set_targets":
                    p.query_resident_dev(k, i_, d_)
                else:
                    p.blend_dev(i_, d_, m, k, mode, c_, n_)
                pending = not E.query()
            B.synchronize()
        assert E.query(), "the new stream was drained but the work queued on the old one is not done"
        what = "switch by %s%s" % (second, " (warm-up)" if warm else "")
        check_exact(_np_lists(i_, d_), want, what)
        if second != "set_targets":
            check_blend(c_.cpu().numpy(), n_.cpu().numpy(), want[0], want[1], c["rgb"], c["nrm"], mode, sc, sn, oracle, what)
    assert pending, "the first call had finished before the second was enqueued: the switch was not tested with work in flight"


def test_back_to_back_enqueues_that_grow_the_scratch(pkg, clouds):
    """a small query, then one with more targets and a larger k on the same stream with no wait between: the second call frees and
    reallocates the scratch buffers the first one's kernels use (hipFree waits for the device).  Both exact after one wait."""
    c = clouds("f32", "uniform")
    m0, k0, m1, k1 = 500, 4, c["tgt"].shape[1], 32
    with pkg.PointsTransfer(device=0, k_hint=16) as p:
        p.build(c["src"])
        p.set_param("sync", 0)
        x0, x1 = _dev(c["tgt"][:, :m0]), _dev(c["tgt"])
        a, b = _lists(m0, k0), _lists(m1, k1)
        p.query_dev(x0, pkg.F32, m0, k0, *a)
        p.query_dev(x1, pkg.F32, m1, k1, *b)
        p.synchronize()
    check_exact(_np_lists(*a), (c["idx"][:m0, :k0], c["d2"][:m0, :k0]), "the small query")
    check_exact(_np_lists(*b), (c["idx"][:, :k1], c["d2"][:, :k1]), "the large query behind it")
