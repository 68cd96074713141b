"""GPU suite for the max-distance cutoff (pt_set_param "max_dist", PointsTransfer(max_dist=...), pointsTransfer --max-dist).

Contract (include/pt_api.h): with the cap r set, every query result equals the uncapped result with each entry of d2 > r*r replaced by
(NOIDX, +inf), bit for bit; blends blend a row over the entries it has and leave a row without any entry as the caller's output held it.
Every expectation here is the oracle's uncapped answer, truncated in Python."""
import math
import os
import subprocess

import numpy as np
import pytest

from _capped import NOIDX, TOL, check_blend, check_exact, truncate  # noqa: F401

pytestmark = pytest.mark.gpu


def sphere_shell(rng, n, cut=True):
    """points on the unit sphere around (0.5, 0.5, 0.5), radius 0.4; cut: without the cap z > 0.5 + 0.2 (a hole for the targets there)"""
    v = rng.standard_normal((3, n * 2))
    v /= np.linalg.norm(v, axis=0)
    if cut:
        v = v[:, v[2] < 0.5]
    v = v[:, :n]
    return (0.5 + 0.4 * v).astype(np.float32)


def make_cloud(oracle, kind, n, m, seed):
    if kind == "uniform":
        return oracle.synth_xyz(seed, 0, n), oracle.synth_xyz(seed, 1, m)
    if kind == "clustered":
        return oracle.synth_xyz(seed, 0, n, dist=1), oracle.synth_xyz(seed, 1, m, dist=1, n_total=n, m_total=m)
    rng = np.random.default_rng(seed)
    return sphere_shell(rng, n, cut=True), sphere_shell(rng, m, cut=False)       # targets on the whole sphere, the cap's included


def radii(d2_full, k):
    """r = 0; small (most lists short or empty); about the median k-th distance; large (every list unchanged)"""
    kth = d2_full[:, k - 1]
    return [0.0, math.sqrt(float(np.quantile(d2_full[:, 0], 0.3))), math.sqrt(float(np.median(kth))), math.sqrt(float(kth.max())) * 1.01]


# ---- 1. exactness grid ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "clustered", "shell"])
@pytest.mark.parametrize("xyz", ["f32", "f64", "f16"])
def test_capped_queries_equal_truncated_oracle(pkg, oracle, kind, xyz):
    import torch
    n, m, seed = 40000, 2500, 0xD1
    src, tgt = make_cloud(oracle, kind, n, m, seed)
    dt = {"f32": np.float32, "f64": np.float64, "f16": np.float16}[xyz]
    xt = {"f32": pkg.F32, "f64": pkg.F64, "f16": pkg.F16}[xyz]
    src = src.astype(dt); tgt = tgt.astype(dt)
    kdev = pkg.F64 if xyz == "f64" else pkg.F32                            # (fp16 targets are widened to fp32 on the device)
    tdev = tgt.astype(np.float64 if xyz == "f64" else np.float32)
    want_all = oracle.knn_bruteforce(src.astype(np.float64), tgt.astype(np.float64), 32)
    with pkg.PointsTransfer(device=0) as p:
        p.build(src)
        p.set_targets(tgt)
        x = torch.from_numpy(np.ascontiguousarray(tdev)).cuda()
        for k in (1, 8, 16, 20, 24, 32):
            wi, wd = want_all[0][:, :k].copy(), want_all[1][:, :k].copy()
            for r in radii(wd, k):
                p.max_dist = r
                want = truncate(wi, wd, r)
                tag = "%s %s k=%d r=%.6g" % (kind, xyz, k, r)
                check_exact(p.query(tgt, k), want, tag + " query_soa (host)")
                i_ = torch.empty((m, k), dtype=torch.int32, device="cuda"); d_ = torch.empty((m, k), dtype=torch.float64, device="cuda")
                p.query_dev(x, kdev, m, k, i_, d_)
                check_exact((i_.cpu().numpy().view(np.uint32), d_.cpu().numpy()), want, tag + " query_soa (device)")
                p.query_resident_dev(k, i_, d_)
                check_exact((i_.cpu().numpy().view(np.uint32), d_.cpu().numpy()), want, tag + " resident")
                # per-target bounds above and below R2: each target gets min(bound2[t], R2)
                R2 = r * r
                b = np.where(np.arange(m) % 2 == 0, R2 * 4.0 + 1e-9, R2 * 0.25).astype(np.float64)
                b[::7] = wd[::7, k - 1]                                    # (some at the target's own uncapped k-th distance)
                p.query_bounded_dev(x, kdev, torch.from_numpy(b).cuda(), m, k, i_, d_)
                eff = np.minimum(b, R2)
                bi, bd = wi.copy(), wd.copy()
                far = bd > eff[:, None]
                bi[far] = NOIDX; bd[far] = np.inf
                check_exact((i_.cpu().numpy().view(np.uint32), d_.cpu().numpy()), (bi, bd), tag + " bounded_dev")
            if xyz == "f64" and k in (8, 20):                               # AoS records (the CLI's query) are fp64
                from _bake_cases import point_records
                rec = point_records(pkg.POINT_DTYPE, tgt.astype(np.float64), np.zeros((m, 3), np.uint8))
                for r in radii(wd, k)[1:3]:
                    p.max_dist = r
                    check_exact(p.query_aos(rec, k), truncate(wi, wd, r), "%s k=%d r=%.6g query_aos" % (kind, k, r))
        # the largest radius gave the uncapped lists back, bit for bit
        p.max_dist = None
        check_exact(p.query(tgt, 32), want_all, kind + " uncapped")


# ---- 2. the boundary is inclusive ----------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1.0, 2.0])
def test_boundary_points_at_exactly_r_are_in(pkg, oracle, r):
    g = np.arange(12, dtype=np.float32)
    src = np.stack(np.meshgrid(g, g, g, indexing="ij")).reshape(3, -1).astype(np.float32)
    rng = np.random.default_rng(3)
    tgt = src[:, rng.choice(src.shape[1], 400, replace=False)].copy()
    tgt[:, ::2] += np.float32(0.5)                                         # half of them between lattice points
    k = 32
    wi, wd = oracle.knn_bruteforce(src, tgt, k)
    R2 = r * r
    assert (wd == R2).sum() > 100, "the case must put points at exactly r"
    with pkg.PointsTransfer(device=0) as p:
        p.build(src)
        p.max_dist = r
        gi, gd = p.query(tgt, k)
        check_exact((gi, gd), truncate(wi, wd, r), "r = %g" % r)
        assert (gd == R2).sum() == (wd == R2).sum()                        # d2 == R2: in reach
        below = float(np.nextafter(r, 0.0))
        p.max_dist = below
        gi, gd = p.query(tgt, k)
        check_exact((gi, gd), truncate(wi, wd, below), "r = nextafter(%g, 0)" % r)
        assert not (gd == R2).any()                                        # ... and out of it just below


# ---- 3. the tile kernel answers capped fused queries ------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 20])
def test_tile_kernel_answers_capped_fused_queries(pkg, oracle, k):
    import torch
    n, m, seed = 2_000_000, 200_000, 0xD3
    src, tgt = oracle.synth_xyz(seed, 0, n), oracle.synth_xyz(seed, 1, m)
    rgb, nrm = oracle.synth_rgb(seed, n), oracle.synth_nrm(seed, n)
    wi, wd = oracle.KdTree(src).query(tgt, k)
    r = 1.5 * math.sqrt(float(np.median(wd[:, k - 1])))                  # beyond most k-th distances: ring 1 settles most targets
    want = truncate(wi, wd, r)
    leftover = {}
    with pkg.PointsTransfer(device=0, k_hint=k) as p:
        p.set_param("sync", 1)
        p.build(src, rgb, nrm)
        p.set_targets(tgt)
        for cap in (None, r):
            p.max_dist = cap
            i_ = torch.empty((m, k), dtype=torch.int32, device="cuda"); d_ = torch.empty((m, k), dtype=torch.float64, device="cuda")
            c_ = torch.full((m, 3), float("nan"), dtype=torch.float32, device="cuda"); n_ = torch.full((m, 3), float("nan"), dtype=torch.float32, device="cuda")
            p.query_blend_resident_dev(k, pkg.BLEND_MEAN, i_, d_, c_, n_)
            torch.cuda.synchronize()
            leftover[cap] = p.stats()["n_leftover"]
            gi, gd = i_.cpu().numpy().view(np.uint32), d_.cpu().numpy()
            check_exact((gi, gd), want if cap else (wi, wd), "k=%d cap=%s" % (k, cap))
            sent = np.full((m, 3), np.nan, np.float32)
            check_blend(c_.cpu().numpy(), n_.cpu().numpy(), gi, gd, rgb, nrm, 0, sent, sent, oracle, "fused k=%d" % k)
    assert leftover[r] < 0.05 * m and leftover[None] < 0.05 * m, leftover


# ---- 4. fused blend and the blends of capped lists --------------------------------------------------------------------
@pytest.mark.parametrize("k,mode,wave", [(8, 0, 0), (16, 1, 0), (20, 0, 1), (32, 1, 0)])
def test_capped_blends_leave_empty_rows_alone(pkg, oracle, k, mode, wave):
    import torch
    n, m, seed = 150000, 8000, 0xD4
    src, tgt = oracle.synth_xyz(seed, 0, n), oracle.synth_xyz(seed, 1, m)
    tgt[:, : m // 8] = (tgt[:, : m // 8] * 0.2 + 1.3).astype(np.float32)     # an eighth of the targets well outside the cloud's box
    rgb, nrm = oracle.synth_rgb(seed, n), oracle.synth_nrm(seed, n)
    wi, wd = oracle.knn_bruteforce(src, tgt, k)
    r = math.sqrt(float(np.median(wd[m // 8:, k - 1])))
    ti, td = truncate(wi, wd, r)
    assert (ti[: m // 8] == NOIDX).all() and (ti[m // 8:] != NOIDX).any()
    rng = np.random.default_rng(4)
    sc = rng.random((m, 3)).astype(np.float32) * 100; sn = rng.random((m, 3)).astype(np.float32)
    with pkg.PointsTransfer(device=0, k_hint=k, max_dist=r) as p:
        if wave:
            p.set_param("wave_force", 1); p.set_param("tile", 0)
        p.build(src, rgb, nrm)
        p.set_targets(tgt)
        i_ = torch.empty((m, k), dtype=torch.int32, device="cuda"); d_ = torch.empty((m, k), dtype=torch.float64, device="cuda")
        c_ = torch.from_numpy(sc.copy()).cuda(); n_ = torch.from_numpy(sn.copy()).cuda()
        p.query_blend_resident_dev(k, mode, i_, d_, c_, n_)
        gi, gd = i_.cpu().numpy().view(np.uint32), d_.cpu().numpy()
        check_exact((gi, gd), (ti, td), "fused")
        e = check_blend(c_.cpu().numpy(), n_.cpu().numpy(), ti, td, rgb, nrm, mode, sc, sn, oracle, "fused blend")
        assert e >= m // 8
        # blend_dev of the capped lists
        c_ = torch.from_numpy(sc.copy()).cuda(); n_ = torch.from_numpy(sn.copy()).cuda()
        p.blend_dev(i_, d_, m, k, mode, c_, n_)
        check_blend(c_.cpu().numpy(), n_.cpu().numpy(), ti, td, rgb, nrm, mode, sc, sn, oracle, "blend_dev")
        # host blend, caller's arrays and the default zeros
        oc, on = sc.copy(), sn.copy()
        p.blend(ti, td, mode=mode, rgb_out=oc, nrm_out=on)
        check_blend(oc, on, ti, td, rgb, nrm, mode, sc, sn, oracle, "blend (host)")
        zc, zn = p.blend(ti, td, mode=mode)
        z = np.zeros((m, 3), np.float32)
        check_blend(zc, zn, ti, td, rgb, nrm, mode, z, z, oracle, "blend (host, default outputs)")
        # the host round trip of the resident query keeps the caller's values of empty rows too
        hi, hd = np.empty((m, k), np.uint32), np.empty((m, k))
        oc, on = sc.copy(), sn.copy()
        p._chk(p._L.pt_query_resident_host(p._h, k, mode, hi.ctypes.data, hd.ctypes.data, oc.ctypes.data, on.ctypes.data))
        check_exact((hi, hd), (ti, td), "resident_host")
        check_blend(oc, on, ti, td, rgb, nrm, mode, sc, sn, oracle, "resident_host blend")


# ---- 5. streamed source ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 20])
def test_stream_query_with_cap(pkg, oracle, k):
    import torch
    n, m, seed = 400000, 20000, 0xD5
    src, tgt = oracle.synth_xyz(seed, 0, n), oracle.synth_xyz(seed, 1, m)
    order = np.argsort(src[0], kind="stable")
    src_x = np.ascontiguousarray(src[:, order])                            # sorted along x: eight chunks are eight slabs
    wi, wd = oracle.knn_bruteforce(src_x, tgt, k)
    r = 0.8 * math.sqrt(float(np.median(wd[:, k - 1])))
    want = truncate(wi, wd, r)
    with pkg.PointsTransfer(device=0, k_hint=k) as p:
        p.set_targets(tgt)
        gi, gd = p.stream_query(src_x, n // 8, k)
        unc = p.stats()
        assert np.array_equal(gi.astype(np.uint32), wi) and np.array_equal(gd, wd)
        p.max_dist = r
        gi, gd = p.stream_query(src_x, n // 8, k)
        cap = p.stats()
        check_exact((np.where(gi == np.uint64(2**64 - 1), NOIDX, gi).astype(np.uint32), gd), want, "stream, capped")
        assert cap["stream_revisited"] == 0
        assert cap["stream_skipped"] >= unc["stream_skipped"]
        # bit-identical to the capped resident query of the same cloud
        p.build(src_x)
        p.set_targets(tgt)
        i_ = torch.empty((m, k), dtype=torch.int32, device="cuda"); d_ = torch.empty((m, k), dtype=torch.float64, device="cuda")
        p.query_resident_dev(k, i_, d_)
        ri = i_.cpu().numpy().view(np.uint32)
        assert np.array_equal(np.where(gi == np.uint64(2**64 - 1), NOIDX, gi).astype(np.uint32), ri) and np.array_equal(gd, d_.cpu().numpy())


# ---- 6. slab exchange ------------------------------------------------------------------------------------------------------------
def _exchange(pkg, oracle, src, tgt, rgb, nrm, g, k, r, sharded, bounds=None):
    """G contexts of one process (pt_exchange_merge_local): home search + blend, exchange, re-blend; returns merged lists and blends"""
    import torch
    m = tgt.shape[1]
    if bounds is None:
        bounds = [-math.inf] + [float(v) for v in np.quantile(src[0], np.arange(1, g) / g)] + [math.inf]
    home = np.clip(np.searchsorted(np.array(bounds), tgt[0], side="right") - 1, 0, g - 1)
    pts, xs, ii, dd, cc, nn, rows = [], [], [], [], [], [], []
    sc = np.full((m, 3), -7.0, np.float32)
    for s in range(g):
        p = pkg.PointsTransfer(device=0, k_hint=k, max_dist=r)
        sel = np.nonzero((src[0] >= bounds[s]) & (src[0] < bounds[s + 1]))[0]
        if sharded:
            p.set_param("local_ids", 1)
        p.build(np.ascontiguousarray(src[:, sel]), gidx=sel.astype(np.uint32))
        if sharded:
            p.set_attributes_local(rgb[sel], nrm[sel])
        else:
            p.set_attributes(rgb, nrm)
        mine = np.nonzero(home == s)[0]
        ms = len(mine)
        x = torch.from_numpy(np.ascontiguousarray(tgt[:, mine])).cuda()
        i_ = torch.empty((ms, k), dtype=torch.int32, device="cuda"); d_ = torch.empty((ms, k), dtype=torch.float64, device="cuda")
        c_ = torch.from_numpy(sc[mine].copy()).cuda(); n_ = torch.from_numpy(sc[mine].copy()).cuda()
        if ms:
            p.query_dev(x, pkg.F32, ms, k, i_, d_)
            p.blend_dev(i_, d_, ms, k, pkg.BLEND_MEAN, c_, n_)
        pts.append(p); xs.append(x); ii.append(i_); dd.append(d_); cc.append(c_); nn.append(n_); rows.append(mine)
    pkg.PointsTransfer.exchange_merge_local(pts, xs, pkg.F32, k, 0, bounds, ii, dd, pkg.BLEND_MEAN, cc, nn)
    torch.cuda.synchronize()
    gi = np.empty((m, k), np.uint32); gd = np.empty((m, k)); gc = np.empty((m, 3), np.float32); gn = np.empty((m, 3), np.float32)
    for s in range(g):
        gi[rows[s]] = ii[s].cpu().numpy().view(np.uint32); gd[rows[s]] = dd[s].cpu().numpy()
        gc[rows[s]] = cc[s].cpu().numpy(); gn[rows[s]] = nn[s].cpu().numpy()
    for p in pts:
        p.close()
    return gi, gd, gc, gn, sc


@pytest.mark.parametrize("g,k,sharded", [(2, 8, False), (3, 20, True), (8, 8, True), (8, 20, False), (3, 16, False), (2, 32, True)])
def test_exchange_with_cap_equals_single_context(pkg, oracle, g, k, sharded):
    n, m, seed = 150000, 9000, 0xD6 + g
    src, tgt = oracle.synth_xyz(seed, 0, n), oracle.synth_xyz(seed, 1, m)
    tgt[:, :300] = (tgt[:, :300] * 0.1 + 1.2).astype(np.float32)          # some rows with nothing in reach
    rgb, nrm = oracle.synth_rgb(seed, n), oracle.synth_nrm(seed, n)
    wi, wd = oracle.KdTree(src).query(tgt, k)
    r = math.sqrt(float(np.median(wd[300:, k - 1])))
    ti, td = truncate(wi, wd, r)
    gi, gd, gc, gn, sc = _exchange(pkg, oracle, src, tgt, rgb, nrm, g, k, r, sharded)
    check_exact((gi, gd), (ti, td), "exchange g=%d" % g)
    check_blend(gc, gn, ti, td, rgb, nrm, 0, sc, sc, oracle, "exchange re-blend g=%d" % g)


def test_exchange_band_no_crossing_and_mismatched_caps(pkg, oracle):
    import torch
    rng = np.random.default_rng(61)
    n, m, k = 20000, 6000, 8                                              # sparse: k-th distances near the band reach across it
    src = rng.random((3, n)).astype(np.float32)
    band = 0.05
    src = src[:, (np.abs(src[0] - 0.5) > band)]                           # an empty band of width 0.1 around the slab boundary x = 0.5
    tgt = rng.random((3, m)).astype(np.float32)
    tgt = tgt[:, (np.abs(tgt[0] - 0.5) > band)]
    m = tgt.shape[1]
    wi, wd = oracle.knn_bruteforce(src, tgt, k)
    r = 0.9 * band                                                         # 2r < the band's width
    bounds = [-math.inf, 0.5, math.inf]
    x = torch.from_numpy(tgt).cuda()
    h0 = np.nonzero(tgt[0] < 0.5)[0]                                         # slab 0's home targets
    mh = len(h0)
    xh = torch.from_numpy(np.ascontiguousarray(tgt[:, h0])).cuda()
    counts = {}
    for cap in (None, r):
        with pkg.PointsTransfer(device=0, max_dist=cap) as p:
            sel = np.nonzero(src[0] < 0.5)[0]
            p.build(np.ascontiguousarray(src[:, sel]), gidx=sel.astype(np.uint32))
            i_ = torch.empty((mh, k), dtype=torch.int32, device="cuda"); d_ = torch.empty((mh, k), dtype=torch.float64, device="cuda")
            p.query_dev(xh, pkg.F32, mh, k, i_, d_)
            sel_ = torch.empty(mh, dtype=torch.int32, device="cuda"); pkt = torch.empty((mh, 5), dtype=torch.float64, device="cuda")
            counts[cap] = p.pack_requests_dev(xh, pkg.F32, d_, mh, k, 0, bounds, 0, sel_, pkt)
    assert counts[r] == 0 and counts[None] > 0, counts
    # the merged lists of the capped exchange still equal the capped single-context search
    rgb, nrm = np.zeros((src.shape[1], 3), np.uint8), np.zeros((src.shape[1], 3), np.float32)
    gi, gd, _, _, _ = _exchange(pkg, oracle, src, tgt, rgb, nrm, 2, k, r, False, bounds)
    check_exact((gi, gd), truncate(wi, wd, r), "band")
    # contexts that disagree on the cap are refused
    ps = [pkg.PointsTransfer(device=0, max_dist=r), pkg.PointsTransfer(device=0, max_dist=2 * r)]
    xs, ii, dd = [], [], []
    for s, p in enumerate(ps):
        sel = np.nonzero((src[0] >= bounds[s]) & (src[0] < bounds[s + 1]))[0]
        p.build(np.ascontiguousarray(src[:, sel]), gidx=sel.astype(np.uint32))
        xs.append(x[:, :10].contiguous()); ii.append(torch.empty((10, k), dtype=torch.int32, device="cuda")); dd.append(torch.empty((10, k), dtype=torch.float64, device="cuda"))
        p.query_dev(xs[-1], pkg.F32, 10, k, ii[-1], dd[-1])
    with pytest.raises(pkg.PtError) as e:
        pkg.PointsTransfer.exchange_merge_local(ps, xs, pkg.F32, k, 0, bounds, ii, dd)
    assert e.value.code == pkg.capi.ERR_ARG
    for p in ps:
        p.close()


@pytest.mark.parametrize("g,k", [(4, 8), (6, 20)])
def test_slab_need_and_requests_reach_min_kth_cap(pkg, oracle, g, k):
    import torch
    n, m, seed = 100000, 5000, 0xD8
    src, tgt = oracle.synth_xyz(seed, 0, n), oracle.synth_xyz(seed, 1, m)
    bounds = [-math.inf] + [float(v) for v in np.quantile(src[0], np.arange(1, g) / g)] + [math.inf]
    my = 1
    sel = np.nonzero((src[0] >= bounds[my]) & (src[0] < bounds[my + 1]))[0]
    wi, wd = oracle.knn_bruteforce(src[:, sel], tgt, k, gidx=sel)
    r = math.sqrt(float(np.median(wd[:, k - 1]))) * 0.7
    with pkg.PointsTransfer(device=0, max_dist=r) as p:
        p.build(np.ascontiguousarray(src[:, sel]), gidx=sel.astype(np.uint32))
        x = torch.from_numpy(tgt).cuda()
        i_ = torch.empty((m, k), dtype=torch.int32, device="cuda"); d_ = torch.empty((m, k), dtype=torch.float64, device="cuda")
        p.query_dev(x, pkg.F32, m, k, i_, d_)
        d2 = d_.cpu().numpy()
        check_exact((i_.cpu().numpy().view(np.uint32), d2), truncate(wi, wd, r), "slab query")
        need = torch.empty((g, m), dtype=torch.uint8, device="cuda")
        p.slab_need_dev(x, pkg.F32, d_, m, k, 0, bounds, my, need)
        sel_ = torch.empty(m, dtype=torch.int32, device="cuda"); pkt = torch.empty((m, 5), dtype=torch.float64, device="cuda")
        c = p.pack_requests_dev(x, pkg.F32, d_, m, k, 0, bounds, my, sel_, pkt)
    reach = np.minimum(d2[:, k - 1], r * r)                                 # numpy restatement
    cx = tgt[0].astype(np.float64)
    want = np.zeros((g, m), np.uint8)
    for s in range(g):
        if s == my:
            continue
        lo, hi = bounds[s], bounds[s + 1]
        gap = np.where(cx < lo, lo - cx, np.where(cx >= hi, cx - hi, 0.0))
        want[s] = (gap * gap * (1.0 - 1e-12) <= reach)
    assert np.array_equal(need.cpu().numpy(), want)
    rows = np.nonzero(want.any(axis=0))[0]
    assert c == len(rows)
    got_rows = sel_[:c].cpu().numpy()
    o = np.argsort(got_rows)
    pk = pkt[:c].cpu().numpy()[o]
    assert np.array_equal(got_rows[o], rows)
    assert np.array_equal(pk[:, 3], reach[rows])                             # the packets carry the capped reach as their bound
    masks = (want[:, rows].astype(np.uint64) << np.arange(g, dtype=np.uint64)[:, None]).sum(axis=0)
    assert np.array_equal(pk[:, 4].astype(np.uint64), masks)


# ---- 7. texture bake from capped lists -----------------------------------------------------------------------------------------
def test_bake_texture_from_capped_lists(pkg, oracle):
    from _bake_cases import make_case, point_records
    src, rgb, verts, uv, vrgb, faces = make_case(17, n=6000, grid=6)
    k, R = 20, 256
    keep = ~((np.abs(src[0] - 0.5) < 0.2) & (np.abs(src[1] - 0.5) < 0.2))   # a hole in the middle of the cloud
    src, rgb = np.ascontiguousarray(src[:, keep]), np.ascontiguousarray(rgb[keep])
    src32 = src.astype(np.float32)
    wi, wd = oracle.knn_bruteforce(src32, verts.astype(np.float32), k)
    r = math.sqrt(float(np.median(wd[:, k - 1])))
    ti, td = truncate(wi, wd, r)
    assert (ti == NOIDX).all(axis=1).any()
    with pkg.PointsTransfer(device=0, k_hint=k, max_dist=r) as p:
        p.build(src32, rgb, np.zeros((src.shape[1], 3), np.float32))
        idx, d2 = p.query(verts.astype(np.float32), k)
        check_exact((idx, d2), (ti, td), "bake lists")
        vrec = point_records(pkg.POINT_DTYPE, verts.astype(np.float32).astype(np.float64), vrgb, uv)
        got = p.bake_texture(vrec, faces, idx, R)
        want = oracle.bake_texture(src32.astype(np.float64), rgb, verts.astype(np.float32).astype(np.float64), uv, vrgb, faces, ti, R)
        assert np.array_equal(got, want)


# ---- 8. parameter handling ---------------------------------------------------------------------------------------------------
def test_max_dist_parameter_handling(pkg, oracle):
    import torch
    n, m, k, seed = 100000, 4000, 8, 0xD9
    src, tgt = oracle.synth_xyz(seed, 0, n), oracle.synth_xyz(seed, 1, m)
    rgb, nrm = oracle.synth_rgb(seed, n), oracle.synth_nrm(seed, n)
    with pkg.PointsTransfer(device=0) as p:
        for bad in (float("nan"), -1.0, -1e-300, -math.inf):
            with pytest.raises(pkg.PtError) as e:
                p.set_param("max_dist", bad)
            assert e.value.code == pkg.capi.ERR_ARG
        assert p.max_dist is None
        p.set_param("max_dist", 0.0)
        p.set_param("max_dist", math.inf)
    # +inf after a cap: the same results as a context that never had one, blend outputs included
    outs = []
    for history in ((), (0.01, math.inf)):
        with pkg.PointsTransfer(device=0, k_hint=k) as p:
            p.set_param("sync", 1)
            p.build(src, rgb, nrm)
            p.set_targets(tgt)
            for r in history:
                p.set_param("max_dist", r)
                p.query(tgt, k)
            i_ = torch.empty((m, k), dtype=torch.int32, device="cuda"); d_ = torch.empty((m, k), dtype=torch.float64, device="cuda")
            c_ = torch.full((m, 3), float("nan"), device="cuda"); n_ = torch.full((m, 3), float("nan"), device="cuda")
            p.query_blend_resident_dev(k, pkg.BLEND_MEAN, i_, d_, c_, n_)
            few = np.full((m, k), NOIDX, np.uint32); few[:, 0] = np.arange(m) % n
            few[::3] = NOIDX                                              # empty rows: written with zeros uncapped
            bc, bn = p.blend(few, np.ones((m, k)), rgb_out=np.full((m, 3), np.nan, np.float32), nrm_out=np.full((m, 3), np.nan, np.float32))
            outs.append([t.cpu().numpy() for t in (i_, d_, c_, n_)] + [bc, bn])
    for a, b in zip(*outs):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert (outs[0][4][::3] == 0).all()
    # changing the cap needs no rebuild and leaves what the context learned for its next build as it was
    sorts = []
    for change in (False, True):
        with pkg.PointsTransfer(device=0, k_hint=k) as p:
            p.set_param("sync", 1)
            p.build(src)
            i0, d0 = p.query(tgt, k)
            if change:
                r = math.sqrt(float(np.median(d0[:, k - 1])))
                p.max_dist = r
                check_exact(p.query(tgt, k), truncate(i0, d0, r), "cap set after the build")
                p.max_dist = r * 0.5
                check_exact(p.query(tgt, k), truncate(i0, d0, r * 0.5), "cap changed")
                p.max_dist = None
            p.rebuild()
            sorts.append(p.stats()["n_sorts"])
            check_exact(p.query(tgt, k), (i0, d0), "after the rebuild")
    assert sorts[0] == sorts[1], sorts


# ---- 9. CLI --------------------------------------------------------------------------------------------------------------------------
def _hole_case():
    from _bake_cases import make_case
    src, rgb, verts, uv, vrgb, faces = make_case(23, n=9000, grid=8)
    keep = ~((np.abs(src[0] - 0.5) < 0.22) & (np.abs(src[1] - 0.45) < 0.22))  # a scan hole the mesh spans
    return np.ascontiguousarray(src[:, keep]), np.ascontiguousarray(rgb[keep]), verts, uv, vrgb, faces


def _write_plys(pc, mesh, src, rgb, verts, uv, vrgb, vnrm, faces, binary):
    n, m = src.shape[1], verts.shape[1]
    if binary:
        cd = np.dtype([("p", "<f8", 3), ("n", "<f4", 3), ("c", "u1", 3)])
        a = np.zeros(n, cd); a["p"] = src.T; a["n"] = (0, 0, 1); a["c"] = rgb
        with open(pc, "wb") as f:
            f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty double x\nproperty double y\nproperty double z\n"
                     "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % n).encode())
            f.write(a.tobytes())
        md = np.dtype([("p", "<f8", 3), ("n", "<f8", 3), ("uv", "<f8", 2), ("c", "<i4", 3)])
        b = np.zeros(m, md); b["p"] = verts.T; b["n"] = vnrm; b["uv"] = uv; b["c"] = vrgb
        fd = np.dtype([("k", "u1"), ("v", "<i4", 3)])
        fc = np.zeros(len(faces), fd); fc["k"] = 3; fc["v"] = faces
        with open(mesh, "wb") as f:
            f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty double x\nproperty double y\nproperty double z\n"
                     "property double nx\nproperty double ny\nproperty double nz\nproperty double s\nproperty double t\nproperty int red\n"
                     "property int green\nproperty int blue\nelement face %d\nproperty list uchar int vertex_indices\nend_header\n" % (m, len(faces))).encode())
            f.write(b.tobytes()); f.write(fc.tobytes())
        return
    with open(pc, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\n"
                "property float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % n)
        for i in range(n):
            f.write("%.17g %.17g %.17g 0 0 1 %d %d %d\n" % (*src[:, i], *rgb[i]))
    with open(mesh, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\n"
                "property float ny\nproperty float nz\nproperty float s\nproperty float t\nproperty uchar red\nproperty uchar green\n"
                "property uchar blue\nelement face %d\nproperty list uchar int vertex_indices\nend_header\n" % (m, len(faces)))
        for i in range(m):
            f.write("%.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %d %d %d\n" % (*verts[:, i], *vnrm[i], *uv[i], *vrgb[i]))
        for fc in faces:
            f.write("3 %d %d %d\n" % tuple(fc))


def _read_png_rgba(path):
    import struct, zlib
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    off, idat, w, h = 8, [], 0, 0
    while off < len(data):
        ln, typ = struct.unpack(">I4s", data[off:off + 8])
        body = data[off + 8:off + 8 + ln]
        if typ == b"IHDR":
            w, h = struct.unpack(">II", body[:8])
        elif typ == b"IDAT":
            idat.append(body)
        off += 12 + ln
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8).reshape(h, w * 4 + 1)
    return raw[:, 1:].reshape(h, w, 4)


@pytest.mark.parametrize("fmt,gpus", [("ascii", 0), ("binary", 0), ("binary", 2)])
def test_cli_max_dist(tmp_path, pkg, oracle, fmt, gpus):
    import json
    import torch
    if gpus and torch.cuda.device_count() < gpus:
        pytest.skip("needs >= %d GPUs: this box shows %d" % (gpus, torch.cuda.device_count()))
    src, rgb, verts, uv, vrgb, faces = _hole_case()
    m, k, R = verts.shape[1], 8, 256
    rng = np.random.default_rng(5)
    vnrm = rng.standard_normal((m, 3)).round(3)
    pc, mesh = tmp_path / "cloud.ply", tmp_path / "mesh.ply"
    _write_plys(pc, mesh, src, rgb, verts, uv, vrgb, vnrm, faces, fmt == "binary")
    wi, wd = oracle.knn_bruteforce(src, verts, k)
    r = 0.06
    ti, td = truncate(wi, wd, r)
    empty = (ti == NOIDX).all(axis=1)
    assert 0 < empty.sum() < m // 2
    exe = os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "pointsTransfer")
    cmd = [exe, str(pc), str(mesh), "--k", str(k), "--resolution", str(R), "--max-dist", repr(r), "--out", str(tmp_path / "out.ply"), "--json", str(tmp_path / "run.json")]
    if gpus:
        cmd += ["--gpus", str(gpus)]
    else:
        cmd += ["--neighbors", str(tmp_path / "nb.bin")]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp_path, timeout=600)
    assert res.returncode == 0, res.stderr
    assert "%d of %d vertices have no point within" % (empty.sum(), m) in res.stderr
    lines = [l.split(":")[0] for l in res.stdout.strip().splitlines()]
    assert lines[-2:] == ["VIRT", "RES"] and "Neighbor search total time" in lines     # the reference's lines, nothing added
    if not gpus:
        got = np.fromfile(tmp_path / "nb.bin", dtype=np.uint32).reshape(m, k)
        assert np.array_equal(got, ti)
        rep = json.load(open(tmp_path / "run.json"))
        assert abs(rep["max_dist"] - r) <= 1e-8 * r and rep["vertices_without_neighbours"] == empty.sum()
    out = [l.split() for l in open(tmp_path / "out.ply").read().split("end_header\n")[1].strip().splitlines()][:m]
    col = np.array([[int(v) for v in row[8:11]] for row in out])
    nrm_out = np.array([[float(v) for v in row[3:6]] for row in out])
    # vertices over the hole: their own colour and normal, exactly (as float32)
    assert np.array_equal(col[empty], vrgb[empty].astype(int))
    assert np.array_equal(nrm_out[empty].astype(np.float32), vnrm[empty].astype(np.float32))
    rc, rn = oracle.blend(ti, td, rgb, np.tile(np.float32([0, 0, 1]), (src.shape[1], 1)), 0)
    assert np.abs(col[~empty] - np.floor(rc[~empty])).max() <= 1
    assert np.abs(nrm_out[~empty] - rn[~empty]).max() <= 1e-5
    png = _read_png_rgba(tmp_path / "texture.png")
    want = oracle.dilate_pad(oracle.bake_texture(src, rgb, verts, uv, vrgb, faces, ti, R), 25)
    assert np.array_equal(png[:, :, [2, 1, 0, 3]], want)


@pytest.mark.parametrize("bad", ["-1", "nan", "x", ""])
def test_cli_rejects_invalid_max_dist(tmp_path, pkg, bad):
    exe = os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "pointsTransfer")
    r = subprocess.run([exe, "a.ply", "b.ply", "--max-dist", bad], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 2 and "--max-dist" in r.stderr


def test_cli_synthetic_with_cap(tmp_path, pkg, oracle):
    import json
    exe = os.path.join(os.path.dirname(pkg.capi.LIB_PATH), "pointsTransfer")
    n, m, k, seed = 20000, 2000, 8, 0xC2
    src, tgt = oracle.synth_xyz(seed, 0, n), oracle.synth_xyz(seed, 1, m)
    wi, wd = oracle.knn_bruteforce(src, tgt, k)
    r = math.sqrt(float(np.quantile(wd[:, 0], 0.4)))
    ti, _ = truncate(wi, wd, r)
    e = int((ti == NOIDX).all(axis=1).sum())
    nb, js = tmp_path / "nb.bin", tmp_path / "s.json"
    res = subprocess.run([exe, "-", "-", "--synthetic", str(n), str(m), hex(seed), "--k", str(k), "--max-dist", repr(r), "--neighbors", str(nb), "--json", str(js)],
                         capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert res.returncode == 0, res.stderr
    assert np.array_equal(np.fromfile(nb, dtype=np.uint32).reshape(m, k), ti)
    rep = json.load(open(js))
    assert abs(rep["max_dist"] - r) <= 1e-8 * r and rep["vertices_without_neighbours"] == e
    assert "%d of %d vertices have no point within" % (e, m) in res.stderr


# ---- 10. one large case ------------------------------------------------------------------------------------------------------------
def test_full_size_capped_fused_query(pkg, oracle):
    """100 M / 10 M uniform fp32, k = 20, r about the median k-th distance, fused query; sub-boxes checked against brute force."""
    import torch
    n, m, k, seed = 100_000_000, 10_000_000, 20, 0xC4
    r = 0.62 * (k / n) ** (1.0 / 3.0)                                      # ~ the median k-th distance of a uniform unit cube
    with pkg.PointsTransfer(device=0, k_hint=k, max_dist=r) as p:
        p.build_synth(n, seed)
        p.targets_synth(m, seed)
        idx = torch.empty((m, k), dtype=torch.int32, device="cuda"); d2 = torch.empty((m, k), dtype=torch.float64, device="cuda")
        rgb = torch.full((m, 3), float("nan"), device="cuda"); nrm = torch.full((m, 3), float("nan"), device="cuda")
        p.query_blend_resident_dev(k, pkg.BLEND_MEAN, idx, d2, rgb, nrm)
        torch.cuda.synchronize()
        gi = idx.cpu().numpy().view(np.uint32); gd = d2.cpu().numpy()
        frac_full = float((gi[:, k - 1] != NOIDX).mean())
        assert 0.2 < frac_full < 0.8, frac_full                            # the cap does cut lists here
        ids_t = torch.empty(m, dtype=torch.int32, device="cuda")
        p.resident_target_ids_dev(ids_t)
        assert np.array_equal(ids_t.cpu().numpy().view(np.uint32), np.arange(m, dtype=np.uint32))     # row t = generated target t
    # sub-boxes: targets well inside, sources of the box grown by r
    rng = np.random.default_rng(9)
    for b in range(3):
        c = rng.random(3) * 0.8 + 0.1
        ilo, ihi = (c - 0.004).astype(np.float32)[None], (c + 0.004).astype(np.float32)[None]
        olo, ohi = (c - 0.004 - 2 * r).astype(np.float32)[None], (c + 0.004 + 2 * r).astype(np.float32)[None]
        sxyz, sidx, _ = oracle.synth_filter_boxes(seed, 0, n, olo, ohi)
        txyz, tidx, _ = oracle.synth_filter_boxes(seed, 1, m, ilo, ihi)
        wi, wd = oracle.knn_bruteforce(sxyz, txyz, k, gidx=sidx)
        want = truncate(wi, wd, r)
        check_exact((gi[tidx], gd[tidx]), want, "sub-box %d" % b)
