"""GPU matrix of the LDS tile kernel: every compiled instantiation (one row of tests/_tile_variants.py each) is made to answer a query,
pt_stats proves which instantiation did (tile_variant, and the retry launch of the two-per-CU geometries), and its lists equal the fp64
oracle's bit for bit -- under the cap, the oracle's lists truncated at d2 <= r*r; streamed, the oracle's lists of the whole cloud.
Fused rows blend within 1e-5 of the oracle's blend and, capped, leave a row without a neighbour as the caller's outputs held it.

The clouds carry what ranks go wrong on: exact duplicates (ties at every rank, the k-th included), targets on source points (d2 = 0),
targets outside the bounding box, a dense clump that overflows the small regions (the retry launch), a copy far from the origin where
fp32 spacing makes exact ties common, and pairs of source points whose fp32 roundings coincide while their fp64 values differ (only the
exact pass 3 of an fp64 cloud orders them).  The capped rows also run an integer lattice with r = 1 and 2 -- candidates at d2 = r*r
exactly must be in -- and r just below."""
import math

import numpy as np
import pytest

import _tile_variants as TV
from _capped import NOIDX, check_blend, check_exact, truncate

pytestmark = pytest.mark.gpu

N, M, KMAX = 150_000, 5000, 32
CLUMP, CLUMP_TGT = 800, 40
N_STREAM, STREAM_CHUNKS = 120_001, 3
LATTICE = 36
U64_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def _make_cloud(dtype, scenario, n=N, m=M):
    """planar (3, n) sources and (3, m) targets of `dtype`: "uniform" (unit cube), "clumped" (the same with a dense clump), "far" (the
    unit cube 65536 away from the origin), "stream" (duplicates across the borders of the stream's chunks)"""
    rng = np.random.default_rng({"uniform": 0x7A1, "far": 0x7A2, "stream": 0x7A3, "clumped": 0x7A5}[scenario])
    off = 65536.0 if scenario == "far" else 0.0
    centre = np.array([[0.3], [0.6], [0.4]])
    src = rng.random((3, n))
    clump = scenario == "clumped"
    if clump:                                                   # a dense clump: regions over the small budgets at k <= 8, under the large one
        src[:, :CLUMP] = centre + 0.03 * rng.random((3, CLUMP))
    i = np.arange(CLUMP + 1, n, 9)
    src[:, i] = src[:, i - 1]                                   # exact duplicates: ties at every rank
    if scenario == "stream":                                    # duplicates across both chunk borders (ties decided by the global index)
        c = (n + STREAM_CHUNKS - 1) // STREAM_CHUNKS
        src[:, c:c + 300] = src[:, c - 300:c]
        src[:, 2 * c + 5:2 * c + 305] = src[:, :300]
    tgt = 0.1 + 0.8 * rng.random((3, m))                       # (the tile kernel hands over most targets near the cloud's faces)
    tgt[:, :300] = src[:, rng.choice(n, 300, replace=False)]   # on source points: d2 = 0
    tgt[0, 300:425] = 1.0 + 0.02 * rng.random(125)             # 2.5 % outside the bounding box
    if clump:
        tgt[:, 425:425 + CLUMP_TGT] = centre + 0.03 * rng.random((3, CLUMP_TGT))
    src += off; tgt += off
    src = src.astype(np.float32).astype(np.float64)             # the fp32 values ("far": a 2^-7 grid, many exact d2 ties)
    tgt = tgt.astype(np.float32).astype(np.float64)
    # pairs of sources near targets 600..999 whose fp32 roundings coincide: the farther one has the smaller index, so a ranking of the
    # fp32 values (a tie, decided by the index) orders them wrongly and the exact one does not (fp32 clouds: two more duplicates)
    j = np.arange(600, 1000)
    d = rng.standard_normal((3, len(j))); d /= np.linalg.norm(d, axis=0)
    b = (tgt[:, j] + (0.02 if off else 0.002) * d).astype(np.float32)
    ulp = np.spacing(np.nextafter(np.abs(b), np.float32(0))).astype(np.float64)      # (the finer spacing, where b is a power of two)
    b = b.astype(np.float64)
    toward = np.sign(tgt[:, j] - b)
    sa, sb = n - 2 - 2 * np.arange(len(j)), n - 1 - 2 * np.arange(len(j))
    src[:, sa] = b - 0.3 * ulp * toward
    src[:, sb] = b + 0.1 * ulp * toward
    assert (src[:, sa].astype(np.float32) == src[:, sb].astype(np.float32)).all()
    return np.ascontiguousarray(src.astype(dtype)), np.ascontiguousarray(tgt.astype(dtype))


def _lattice(dtype):
    """an integer lattice (x-major: stored in spatial order) and targets on it and half a step off it along one axis"""
    g = np.arange(LATTICE, dtype=np.float64)
    src = np.stack(np.meshgrid(g, g, g, indexing="ij")).reshape(3, -1)
    rng = np.random.default_rng(0x7A4)
    tgt = src[:, rng.choice(src.shape[1], 1500, replace=False)].copy()
    tgt[rng.integers(0, 3), 1::2] += 0.5
    return np.ascontiguousarray(src.astype(dtype)), np.ascontiguousarray(tgt.astype(dtype))


@pytest.fixture(scope="module")
def clouds(oracle):
    """(dtype, scenario) -> dict(src, tgt, rgb, nrm, idx, d2) with the oracle's 32 nearest, taken once: a k-list is its first k columns
    (exact under the order (d2, index))"""
    cache = {}

    def get(dtype, scenario):
        key = (dtype, scenario)
        if key not in cache:
            dt = np.float64 if dtype == "f64" else np.float32
            if scenario == "lattice":
                src, tgt = _lattice(dt)
            else:
                src, tgt = _make_cloud(dt, scenario, N_STREAM if scenario == "stream" else N)
            n = src.shape[1]
            wi, wd = oracle.knn_bruteforce(src, tgt, KMAX)
            cache[key] = dict(src=src, tgt=tgt, rgb=oracle.synth_rgb(0x7A, n), nrm=oracle.synth_nrm(0x7A, n), idx=wi, d2=wd)
        return cache[key]
    return get


def _check_route(pkg, st, row, k, m, what, want_retry, bound_leftover=True):
    """the row's instantiation ran (and, where asked, its retry launch over the blocks it passed on); it handed at most 5 % of the
    targets to the group kernel (25 % at k > 24).  bound_leftover=False: the clouds where exact d2 ties are everywhere -- the lattice,
    and the one far from the origin, where an fp64 cloud's fp32 shadow is also 2^-7 coarse: the tile kernel hands most of its targets
    over there (the group kernel answers them)"""
    got = st["tile_variant"]
    assert got[0] == TV.row_code(row), "%s: the tile launch ran %s, not the row's %s" % (what, TV.decode(got[0]), TV.decode(TV.row_code(row)))
    assert st["query_route"] & pkg.capi.ROUTE_TILE, what
    if bound_leftover:
        assert st["n_leftover"] <= (0.25 if k > 24 else 0.05) * m, "%s: %d of %d targets handed over" % (what, st["n_leftover"], m)
    if got[1] or st["tile_retry_blocks"]:
        assert row["retry"] and got[1] == TV.retry_code(row) and st["tile_retry_blocks"] > 0, "%s: retry %s over %d blocks" % (
            what, TV.decode(got[1]), st["tile_retry_blocks"])
    if want_retry:
        assert st["tile_retry_blocks"] > 0 and got[1] == TV.retry_code(row), "%s: no retry launch (%s)" % (what, st)


def _below(r, dtype):
    """the largest radius below r in the row's precision"""
    return float(np.nextafter(np.float32(r), np.float32(0))) if dtype == "f32" else float(np.nextafter(r, 0.0))


def _resident(pkg, oracle, row, c, scenario):
    import torch
    src, tgt, rgb, nrm = c["src"], c["tgt"], c["rgb"], c["nrm"]
    m = tgt.shape[1]
    with pkg.PointsTransfer(device=0, k_hint=max(row["ks"])) as p:
        p.set_param("tile", row["tile"]); p.set_param("tile_sparse", 0)
        p.build(src, rgb, nrm)
        p.set_targets(tgt)
        for k in row["ks"]:
            wi, wd = c["idx"][:, :k].copy(), c["d2"][:, :k].copy()
            if row["bound"] != "cap":
                radii = [None]
            elif scenario == "lattice":
                radii = [1.0, _below(1.0, row["dtype"]), 2.0, _below(2.0, row["dtype"])]
            else:                                               # 0; small; about the median k-th distance
                radii = [0.0, math.sqrt(float(np.quantile(wd[:, 0], 0.3))), math.sqrt(float(np.median(wd[:, k - 1])))]
            for r in radii:
                p.max_dist = r
                want = truncate(wi, wd, r) if r is not None else (wi, wd)
                what = "%s %s k=%d r=%r" % (row["id"], scenario, k, r)
                for mode in ((pkg.BLEND_MEAN, pkg.BLEND_INV_D2) if row["fused"] else (None,)):
                    i_ = torch.empty((m, k), dtype=torch.int32, device="cuda"); d_ = torch.empty((m, k), dtype=torch.float64, device="cuda")
                    if mode is None:
                        p.query_resident_dev(k, i_, d_)
                    else:
                        sc = np.full((m, 3), np.nan, np.float32); sc[1::2] = -7.0      # sentinels an empty row must keep
                        sn = np.full((m, 3), 3.0, np.float32)
                        c_ = torch.from_numpy(sc.copy()).cuda(); n_ = torch.from_numpy(sn.copy()).cuda()
                        p.query_blend_resident_dev(k, mode, i_, d_, c_, n_)
                    torch.cuda.synchronize()
                    _check_route(pkg, p.stats(), row, k, m, what, row["retry"] and scenario in ("uniform", "clumped"),
                                 scenario in ("uniform", "clumped"))
                    check_exact((i_.cpu().numpy().view(np.uint32), d_.cpu().numpy()), want, what)
                    if mode is not None:
                        check_blend(c_.cpu().numpy(), n_.cpu().numpy(), want[0], want[1], rgb, nrm, mode, sc, sn, oracle, "%s mode %d" % (what, mode))
            if scenario == "lattice":
                assert k == 1 or (wd == 1.0).any() or (wd == 4.0).any(), "the lattice must put candidates at exactly r"


def _stream(pkg, row, c, k, cap=None):
    n = c["src"].shape[1]
    with pkg.PointsTransfer(device=0, k_hint=k, max_dist=cap) as p:
        p.set_param("tile", row["tile"]); p.set_param("tile_sparse", 0)
        p.set_targets(c["tgt"])
        gi, gd = p.stream_query(c["src"], (n + STREAM_CHUNKS - 1) // STREAM_CHUNKS, k)
        return gi, gd, p.stats()


@pytest.mark.parametrize("row", TV.ROWS, ids=[r["id"] for r in TV.ROWS])
def test_tile_variant_answers_like_the_oracle(pkg, oracle, clouds, row):
    if row["bound"] != "stream":
        main = "clumped" if row["K"] == 8 else "uniform"       # (k <= 8: only the clump's regions exceed the small budget)
        for scenario in ((main, "lattice") if row["bound"] == "cap" else (main, "far")):
            _resident(pkg, oracle, row, clouds(row["dtype"], scenario), scenario)
        return
    # streamed chunks: the bounded variant searches every chunk under the bounds the targets bring.  Chunks in random order: nearly every
    # target lies inside the first chunk's box, gets a full list there, and brings a FINITE bound into the later chunks
    c = clouds(row["dtype"], "stream")
    first = c["src"][:, :(c["src"].shape[1] + STREAM_CHUNKS - 1) // STREAM_CHUNKS]
    lo, hi = first.min(axis=1), first.max(axis=1)
    assert ((c["tgt"] >= lo[:, None]) & (c["tgt"] <= hi[:, None])).all(axis=0).mean() > 0.9
    L = clouds(row["dtype"], "lattice")
    for k in row["ks"]:
        gi, gd, st = _stream(pkg, row, c, k)
        what = "%s stream k=%d" % (row["id"], k)
        _check_route(pkg, st, row, k, c["tgt"].shape[1], what, False)
        assert st["stream_revisited"] == 0, what
        assert np.array_equal(gi, c["idx"][:, :k].astype(np.uint64)), what + ": indices"
        assert np.array_equal(gd, c["d2"][:, :k]), what + ": d2"
        # the lattice in spatial order under the cap: a target without a list is searched within r, one with a list within min(k-th, r):
        # candidates at exactly r are in, just below r they are out
        for r in (1.0, _below(1.0, row["dtype"]), 2.0, _below(2.0, row["dtype"])):
            gi, gd, st = _stream(pkg, row, L, k, cap=r)
            what = "%s stream lattice k=%d r=%r" % (row["id"], k, r)
            _check_route(pkg, st, row, k, L["tgt"].shape[1], what, False)
            check_exact((np.where(gi == U64_NONE, np.uint64(NOIDX), gi).astype(np.uint32), gd), truncate(L["idx"][:, :k], L["d2"][:, :k], r), what)
