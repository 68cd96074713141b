"""max_dist ("--max-dist") cost and gain: one JSON line per case.

  full   100 M / 10 M uniform fp32, fused query (query + blend), k = 8 and 20: uncapped against a cap so large that every list stays
         full (the capped tile variants pay their bound and nothing else)
  holes  50 M-point sphere shell with a quarter of the sphere removed, 2.5 M targets on the whole sphere, k = 20, r = 3x the median
         k-th distance: query and fused query, uncapped against capped, with the hand-over counters (n_leftover, n_wave)

ms are device times of the search (pt_stats ms_query, sync mode), the median of REPS runs after one warm-up.
usage: python tools/probe_max_dist.py [full|holes|all] [REPS]"""
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (before libpt_hip.so: one HIP runtime)
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package()
WHAT = sys.argv[1] if len(sys.argv) > 1 else "all"
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5


def timed(p, run):
    run()                                                                  # warm-up (allocations, first-touch)
    ms, st = [], None
    for _ in range(REPS):
        run()
        torch.cuda.synchronize()
        st = p.stats()
        ms.append(st["ms_query"])
    return float(np.median(ms)), st


def case_full():
    n, m, seed = 100_000_000, 10_000_000, 0xC3
    for k in (8, 20):
        with pkg.PointsTransfer(device=0, k_hint=k) as p:
            p.set_param("sync", 1)
            p.build_synth(n, seed)
            p.targets_synth(m, seed)
            idx = torch.empty((m, k), dtype=torch.int32, device="cuda"); d2 = torch.empty((m, k), dtype=torch.float64, device="cuda")
            rgb = torch.empty((m, 3), dtype=torch.float32, device="cuda"); nrm = torch.empty((m, 3), dtype=torch.float32, device="cuda")
            fused = lambda: p.query_blend_resident_dev(k, pkg.BLEND_MEAN, idx, d2, rgb, nrm)
            res = {}
            for cap in (None, 0.1):                                       # 0.1: ~15x the k-th distance of every target here
                p.max_dist = cap
                ms, st = timed(p, fused)
                res["capped" if cap else "uncapped"] = {"ms": round(ms, 3), "n_leftover": int(st["n_leftover"]), "n_wave": int(st["n_wave"])}
            full = int((idx[:, k - 1].cpu().numpy().view(np.uint32) != pkg.NOIDX).sum())
            print(json.dumps({"case": "full", "n": n, "m": m, "k": k, "r": 0.1, "lists_full": full, **res,
                              "capped_vs_uncapped": round(res["capped"]["ms"] / res["uncapped"]["ms"], 4)}), flush=True)


def shell(rng, n, cut):
    out, have = [], 0
    while have < n:
        v = rng.standard_normal((3, 8_000_000)).astype(np.float64)
        v /= np.linalg.norm(v, axis=0)
        if cut:
            v = v[:, ~((v[0] > 0) & (v[1] > 0))]                          # a quarter of the sphere removed
        out.append((0.5 + 0.4 * v).astype(np.float32)); have += v.shape[1]
    return np.ascontiguousarray(np.concatenate(out, axis=1)[:, :n])


def case_holes():
    n, m, k = 50_000_000, 2_500_000, 20
    rng = np.random.default_rng(0x5E)
    src, tgt = shell(rng, n, True), shell(rng, m, False)
    with pkg.PointsTransfer(device=0, k_hint=k) as p:
        p.set_param("sync", 1)
        rgb = np.zeros((n, 3), np.uint8); nrm = np.zeros((n, 3), np.float32)
        p.build(src, rgb, nrm)
        p.set_targets(tgt)
        idx = torch.empty((m, k), dtype=torch.int32, device="cuda"); d2 = torch.empty((m, k), dtype=torch.float64, device="cuda")
        c_ = torch.empty((m, 3), dtype=torch.float32, device="cuda"); n_ = torch.empty((m, 3), dtype=torch.float32, device="cuda")
        p.query_resident_dev(k, idx, d2)
        kth = d2[:, k - 1].cpu().numpy()
        r = 3.0 * math.sqrt(float(np.median(kth)))
        for name, run in (("query", lambda: p.query_resident_dev(k, idx, d2)),
                          ("fused", lambda: p.query_blend_resident_dev(k, pkg.BLEND_MEAN, idx, d2, c_, n_))):
            res = {}
            for cap in (None, r):
                p.max_dist = cap
                ms, st = timed(p, run)
                res["capped" if cap else "uncapped"] = {"ms": round(ms, 3), "n_leftover": int(st["n_leftover"]), "n_wave": int(st["n_wave"])}
            empty = int((idx[:, 0].cpu().numpy().view(np.uint32) == pkg.NOIDX).sum())
            print(json.dumps({"case": "holes", "path": name, "n": n, "m": m, "k": k, "r": r, "targets_without_neighbours": empty, **res,
                              "capped_vs_uncapped": round(res["capped"]["ms"] / res["uncapped"]["ms"], 4)}), flush=True)


if WHAT in ("full", "all"):
    case_full()
if WHAT in ("holes", "all"):
    case_holes()
