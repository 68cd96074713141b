"""pt_remove_outliers against the composition it replaces (the cloud uploaded as targets, pt_query_resident with d2, the distances read
back, the mask computed on the host, pt_build_soa of the kept subset), on 100 M uniform points with 1 % injected strays (fp32, k = 16)
and on the 50 M-point sphere shell of tools/probe_surface.py with the same share of strays (k = 20), statistical filter, alpha = 2:
warm times (median and spread of the repeats) and the new entry's split into search, score + reduce, compaction + rebuild.
The new entry's times are device times (HIP events, pt_stats_t.ms_outliers); the composition crosses PCIe and computes on the host, so
it is timed by the host clock around calls that end in a device synchronise -- the new entry's wall time is printed beside it.
    python tools/probe_outliers.py [scale]      # scale < 1 shrinks both clouds (0.1: a quick look)"""
import json
import statistics
import sys
import time
sys.path.insert(0, '.')
import numpy as np
import torch
import __graft_entry__ as g
pkg = g.load_package()
scale = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
REPS = 3
ALPHA = 2.0


def with_strays(xyz, seed):
    """1 % of the points replaced by points uniform in [-1, 2)^3, on the device"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    n = xyz.shape[1]
    pos = torch.randperm(n, generator=gen, device="cuda")[: n // 100]
    xyz[:, pos] = torch.rand((3, pos.numel()), generator=gen, device="cuda", dtype=torch.float32) * 3 - 1
    return xyz.contiguous()


def uniform(cnt):
    gen = torch.Generator(device="cuda").manual_seed(0xC3)
    return with_strays(torch.rand((3, cnt), generator=gen, device="cuda", dtype=torch.float32), 7)


def sphere(cnt):
    gen = torch.Generator(device="cuda").manual_seed(1)
    v = torch.randn((3, cnt), generator=gen, device="cuda", dtype=torch.float32)
    v /= v.norm(dim=0, keepdim=True)
    return with_strays(0.5 + 0.45 * v + 1e-4 * torch.randn((3, cnt), generator=gen, device="cuda", dtype=torch.float32), 8)


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def build_dev(p, xyz):
    p._adopt_torch_stream()
    p._chk(p._L.pt_build_soa(p._h, xyz.data_ptr(), pkg.F32, None, None, xyz.shape[1], 1))


def run(name, xyz, k):
    n = xyz.shape[1]
    rows = []
    keep_dev = torch.empty(n, dtype=torch.uint8, device="cuda")
    with pkg.PointsTransfer(device=0, k_hint=k) as p:
        tot, search, dry, rebuild, wall = [], [], [], [], []
        for it in range(REPS + 1):
            build_dev(p, xyz)
            p.remove_outliers_dev(keep_dev, None, k, ALPHA, apply=False); torch.cuda.synchronize()
            a = p.stats()
            t0 = time.perf_counter()
            info = p.remove_outliers_dev(keep_dev, None, k, ALPHA, apply=True); torch.cuda.synchronize()
            w = (time.perf_counter() - t0) * 1e3
            b = p.stats()
            if it:      # (the first round allocates)
                tot.append(b["ms_outliers"]); search.append(b["ms_sort_targets"] + b["ms_query"]); dry.append(a["ms_outliers"]); rebuild.append(b["ms_build"]); wall.append(w)
        rows.append({"workload": name, "n": n, "k": k, "entry": "pt_remove_outliers", "kept": info["n_kept"], "threshold": info["threshold"], "chunks": b["n_outlier_chunks"],
                     "ms": spread(tot), "ms_wall": spread(wall), "ms_search": statistics.median(search),
                     "ms_score_reduce": statistics.median(dry) - statistics.median(search), "ms_compact_rebuild": statistics.median(tot) - statistics.median(dry),
                     "ms_rebuild_alone": statistics.median(rebuild), "device_bytes": b["device_bytes"], "route": b["query_route"]})
        print(json.dumps(rows[-1]), flush=True)
        new_keep = keep_dev.cpu().numpy().astype(bool)
    # the composition available without the entry, in a context of its own
    with pkg.PointsTransfer(device=0, k_hint=k) as p:
        d2 = torch.empty((n, k), dtype=torch.float64, device="cuda")
        idx = torch.empty((n, k), dtype=torch.int32, device="cuda")
        host = np.empty((n, k), np.float64)
        wall, parts = [], []
        for it in range(REPS + 1):
            build_dev(p, xyz)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p.set_targets(xyz, xyz_type=pkg.F32)
            p.query_resident_dev(k, idx, d2); torch.cuda.synchronize()
            t1 = time.perf_counter()
            for lo in range(0, n, 1 << 22):      # (in slices: no second host copy of the matrix)
                host[lo:lo + (1 << 22)] = d2[lo:lo + (1 << 22)].cpu().numpy()
            t2 = time.perf_counter()
            s = np.sqrt(host[:, 1:]).sum(axis=1) / (k - 1)
            mu = s.mean()
            keep = s <= mu + ALPHA * np.sqrt(((s - mu) ** 2).mean())
            sub = np.ascontiguousarray(xyz.cpu().numpy()[:, keep])
            t3 = time.perf_counter()
            p.build(sub); torch.cuda.synchronize()
            t4 = time.perf_counter()
            if it:
                wall.append((t4 - t0) * 1e3); parts.append([(t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3])
        med = [statistics.median(c) for c in zip(*parts)]
        rows.append({"workload": name, "n": n, "k": k, "entry": "targets + query_resident(d2) + read-back + host mask + build_soa", "kept": int(keep.sum()),
                     "ms_wall": spread(wall), "ms_query": med[0], "ms_readback": med[1], "ms_host_mask": med[2], "ms_upload_build": med[3],
                     "device_bytes": p.stats()["device_bytes"], "same_mask_as_new_entry": bool(np.array_equal(keep, new_keep))})
        print(json.dumps(rows[-1]), flush=True)
    return rows


n1, n2 = int(100_000_000 * scale), int(50_000_000 * scale)
rows = run("uniform + 1 % strays", uniform(n1), 16)
torch.cuda.empty_cache()
rows += run("sphere shell + 1 % strays", sphere(n2), 20)
for r in rows:
    print("%-26s %-66s %10.2f ms wall (%.2f .. %.2f)%s" % (r["workload"], r["entry"], r["ms_wall"]["median"], r["ms_wall"]["min"], r["ms_wall"]["max"],
          ", %.2f ms device: search %.2f, score + reduce %.2f, compaction + rebuild %.2f" % (r["ms"]["median"], r["ms_search"], r["ms_score_reduce"], r["ms_compact_rebuild"]) if "ms" in r else ""))
