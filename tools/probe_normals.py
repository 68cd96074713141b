"""pt_estimate_normals against the composition it replaces (targets = the cloud itself, pt_query_resident, pt_pca_normals_dev), on
the C3 shape (100 M uniform points, fp32, k = 16) and on the 50 M-point sphere shell of tools/probe_surface.py (k = 20):
warm device time from HIP events (median and spread of the repeats), per-phase split, peak device bytes, chunk-size sensitivity.
    python tools/probe_normals.py [scale]      # scale < 1 shrinks both clouds (0.1: a quick look)"""
import json
import statistics
import sys
sys.path.insert(0, '.')
import numpy as np
import torch
import __graft_entry__ as g
pkg = g.load_package()
scale = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
REPS = 3
MI = 1 << 20


def sphere(cnt, noise, rng):
    v = rng.standard_normal((3, cnt)).astype(np.float32)
    v /= np.linalg.norm(v, axis=0, keepdims=True)
    return (0.5 + 0.45 * v + noise * rng.standard_normal((3, cnt)).astype(np.float32)).astype(np.float32)


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def run(name, build, k):
    rows = []
    with pkg.PointsTransfer(device=0, k_hint=k) as p:
        build(p)
        n = p.num_source
        base = p.stats()["device_bytes"]
        out = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        for chunk in (1 * MI, 8 * MI, 32 * MI):      # (ascending: buffers only grow, so device_bytes is each size's own peak)
            p.set_param("normals_chunk", chunk)
            tot, cp, se = [], [], []
            for it in range(REPS + 1):
                p.estimate_normals_dev(k, out); torch.cuda.synchronize()
                st = p.stats()
                if it:      # (the first call allocates)
                    tot.append(st["ms_normals"]); cp.append(st["ms_sort_targets"]); se.append(st["ms_query"])
            rows.append({"workload": name, "n": n, "k": k, "entry": "pt_estimate_normals", "chunk": chunk, "chunks": st["n_normal_chunks"], "ms": spread(tot),
                         "ms_chunk_copy": statistics.median(cp), "ms_search": statistics.median(se), "ms_pca_and_rest": statistics.median(tot) - statistics.median(cp) - statistics.median(se),
                         "device_bytes": st["device_bytes"], "device_bytes_over_built_cloud": st["device_bytes"] - base, "caller_bytes": out.numel() * 4,
                         "route": st["query_route"]})
            print(json.dumps(rows[-1]), flush=True)
        new = out.clone()
    # the composition, in a context of its own (so that its peak is its own)
    with pkg.PointsTransfer(device=0, k_hint=k) as p:
        build(p)
        n = p.num_source
        base = p.stats()["device_bytes"]
        xyz = torch.empty((3, n), dtype=torch.float32, device="cuda")
        assert p.resident_source_xyz_dev(xyz) == pkg.F32
        idx = torch.empty((n, k), dtype=torch.int32, device="cuda")
        out = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        tot, so, se, pc = [], [], [], []
        for it in range(REPS + 1):
            p.set_targets(xyz, xyz_type=pkg.F32)
            p.query_resident_dev(k, idx); torch.cuda.synchronize()
            a = p.stats()
            p.pca_normals_dev(idx, n, k, out); torch.cuda.synchronize()
            b = p.stats()
            if it:
                so.append(a["ms_sort_targets"]); se.append(a["ms_query"]); pc.append(b["ms_pca"]); tot.append(so[-1] + se[-1] + pc[-1])
        rows.append({"workload": name, "n": n, "k": k, "entry": "targets + query_resident + pca_normals_dev", "ms": spread(tot), "ms_target_sort": statistics.median(so),
                     "ms_search": statistics.median(se), "ms_pca": statistics.median(pc), "device_bytes": b["device_bytes"], "device_bytes_over_built_cloud": b["device_bytes"] - base,
                     "caller_bytes": (xyz.numel() + idx.numel() + out.numel()) * 4, "route": a["query_route"],
                     "same_as_new_entry_up_to_sign": bool(torch.equal(out.abs(), new.abs()))})
        print(json.dumps(rows[-1]), flush=True)
    return rows


n1, n2 = int(100_000_000 * scale), int(50_000_000 * scale)
rows = run("uniform", lambda p: p.build_synth(n1, 0xC3, xyz_type=pkg.F32), 16)
src = sphere(n2, 1e-4, np.random.default_rng(1))
rows += run("sphere shell", lambda p: p.build(src), 20)
for r in rows:
    print("%-13s %-44s chunk %9s: %8.2f ms (%.2f .. %.2f), %6.2f GB in the context over the built cloud + %5.2f GB held by the caller" % (
        r["workload"], r["entry"], r.get("chunk", "-"), r["ms"]["median"], r["ms"]["min"], r["ms"]["max"], r["device_bytes_over_built_cloud"] / 1e9, r["caller_bytes"] / 1e9))
