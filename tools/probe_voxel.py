"""pt_voxel_downsample against the composition it replaces (the cloud read back, downsampled on the host with numpy -- lexsort of the
voxel indices, segment means -- uploaded and built again), on 100 M uniform fp32 points, for a few voxel sizes: warm times (median and
spread of the repeats).  The new entry's times are device times (HIP events, pt_stats_t.ms_voxel) with its wall time beside them; the
composition crosses PCIe and computes on the host, so it is timed by the host clock around calls that end in a device synchronise.
Both are measured in the same run; the last lines are the README row.
    python tools/probe_voxel.py [scale]      # scale < 1 shrinks the cloud (0.1: a quick look)"""
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
N = int(100_000_000 * scale)
VOXELS = (0.002, 0.005, 0.02)      # ~0.8, ~12 and ~800 points per voxel at 100 M points in the unit cube


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def build_dev(p, xyz):
    p._adopt_torch_stream()
    p._chk(p._L.pt_build_soa(p._h, xyz.data_ptr(), pkg.F32, None, None, xyz.shape[1], 1))


def host_downsample(x, v):
    """what a host would do: means per voxel in float64 (not the entry's bit-exact definition, which no host tool implements)"""
    p = x.astype(np.float64)
    i = np.floor((p - p.min(axis=1, keepdims=True)) / v).astype(np.int64)
    order = np.lexsort((i[0], i[1], i[2]))
    s = i[:, order]
    head = np.ones(x.shape[1], bool)
    head[1:] = (s[:, 1:] != s[:, :-1]).any(axis=0)
    start = np.flatnonzero(head)
    cnt = np.diff(np.append(start, x.shape[1]))
    return np.ascontiguousarray((np.add.reduceat(p[:, order], start, axis=1) / cnt).astype(np.float32))


gen = torch.Generator(device="cuda").manual_seed(0xC3)
xyz = torch.rand((3, N), generator=gen, device="cuda", dtype=torch.float32).contiguous()
rows = []
for v in VOXELS:
    with pkg.PointsTransfer(device=0, k_hint=16) as p:
        dev, wall, dry, rebuild = [], [], [], []
        for it in range(REPS + 1):
            build_dev(p, xyz)
            p.voxel_downsample_dev(None, None, v, apply=False); torch.cuda.synchronize()
            a = p.stats()
            t0 = time.perf_counter()
            info = p.voxel_downsample_dev(None, None, v, apply=True); torch.cuda.synchronize()
            w = (time.perf_counter() - t0) * 1e3
            b = p.stats()
            if it:      # (the first round allocates)
                dev.append(b["ms_voxel"]); wall.append(w); dry.append(a["ms_voxel"]); rebuild.append(b["ms_build"])
        rows.append({"entry": "pt_voxel_downsample", "n": N, "voxel": v, "n_voxels": info["n_voxels"], "max_count": info["max_count"], "passes": b["n_voxel_passes"],
                     "ms": spread(dev), "ms_wall": spread(wall), "ms_without_apply": statistics.median(dry), "ms_rebuild_alone": statistics.median(rebuild), "device_bytes": b["device_bytes"]})
        print(json.dumps(rows[-1]), flush=True)
    with pkg.PointsTransfer(device=0, k_hint=16) as p:
        wall, parts = [], []
        for it in range(REPS + 1):
            build_dev(p, xyz)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = xyz.cpu().numpy()
            t1 = time.perf_counter()
            thin = host_downsample(host, v)
            t2 = time.perf_counter()
            p.build(thin); torch.cuda.synchronize()
            t3 = time.perf_counter()
            if it:
                wall.append((t3 - t0) * 1e3); parts.append([(t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3])
        med = [statistics.median(c) for c in zip(*parts)]
        rows.append({"entry": "read-back + host downsample + upload + build", "n": N, "voxel": v, "n_voxels": int(thin.shape[1]), "ms_wall": spread(wall),
                     "ms_readback": med[0], "ms_host": med[1], "ms_upload_build": med[2], "same_count_as_new_entry": bool(thin.shape[1] == info["n_voxels"])})
        print(json.dumps(rows[-1]), flush=True)
for r in rows:
    print("v = %-6g %-46s %10.2f ms wall (%.2f .. %.2f)%s" % (r["voxel"], r["entry"], r["ms_wall"]["median"], r["ms_wall"]["min"], r["ms_wall"]["max"],
          ", %.2f ms device (%d passes, %d voxels)" % (r["ms"]["median"], r["passes"], r["n_voxels"]) if "ms" in r else ""))
new = [r for r in rows if "ms" in r]
old = [r for r in rows if "ms" not in r]
print("README row: | `pt_voxel_downsample` ... | %d M points, v = %s: %s ms on the device (%s ms wall) against %s ms for read-back + host downsample + upload + build |" % (
    N // 1_000_000, " / ".join("%g" % r["voxel"] for r in new), " / ".join("%.1f" % r["ms"]["median"] for r in new), " / ".join("%.1f" % r["ms_wall"]["median"] for r in new),
    " / ".join("%.0f" % r["ms_wall"]["median"] for r in old)))
