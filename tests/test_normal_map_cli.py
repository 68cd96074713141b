"""The CLI's --normal-map argument check (no GPU needed: arguments are checked before any device work)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "3d-reconstruction-from-point-cloud_amd", "pointsTransfer")


def test_normal_map_with_synthetic_exits_2(tmp_path):
    # --synthetic has no mesh, so there is nothing to bake a map onto: refused like any other bad argument, before any device work
    r = subprocess.run([EXE, "a", "b", "--synthetic", "1000", "100", "1", "--normal-map", "x.png"], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 2 and "--normal-map" in r.stderr
    assert not os.path.exists(tmp_path / "x.png")


def test_normal_map_is_a_known_option(tmp_path):
    # the flag gets past the argument loop: the missing cloud file is then reported and the tool exits 0, as the reference does
    r = subprocess.run([EXE, "missing_cloud.ply", "missing_mesh.ply", "--normal-map", "n.png"], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert "unknown option" not in r.stderr and "Cannot read or find point cloud file" in r.stderr
