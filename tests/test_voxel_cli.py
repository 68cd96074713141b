"""The CLI's --voxel-downsample argument checks (no GPU needed: arguments are checked before any device work)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "3d-reconstruction-from-point-cloud_amd", "pointsTransfer")
VOX = "--voxel-downsample"


def _run(args, cwd):
    return subprocess.run([EXE] + args, capture_output=True, text=True, cwd=cwd)


def test_the_flag_is_a_known_option(tmp_path):
    # the flag gets past the argument loop: the missing cloud file is then reported and the tool exits 0, as the reference does
    for opts in ([VOX, "0.005"], [VOX, "1e-3", "--gpus", "1"], [VOX, "2.5", "--max-dist", "0.1"],
                 [VOX, "0.01", "--remove-isolated", "4", "0.05", "--remove-outliers", "16", "2.0", "--estimate-normals", "16"],
                 ["--estimate-normals", "16", "--remove-outliers", "16", "2.0", VOX, "0.01", "--remove-isolated", "4", "0.05", "--gpus", "1"]):
        r = _run(["missing_cloud.ply", "missing_mesh.ply"] + opts, tmp_path)
        assert r.returncode == 0, (opts, r.stderr)
        assert "unknown option" not in r.stderr and "Cannot read or find point cloud file" in r.stderr
    assert not os.listdir(tmp_path)


@pytest.mark.parametrize("v", ["0", "0.0", "-0.01", "nan", "inf", "-inf", "small", "0.01x", ""])
def test_the_voxel_size_must_be_finite_and_positive(tmp_path, v):
    r = _run(["a", "b", VOX, v], tmp_path)
    assert r.returncode == 2 and VOX in r.stderr
    assert not os.listdir(tmp_path)


def test_missing_value_exits_2(tmp_path):
    r = _run(["a", "b", VOX], tmp_path)
    assert r.returncode == 2 and VOX in r.stderr
    assert not os.listdir(tmp_path)


@pytest.mark.parametrize("opts", [[VOX, "0.01"], [VOX, "0.01", "--remove-outliers", "16", "2"]])
def test_not_with_synthetic(tmp_path, opts):
    r = _run(["a", "b", "--synthetic", "1000", "100", "1"] + opts, tmp_path)
    assert r.returncode == 2 and VOX in r.stderr and "--synthetic" in r.stderr
    assert not os.listdir(tmp_path)


@pytest.mark.parametrize("extra", [["--gpus", "2"], ["--gpus", "2", "--rank", "0", "--rendezvous", "rv"], ["--gpus", "2", "--finalize", "--rendezvous", "rv"]])
def test_not_with_several_gpus(tmp_path, extra):
    # nothing is launched and nothing is written: neither by a launcher, nor by a rank or finalize process
    r = _run(["a", "b"] + extra + [VOX, "0.01"], tmp_path)
    assert r.returncode == 2 and VOX in r.stderr and "--gpus" in r.stderr
    assert not os.listdir(tmp_path)
