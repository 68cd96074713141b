"""The CLI's --remove-outliers / --remove-isolated argument checks (no GPU needed: arguments are checked before any device work)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "3d-reconstruction-from-point-cloud_amd", "pointsTransfer")
SOR, RAD = "--remove-outliers", "--remove-isolated"


def _run(args, cwd):
    return subprocess.run([EXE] + args, capture_output=True, text=True, cwd=cwd)


def test_both_flags_are_known_options(tmp_path):
    # both flags get past the argument loop: the missing cloud file is then reported and the tool exits 0, as the reference does
    r = _run(["missing_cloud.ply", "missing_mesh.ply", SOR, "16", "2.0", RAD, "4", "0.05"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert "unknown option" not in r.stderr and "Cannot read or find point cloud file" in r.stderr
    for opts in ([SOR, "2", "0"], [SOR, "32", "1e3"], [RAD, "1", "1e-6"], [RAD, "31", "2.5"], [SOR, "16", "2", "--estimate-normals", "16"]):
        r = _run(["missing_cloud.ply", "missing_mesh.ply"] + opts + ["--gpus", "1"], tmp_path)      # one GPU: the unsharded path
        assert r.returncode == 0, (opts, r.stderr)
        assert "Cannot read or find point cloud file" in r.stderr


@pytest.mark.parametrize("k", ["1", "33", "0", "-4", "many", "16.5"])
def test_statistical_k_out_of_range_exits_2(tmp_path, k):
    r = _run(["a", "b", SOR, k, "2.0"], tmp_path)
    assert r.returncode == 2 and SOR in r.stderr


@pytest.mark.parametrize("alpha", ["-0.5", "nan", "inf", "two", "1.0x"])
def test_statistical_alpha_must_be_finite_and_not_negative(tmp_path, alpha):
    r = _run(["a", "b", SOR, "16", alpha], tmp_path)
    assert r.returncode == 2 and SOR in r.stderr


@pytest.mark.parametrize("m", ["0", "32", "-1", "few"])
def test_radius_min_out_of_range_exits_2(tmp_path, m):
    r = _run(["a", "b", RAD, m, "0.05"], tmp_path)
    assert r.returncode == 2 and RAD in r.stderr


@pytest.mark.parametrize("radius", ["0", "-1", "nan", "inf", "wide"])
def test_radius_must_be_finite_and_positive(tmp_path, radius):
    r = _run(["a", "b", RAD, "4", radius], tmp_path)
    assert r.returncode == 2 and RAD in r.stderr


@pytest.mark.parametrize("opts", [[SOR], [SOR, "16"], [RAD], [RAD, "4"]])
def test_missing_value_exits_2(tmp_path, opts):
    r = _run(["a", "b"] + opts, tmp_path)
    assert r.returncode == 2 and opts[0] in r.stderr


@pytest.mark.parametrize("opts", [[SOR, "16", "2"], [RAD, "4", "0.05"], [RAD, "4", "0.05", SOR, "16", "2"]])
def test_not_with_synthetic(tmp_path, opts):
    r = _run(["a", "b", "--synthetic", "1000", "100", "1"] + opts, tmp_path)
    assert r.returncode == 2 and opts[0] in r.stderr and "--synthetic" in r.stderr


@pytest.mark.parametrize("extra", [["--gpus", "2"], ["--gpus", "2", "--rank", "0", "--rendezvous", "rv"], ["--gpus", "2", "--finalize", "--rendezvous", "rv"]])
@pytest.mark.parametrize("opts", [[SOR, "16", "2"], [RAD, "4", "0.05"]])
def test_not_with_several_gpus(tmp_path, opts, extra):
    # nothing is launched and nothing is written: neither by a launcher, nor by a rank or finalize process
    r = _run(["a", "b"] + extra + opts, tmp_path)
    assert r.returncode == 2 and opts[0] in r.stderr and "--gpus" in r.stderr
    assert not os.listdir(tmp_path)
