"""Encode to an RMS or PSNR target, the parts that need no GPU: wr_psnr_rms against its formula, the argument errors of
wrenc --rmse / --psnr (they come before any device call), and the reference the GPU tests are judged by (tests/rms_ref.py) held
against the contract AND the guard condition for exactly the inputs tests/test_gpu_quality.py uses (tests/rms_cases.py): at the
reference's g and g + 1, R* lies further than 2^-30 (relative) from the target, so the library's 2^-36 accuracy cannot change a
verdict."""
import math
import os

import numpy as np
import pytest

import rms_cases as rc
from rms_ref import GMAX, GUARD
from test_gpu_cli_seg import WRENC, run
from waverange_amd import api

ARGS = ["data.bin", "data.wrb", "data.wrh", "2", "0", "1", "2", "8", "8", "8", "1e-9"]


def ulps(a, b):
    return abs(a - b) / np.spacing(abs(b))


def test_psnr_rms_equals_the_formula_to_4_ulp():
    for db in (60.0, 20.0, 0.0, -3.0, 96.33, 150.0, 1e-3):
        for lo, hi in ((0.0, 1.0), (-1.5, 2.25), (1e-300, 3e-300), (-1e300, 1e300 / 3), (5.0, 5.0 + 2.0 ** -40)):
            want = (np.float64(hi) - np.float64(lo)) * 10.0 ** (-db / 20.0)
            assert ulps(api.psnr_rms(db, lo, hi), want) <= 4, (db, lo, hi)
    assert api.psnr_rms(60.0, 0.0, 2.0) < api.psnr_rms(40.0, 0.0, 2.0) < 2.0
    assert api.psnr_rms(0.0, -1.0, 1.0) == 2.0


def test_psnr_rms_refuses_bad_arguments():
    for bad in (np.nan, np.inf, -np.inf):
        assert math.isnan(api.psnr_rms(bad, 0.0, 1.0)), bad
        assert math.isnan(api.psnr_rms(60.0, bad, 1.0)) and math.isnan(api.psnr_rms(60.0, 0.0, bad)), bad
    assert math.isnan(api.psnr_rms(60.0, 1.0, 1.0))  # an empty range
    assert math.isnan(api.psnr_rms(60.0, 2.0, 1.0))  # hi below lo
    assert math.isnan(api.psnr_rms(60.0, -1e308, 1e308))  # a range that is not finite


@pytest.mark.parametrize("options,message", [
    (["--rmse=0"], "--rmse=0: a positive number is required"),
    (["--rmse=-1e-3"], "--rmse=-1e-3: a positive number is required"),
    (["--rmse=nan"], "a positive number is required"),
    (["--rmse=inf"], "a positive number is required"),
    (["--rmse="], "a positive number is required"),
    (["--psnr=x"], "--psnr=x: a positive number is required"),
    (["--psnr=0"], "--psnr=0: a positive number is required"),
    (["--psnr=60dB"], "a positive number is required"),
    (["--rmse=1e-3", "--psnr=60"], "--rmse and --psnr exclude one another"),
    (["--psnr=60", "--rmse=1e-3"], "--rmse and --psnr exclude one another"),
    (["--rmse=1e-3", "--maxerr=1e-3"], "--rmse and --maxerr exclude one another"),
    (["--psnr=60", "--maxerr=1e-3"], "--psnr and --maxerr exclude one another"),
    (["--rmse=1e-3", "--ratio=8"], "--rmse and --ratio exclude one another"),
    (["--psnr=60", "--ratio=8"], "--psnr and --ratio exclude one another")])
def test_wrenc_refuses_bad_quality_options_before_anything_is_written(tmp_path, options, message):
    np.zeros(512).tofile(str(tmp_path / "data.bin"))
    r = run(WRENC, options + ["--format=wrs1"] + ARGS, tmp_path)
    assert r.returncode == 2, (r.returncode, r.stdout[-500:])
    assert message in r.stdout, r.stdout[-500:]
    assert sorted(os.listdir(tmp_path)) == ["data.bin"]


@pytest.mark.parametrize("fmt", [["--format=ref"], []])
@pytest.mark.parametrize("opt", ["--rmse=1e-3", "--psnr=60"])
def test_wrenc_quality_options_need_a_segmented_format(tmp_path, opt, fmt):
    np.zeros(512).tofile(str(tmp_path / "data.bin"))
    r = run(WRENC, [opt] + fmt + ARGS, tmp_path)
    assert r.returncode == 2, (r.returncode, r.stdout[-500:])
    assert opt.split("=")[0] + " needs --format=wrs1, wrs2 or wrs3" in r.stdout
    assert sorted(os.listdir(tmp_path)) == ["data.bin"]


def all_inputs():
    seen = set()
    for _, kind, dims, seg, wtflag, f32, _, _ in rc.CALLS:
        key = (kind, dims, seg, wtflag, f32)
        if key not in seen:
            seen.add(key)
            yield key


def test_the_reference_meets_the_contract_and_the_guard_on_the_gpu_tests_inputs():
    for key in all_inputs():
        _, ref = rc.ref_of(*key)
        for name, norm, target, m in rc.targets_of(*key):
            g, trials = ref.solve(m)
            assert g is not None and trials >= 1, (key, name)
            assert ref.verdict(g, m) is None, (key, name, ref.verdict(g, m))
            assert ref.R(g) <= m and (g == GMAX or ref.R(g + 1) > m)
            assert ref.guarded(g, m), (key, name, g, m, ref.R(g), ref.R(min(g + 1, GMAX)), GUARD)
            assert ref.R(g) <= ref.E(g)  # the RMS error never exceeds the pointwise one
            if name == "psnr 60":
                assert m == ref.range * 10.0 ** -3 or abs(m - ref.range * 1e-3) <= 4 * np.spacing(m)
            if name == "above max|f|":
                assert g >= GMAX - 64, (key, g)


def test_the_targets_make_the_search_walk_coarser_from_the_start_point():
    """RMS <= max error, so the start point of the pointwise search normally holds and lies finer than the answer"""
    _, ref = rc.ref_of("smooth", (64, 64, 64), 0)
    for name, norm, target, m in rc.targets_of("smooth", (64, 64, 64), 0)[:3]:
        s = ref.start(m)
        g, trials = ref.solve(m)
        assert 0 <= s < g and ref.R(s) <= m, (name, s, g)
        assert 2 <= trials <= 24, (name, trials)


def test_a_tol_min_too_coarse_for_the_target_is_a_miss():
    _, ref = rc.ref_of("smooth", (39, 37, 33), 1024)
    g_coarse = api.budget_index(1e-2)
    m = 1e-7 * ref.absmax
    assert ref.R(g_coarse) > m and ref.solve(m, g_min=g_coarse)[0] is None
