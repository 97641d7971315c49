"""wrenc_mssg --mask=bits --maxerr=E | --rmse=E | --psnr=DB: MSSG regular output coded to a target that is taken over the DEFINED
points.  The masked regular-output case of tests/mssg_cases.py (single precision, big endian, undefined points in two of three
fields) in the WRS1 stream format, then wrdec_mssg: the undefined points come back as `undef` exactly, the defined ones within
the target of the input, and the payload file is, record for record, what wr_encode_host_seg_quality_masked returns for the same
field.  The exclusions, a bad number, the option without --mask=bits and a missing segmented format exit with status 2 before
anything is written.

The decoder writes single precision, as the input was: a restored point is the fp64 reconstruction rounded to float.  The fields
lie in [256, 512), where a float's ulp is 2^-15, so the pointwise check allows E + 2^-16."""
import math
import os
import tempfile

import numpy as np
import pytest

import mssg_cases
from test_mssg_mask_bits import BINDIR, CASE, restored, run_pair
from waverange_amd import api

ENC, DEC = os.path.join(BINDIR, "wrenc_mssg"), os.path.join(BINDIR, "wrdec_mssg")
HALF_ULP = 2.0 ** -16
UNDEF_TEXT = "-9.99E33"  # as the control file spells it


def inputs():
    """(the fields as the tool reads them: float32 widened to fp64, shaped (nt, nz, ny, nx); the undefined set; the tool's threshold)"""
    c = mssg_cases.CASES[CASE]
    f = np.stack(mssg_cases._regout_fields(c)).astype(np.float32).astype(np.float64)
    u = float(UNDEF_TEXT)
    below = u + abs(u) * 1e-4  # mssg_io.h: kMaskThresholdAcc
    und = f < below
    assert und[0].any() and not und[1].any() and und[2].any()
    assert 256.0 <= f[~und].min() and f[~und].max() < 512.0
    return c, f, und, below


def run_tool(options):
    c = mssg_cases.CASES[CASE]
    with tempfile.TemporaryDirectory() as d:
        mssg_cases.write_inputs(CASE, d)
        e = run_pair(d, ENC, DEC, options, "wrs1")
        assert e.returncode == 0, e.stdout + e.stderr
        with open(os.path.join(d, "%s_f.enc" % c["prefix"]), "rb") as fh:
            payload = np.frombuffer(fh.read(), np.uint8)
        return e.stdout, payload, restored(d).astype(np.float64)


@pytest.mark.gpu
@pytest.mark.parametrize("option,norm,target", [("--maxerr=1e-2", api.NORM_MAX, 1e-2), ("--psnr=50", api.NORM_PSNR, 50.0), ("--rmse=2e-3", api.NORM_RMS, 2e-3)])
def test_target_over_the_defined_points_through_the_tools(option, norm, target):
    c, f, und, below = inputs()
    stdout, payload, back = run_tool(["--mask=bits", option])
    assert np.all(back[und] == np.float64(np.float32(mssg_cases.UNDEF)))
    api.set_verbosity(0)
    want = []
    with api.Context(0) as ctx:
        for it in range(c["nt"]):
            info, data, res = ctx.encode_host_seg_quality_masked(np.ascontiguousarray(f[it]), norm, target, below, tol_min=float(c["tol"]))
            nt = info["ntot_enc"]
            want += [data[nt:].copy(), data[:nt].copy()]  # the "mask" record goes first in the container
            assert (info["mask"]["undefined"] > 0) == bool(und[it].any())
            D = ~und[it]
            d = f[it][D] - back[it][D]
            lo, hi = f[it][D].min(), f[it][D].max()
            print(option, "field", it, "g", res["g"], "max", np.abs(d).max(), "rms", math.sqrt(np.mean(d * d)), "library", res["max_abs"], res["rms"])
            if norm == api.NORM_MAX:
                assert res["max_abs"] <= target and np.abs(d).max() <= target + HALF_ULP
            else:
                m = target if norm == api.NORM_RMS else api.psnr_rms(target, lo, hi)
                assert res["max_rms"] == m and res["rms"] <= m
                assert math.sqrt(np.mean(d * d)) <= m + HALF_ULP  # (the rounding to float moves every point by at most 2^-16)
            assert ("grid point %d)" % res["g"]) in stdout and ("%.17g" % res["tolrel"]) in stdout and ("%.17g" % res["max_abs"]) in stdout
    assert np.array_equal(payload, np.concatenate(want))
    assert stdout.count("over the defined points") == c["nt"]


@pytest.mark.parametrize("options,message", [
    (["--mask=bits", "--maxerr=1e-2", "--psnr=60"], "--maxerr and --psnr exclude one another"),
    (["--mask=bits", "--psnr=60", "--rmse=1e-3"], "--psnr and --rmse exclude one another"),
    (["--mask=bits", "--rmse=1e-3", "--maxerr=1e-3"], "--rmse and --maxerr exclude one another"),
    (["--mask=bits", "--maxerr=0"], "--maxerr=0: a positive number is required"),
    (["--mask=bits", "--rmse=nan"], "a positive number is required"),
    (["--mask=bits", "--psnr=60dB"], "a positive number is required"),
    (["--mask=bits", "--psnr="], "a positive number is required"),
    (["--maxerr=1e-2"], "--maxerr needs --mask=bits"),
    (["--psnr=60"], "--psnr needs --mask=bits")])
def test_bad_target_options_are_refused_before_anything_is_written(options, message):
    """(no GPU: the options are judged before a context is made)"""
    assert os.path.exists(ENC), "waverange_amd/bin/wrenc_mssg is not built"
    with tempfile.TemporaryDirectory() as d:
        before = sorted(mssg_cases.write_inputs(CASE, d))
        e = run_pair(d, ENC, ENC, options, "wrs1")
        assert e.returncode == 2, (e.returncode, e.stdout, e.stderr)
        assert message in e.stderr, e.stderr
        assert sorted(os.listdir(d)) == before


@pytest.mark.parametrize("fmt", [None, "ref"])
@pytest.mark.parametrize("option", ["--maxerr=1e-2", "--rmse=1e-3", "--psnr=60"])
def test_target_options_need_a_segmented_stream_format(option, fmt):
    with tempfile.TemporaryDirectory() as d:
        before = sorted(mssg_cases.write_inputs(CASE, d))
        e = run_pair(d, ENC, ENC, ["--mask=bits", option], fmt)
        assert e.returncode == 2, (e.returncode, e.stdout, e.stderr)
        assert "segmented stream format" in e.stderr
        assert sorted(os.listdir(d)) == before
