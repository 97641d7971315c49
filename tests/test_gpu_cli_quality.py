"""wrenc --rmse=E and --psnr=DB (an encode to an RMS error or PSNR target, include/waverange_amd.h) on the GPU: the report line of
every field is parsed, and wrdec -- which needs nothing new -- gives a field whose RMS error against the input, computed here
with math.fsum, is within the target and is the one the tool printed."""
import math
import os
import re

import numpy as np
import pytest

from test_gpu_cli_seg import WRDEC, WRENC, parse_wrh, read, run
from waverange_amd import api, synth

pytestmark = pytest.mark.gpu

NX, NY, NZ = 24, 20, 17
TOL_MIN = "1e-12"
ARGS = ["data.bin", "data.wrb", "data.wrh", "2", "0", "2", "2", str(NX), str(NY), str(NZ), TOL_MIN]
LINE = (r"(RMS error|PSNR) target (\S+): relative tolerance (\S+) \(grid point (\d+)\), rms (\S+) \(allowed (\S+)\), psnr (\S+) dB, "
        r"max error (\S+), (\d+) trials, coded (\d+) bytes")


def fields():
    return [synth.field(NX, NY, NZ, seed=s) for s in (31, 32)]


def rms_of(a, b):
    d = (a.astype(np.float64) - b.astype(np.float64)).ravel()
    return math.sqrt(math.fsum(d * d) / d.size)


@pytest.mark.parametrize("option,fmt", [("--rmse=0.001", "wrs1"), ("--psnr=70", "wrs3"), ("--psnr=55.5", "wrs2:brick=8")])
def test_wrenc_to_a_quality_target_and_wrdec_stays_within_it(tmp_path, option, fmt):
    fs = fields()
    np.concatenate([f.ravel() for f in fs]).tofile(str(tmp_path / "data.bin"))
    r = run(WRENC, [option, "--format=" + fmt] + ARGS, tmp_path)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    chosen = re.findall(LINE, r.stdout)
    assert len(chosen) == 2, r.stdout[-2000:]
    recs = parse_wrh(read(tmp_path / "data.wrh").decode())
    assert len(recs) == 2 and os.path.getsize(tmp_path / "data.wrb") == sum(f["ntot_enc"] for f in recs)
    r = run(WRDEC, ["data.wrb", "data.wrh", "datarec.bin", "2", "0"], tmp_path)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.fromfile(str(tmp_path / "datarec.bin"), dtype=np.float64).reshape(2, NZ, NY, NX)
    name, value = option[2:].split("=")
    g_min = api.budget_index(float(TOL_MIN))
    for k, (f, rec, (what, target, tol, g, rms, allowed, psnr, maxerr, trials, coded)) in enumerate(zip(fs, recs, chosen)):
        assert what == ("RMS error" if name == "rmse" else "PSNR") and float(target) == float(value)
        assert float(tol) == api.budget_tol(int(g)) and g_min <= int(g) <= api.BUDGET_GMAX
        assert int(trials) >= 1 and rec["ntot_enc"] == int(coded)
        rng = float(f.max() - f.min())
        allowed_here = float(value) if name == "rmse" else api.psnr_rms(float(value), float(f.min()), float(f.max()))
        assert float(allowed) == allowed_here, (k, allowed, allowed_here)
        measured = rms_of(f, got[k])
        assert measured <= float(allowed) and float(rms) <= float(allowed), (k, measured, allowed)
        assert abs(measured - float(rms)) <= 2.0 ** -36 * measured, (k, measured, rms)
        assert float(np.abs(f - got[k]).max()) == float(maxerr), k
        assert abs(float(psnr) - 20.0 * math.log10(rng / float(rms))) <= 1e-9, (k, psnr)
        if name == "psnr":
            assert float(psnr) >= float(value) - 1e-9
