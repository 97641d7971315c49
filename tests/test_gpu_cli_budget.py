"""wrenc --ratio=R (an encode to a byte budget, include/waverange_amd.h) on the GPU: every field's record fits its budget, the
tool prints the tolerance it chose, and wrdec -- which needs nothing new -- gives the CPU oracle's reconstruction at those
tolerances, bit for bit.  --ratio with another stream format is refused before anything is written."""
import os
import re

import numpy as np
import pytest

from test_gpu_cli_seg import WRDEC, WRENC, parse_wrh, read, run
from oracle.loader import Oracle
from waverange_amd import api, synth

pytestmark = pytest.mark.gpu

NX = NY = NZ = 32
RATIO = 8
TOL_MIN = "1e-12"
ARGS = ["data.bin", "data.wrb", "data.wrh", "2", "0", "2", "2", str(NX), str(NY), str(NZ), TOL_MIN]


def fields():
    return [synth.field(NX, NY, NZ, seed=s) for s in (21, 22)]


def test_wrenc_ratio_fits_every_field_and_wrdec_gives_the_oracles_decode(tmp_path):
    fs = fields()
    np.concatenate([f.ravel() for f in fs]).tofile(str(tmp_path / "data.bin"))
    r = run(WRENC, ["--ratio=%d" % RATIO, "--format=wrs1"] + ARGS, tmp_path)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    chosen = re.findall(r"Budget (\d+) bytes: relative tolerance (\S+) \(grid point (\d+)\), bound (\d+) bytes, coded (\d+) bytes", r.stdout)
    assert len(chosen) == 2, r.stdout[-2000:]
    budget = NX * NY * NZ * 8 // RATIO
    recs = parse_wrh(read(tmp_path / "data.wrh").decode())
    assert len(recs) == 2 and os.path.getsize(tmp_path / "data.wrb") == sum(f["ntot_enc"] for f in recs)
    g_min = api.budget_index(float(TOL_MIN))
    for rec, (b, tol, g, bound, coded) in zip(recs, chosen):
        assert int(b) == budget and rec["ntot_enc"] == int(coded) <= int(bound) <= budget
        assert float(tol) == api.budget_tol(int(g)) and g_min <= int(g) <= api.BUDGET_GMAX
    r = run(WRDEC, ["data.wrb", "data.wrh", "datarec.bin", "2", "0"], tmp_path)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.fromfile(str(tmp_path / "datarec.bin"), dtype=np.float64).reshape(2, NZ, NY, NX)
    o = Oracle()
    for k, (f, (_, tol, _, _, _)) in enumerate(zip(fs, chosen)):
        want = o.decode(o.encode(f, float(tol)), f.shape)
        assert np.array_equal(got[k].view(np.uint64), want.view(np.uint64)), k


@pytest.mark.parametrize("fmt", ["ref", "wrs2", "wrs3", None])
def test_wrenc_ratio_needs_wrs1(tmp_path, fmt):
    np.concatenate([f.ravel() for f in fields()]).tofile(str(tmp_path / "data.bin"))
    r = run(WRENC, ["--ratio=%d" % RATIO] + (["--format=" + fmt] if fmt else []) + ARGS, tmp_path)
    assert r.returncode == 2, (r.returncode, r.stdout[-500:])
    assert "--ratio needs --format=wrs1" in r.stdout
    assert sorted(os.listdir(tmp_path)) == ["data.bin"]


def test_wrenc_ratio_refuses_a_bad_number(tmp_path):
    np.zeros(8).tofile(str(tmp_path / "data.bin"))
    for bad in ("0", "0.5", "x", "", "-3", "nan"):
        r = run(WRENC, ["--ratio=" + bad, "--format=wrs1"] + ARGS, tmp_path)
        assert r.returncode == 2 and "--ratio" in r.stdout, (bad, r.returncode)
        assert sorted(os.listdir(tmp_path)) == ["data.bin"]
