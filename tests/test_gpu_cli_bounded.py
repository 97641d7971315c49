"""wrenc --maxerr=E (an encode to a pointwise error bound, include/waverange_amd.h) on the GPU: the files are what the plain tool
writes at the tolerance the tool prints, and wrdec -- which needs nothing new -- gives a reconstruction within E of the input at
every sample that is the CPU oracle's, bit for bit.  --maxerr with the reference's stream format or together with --ratio is
refused before anything is written."""
import os
import re

import numpy as np
import pytest

from test_gpu_cli_seg import WRDEC, WRENC, parse_wrh, read, run
from oracle.loader import Oracle
from waverange_amd import api, synth

pytestmark = pytest.mark.gpu

NX, NY, NZ = 40, 36, 33
E = 1e-3
TOL_MIN = "1e-12"
ARGS = ["data.bin", "data.wrb", "data.wrh", "2", "0", "2", "2", str(NX), str(NY), str(NZ), TOL_MIN]
LINE = r"Error bound (\S+): relative tolerance (\S+) \(grid point (\d+)\), error (\S+), (\d+) trials, coded (\d+) bytes"


def fields():
    return [synth.field(NX, NY, NZ, seed=s) for s in (21, 22)]


@pytest.mark.parametrize("fmt", ["wrs1", "wrs3"])
def test_wrenc_maxerr_writes_the_plain_tools_files_and_wrdec_stays_within_the_bound(tmp_path, fmt):
    fs = fields()
    np.concatenate([f.ravel() for f in fs]).tofile(str(tmp_path / "data.bin"))
    r = run(WRENC, ["--maxerr=%r" % E, "--format=" + fmt] + ARGS, tmp_path)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    chosen = re.findall(LINE, r.stdout)
    assert len(chosen) == 2, r.stdout[-2000:]
    recs = parse_wrh(read(tmp_path / "data.wrh").decode())
    assert len(recs) == 2 and os.path.getsize(tmp_path / "data.wrb") == sum(f["ntot_enc"] for f in recs)
    g_min = api.budget_index(float(TOL_MIN))
    for rec, (bound, tol, g, err, trials, coded) in zip(recs, chosen):
        assert float(bound) == E and float(err) <= E and int(trials) >= 1 and rec["ntot_enc"] == int(coded)
        assert float(tol) == api.budget_tol(int(g)) and g_min <= int(g) <= api.BUDGET_GMAX
    # the plain tool at the printed tolerance, field by field (one cutoff serves all fields of a plain run)
    wrb, at = read(tmp_path / "data.wrb"), 0
    for k, (f, rec, (_, tol, _, _, _, _)) in enumerate(zip(fs, recs, chosen)):
        sub = tmp_path / ("plain%d" % k)
        sub.mkdir()
        f.tofile(str(sub / "data.bin"))
        p = run(WRENC, ["--format=" + fmt, "data.bin", "data.wrb", "data.wrh", "2", "0", "1", "2", str(NX), str(NY), str(NZ), tol], sub)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        plain = parse_wrh(read(sub / "data.wrh").decode())[0]
        same = [key for key in rec if key not in ("id", "vary")]  # (the record's number and its place in the header file)
        assert sorted(plain) == sorted(rec) and all(plain[key] == rec[key] for key in same), (k, plain, rec)
        assert read(sub / "data.wrb") == wrb[at:at + rec["ntot_enc"]], k
        at += rec["ntot_enc"]
    r = run(WRDEC, ["data.wrb", "data.wrh", "datarec.bin", "2", "0"], tmp_path)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.fromfile(str(tmp_path / "datarec.bin"), dtype=np.float64).reshape(2, NZ, NY, NX)
    o = Oracle()
    for k, (f, (_, tol, _, err, _, _)) in enumerate(zip(fs, chosen)):
        assert np.abs(got[k] - f).max() <= E and float(np.abs(got[k] - f).max()) == float(err), k
        want = o.decode(o.encode(f, float(tol)), f.shape)
        assert np.array_equal(got[k].view(np.uint64), want.reshape(f.shape).view(np.uint64)), k


@pytest.mark.parametrize("extra,message", [(["--format=ref"], "--maxerr needs --format=wrs1, wrs2 or wrs3"),
                                           (["--format=wrs1", "--ratio=8"], "--maxerr and --ratio exclude one another")])
def test_wrenc_maxerr_refusals(tmp_path, extra, message):
    np.concatenate([f.ravel() for f in fields()]).tofile(str(tmp_path / "data.bin"))
    r = run(WRENC, ["--maxerr=%r" % E] + extra + ARGS, tmp_path)
    assert r.returncode == 2, (r.returncode, r.stdout[-500:])
    assert message in r.stdout
    assert sorted(os.listdir(tmp_path)) == ["data.bin"]


def test_wrenc_maxerr_refuses_a_bad_number(tmp_path):
    np.zeros(8).tofile(str(tmp_path / "data.bin"))
    for bad in ("0", "x", "", "-3", "nan", "inf"):
        r = run(WRENC, ["--maxerr=" + bad, "--format=wrs1"] + ARGS, tmp_path)
        assert r.returncode == 2 and "--maxerr" in r.stdout, (bad, r.returncode)
        assert sorted(os.listdir(tmp_path)) == ["data.bin"]
