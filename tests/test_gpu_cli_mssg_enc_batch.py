"""wrenc_mssg --mask=bits --batch=N: up to N consecutive TYPE 0 time records through one call of
wr_encode_host_seg_batch_masked.  The small MSSG regular-output set of test_gpu_cli_mssg_batch.py's recipe (tests/mssg_cases.py:
single precision, big endian, land as `undef`; 40 x 24 x 8, 6 time records, four of them with undefined points), in WRS1 and
in WRS3: the two files a --batch run writes are byte for byte those of the run without the option -- groups of 4 and 2, one
group of 6, and --batch=1.  The refusals end with status 2 before a file is opened."""
import os
import subprocess

import numpy as np
import pytest

import mssg_cases
from util import ROOT, build_cli, codec_library
from waverange_amd import synth

BINDIR = os.path.join(ROOT, "waverange_amd", "bin")
ENC = os.path.join(BINDIR, "wrenc_mssg")
SET = dict(prefix="n_tm", nx=40, ny=24, nz=8, nt=6, masked=[0, 2, 3, 5], tol="1e-5")
ARGV = [SET["prefix"], ".enc", "0", "1", "1", SET["tol"], "0"]


def fields():
    out = []
    for it in range(SET["nt"]):
        f = synth.field(SET["nx"], SET["ny"], SET["nz"], seed=500 + it) * 3.0 + 280.0
        if it in SET["masked"]:
            z, y, x = np.meshgrid(np.arange(SET["nz"]), np.arange(SET["ny"]), np.arange(SET["nx"]), indexing="ij")
            land = ((x - 11) ** 2 + (y - 9) ** 2 < 30 + 4 * it) | ((x > 30) & (y < 5 + z))
            f = np.where(land, mssg_cases.UNDEF, f)
        out.append(f)
    return out


def write_set(workdir):
    p = SET["prefix"]
    ctl = ("DSET ^%s.grd\nTITLE synthetic MSSG regular output\nOPTIONS big_endian\nUNDEF %s\n"
           "XDEF %d LINEAR 0.0 1.0\nYDEF %d LINEAR 0.0 1.0\nZDEF %d LEVELS 1 2 3\nTDEF %d LINEAR 00Z01JAN2000 1hr\n"
           "VARS 1\nt %d 99 temperature\nENDVARS\n" % (p, "-9.99E33", SET["nx"], SET["ny"], SET["nz"], SET["nt"], SET["nz"]))
    with open(os.path.join(workdir, p + ".ctl"), "w") as fh:
        fh.write(ctl)
    with open(os.path.join(workdir, p + ".grd"), "wb") as fh:
        for f in fields():
            fh.write(np.ascontiguousarray(f).astype(">f4").tobytes())


def env_of(fmt):
    env = dict(os.environ, WR_QUIET="1")
    env["WR_STREAM_FORMAT"] = fmt
    return env


def encode(workdir, options, fmt, exe=ENC):
    r = subprocess.run([exe] + options + ARGV, cwd=workdir, env=env_of(fmt), text=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    out = []
    for tail in ("_h.enc", "_f.enc"):
        path = os.path.join(workdir, SET["prefix"] + tail)
        out.append(open(path, "rb").read() if os.path.exists(path) else None)
    return r, out


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["wrs1", "wrs3:seg=1024:strands=4"], ids=["wrs1", "wrs3"])
def test_batch_writes_the_files_of_the_loop(fmt, tmp_path):
    assert os.path.exists(ENC), "waverange_amd/bin/wrenc_mssg is not built"
    runs = {}
    for name, options in [("loop", []), ("b4", ["--batch=4"]), ("b6", ["--batch=6"]), ("b1", ["--batch=1"])]:
        d = tmp_path / name
        d.mkdir()
        write_set(str(d))
        r, files = encode(str(d), ["--mask=bits"] + options, fmt)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        runs[name] = (r, files)
    want = runs["loop"][1]
    assert want[0] and want[1] and want[0].count(b"Data set name = mask") == len(SET["masked"])
    for name in ("b4", "b6", "b1"):
        assert runs[name][1][0] == want[0], name + ": _h.enc differs"
        assert runs[name][1][1] == want[1], name + ": _f.enc differs"
    assert runs["b4"][0].stdout.count("coded in a batch of 4") == 4 and runs["b4"][0].stdout.count("coded in a batch of 2") == 2
    assert runs["b6"][0].stdout.count("coded in a batch of 6") == 6
    assert "coded in a batch" not in runs["b1"][0].stdout


def test_refusals(tmp_path):
    """(no GPU: refused before a file is opened)"""
    assert os.path.exists(ENC), "waverange_amd/bin/wrenc_mssg is not built"
    d = str(tmp_path)
    for options, word in [(["--batch=4"], "--mask=bits"), (["--mask=bits", "--batch=0"], "--batch=0"), (["--mask=bits", "--batch=x"], "--batch=x"),
                          (["--mask=bits", "--batch=4", "--maxerr=0.1"], "--maxerr"), (["--mask=bits", "--rmse=0.1", "--batch=4"], "--rmse"),
                          (["--mask=bits", "--batch=4", "--psnr=60"], "--psnr")]:
        r, files = encode(d, options, "wrs1")
        assert r.returncode == 2 and files == [None, None], (options, r.returncode, r.stdout, r.stderr)
        assert "--batch" in r.stderr and word in r.stderr, (options, r.stderr)
    assert os.listdir(d) == []


def test_batch_on_a_codec_library_without_the_call(tmp_path):
    """our front-end sources linked against the reference codec (or the oracle under its ABI): the new symbols are weak and null"""
    enc = build_cli("mssg_enc", codec_library(), str(tmp_path))
    work = tmp_path / "work"
    work.mkdir()
    r, files = encode(str(work), ["--mask=bits", "--batch=4"], "wrs1", exe=enc)
    assert r.returncode == 2 and files == [None, None], (r.returncode, r.stdout, r.stderr)
    assert "--batch is not supported by this codec library" in r.stderr
    assert os.listdir(str(work)) == []
