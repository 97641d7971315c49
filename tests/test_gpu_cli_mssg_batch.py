"""wrdec_mssg --batch=N: up to N consecutive time records of a partial decode (--level / --roi / --planes) through one call of
wr_decode_host_seg_roi_batch_masked.  A small MSSG regular-output set by the fixtures' recipe (tests/mssg_cases.py: single
precision, big endian, land as `undef`) with 6 time records, four of them with undefined points, coded with --mask=bits in
WRS1 and in WRS3: the file a --batch run writes is byte for byte the file of --batch=1, the default and the loop over the
records.  --batch without a partial option ends with status 2."""
import os
import subprocess

import numpy as np
import pytest

import mssg_cases
from util import ROOT, build_cli, codec_library
from waverange_amd import synth

BINDIR = os.path.join(ROOT, "waverange_amd", "bin")
ENC, DEC = os.path.join(BINDIR, "wrenc_mssg"), os.path.join(BINDIR, "wrdec_mssg")
SET = dict(prefix="n_tm", nx=40, ny=24, nz=8, nt=6, masked=[0, 2, 3, 5], tol="1e-5")


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


def decode(workdir, out, options, fmt):
    argv = [SET["prefix"], ".enc", out, "0", "1", "1", "0"]
    r = subprocess.run([DEC] + options + argv, cwd=workdir, env=env_of(fmt), text=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    path = os.path.join(workdir, out + ".grd")
    return r, (open(path, "rb").read() if os.path.exists(path) else None)


@pytest.fixture(scope="module", params=["wrs1", "wrs3:seg=1024:strands=4"], ids=["wrs1", "wrs3"])
def coded(request, tmp_path_factory):
    assert os.path.exists(ENC) and os.path.exists(DEC), "waverange_amd/bin/wrenc_mssg and wrdec_mssg are not built"
    d = str(tmp_path_factory.mktemp("mssg_batch"))
    write_set(d)
    argv = [SET["prefix"], ".enc", "0", "1", "1", SET["tol"], "0"]
    e = subprocess.run([ENC, "--mask=bits"] + argv, cwd=d, env=env_of(request.param), text=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert e.returncode == 0, e.stdout + e.stderr
    with open(os.path.join(d, SET["prefix"] + "_h.enc")) as fh:
        assert fh.read().count("Data set name = mask") == len(SET["masked"])
    return d, request.param


@pytest.mark.gpu
@pytest.mark.parametrize("name,options,batch", [("roi", ["--roi=3:20,2:20,1:7"], 4), ("level2", ["--level=2"], 6), ("roi_level1_planes1", ["--roi=1:9,0:5,2:3", "--level=1", "--planes=1"], 2),
                                                ("probe", ["--roi=12:13,9:10,4:5"], 6)])
def test_batch_writes_the_file_of_the_loop(coded, name, options, batch):
    d, fmt = coded
    one, f1 = decode(d, "one_" + name, options + ["--batch=1"], fmt)
    dflt, f0 = decode(d, "dflt_" + name, options, fmt)
    many, fn = decode(d, "many_" + name, options + ["--batch=%d" % batch], fmt)
    for r in (one, dflt, many):
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert f1 is not None and len(f1) > 0 and f1 == f0
    assert fn == f1
    # the land comes back as undef in the batch run too
    if name == "roi":
        a = np.frombuffer(fn, ">f4").reshape(SET["nt"], 6, 18, 17)
        want = np.stack([f[1:7, 2:20, 3:20] for f in fields()]) < -1e30
        assert want.any() and np.array_equal(a == np.float32(mssg_cases.UNDEF), want)
    assert many.stdout.count("  wrote: ") == SET["nt"] == one.stdout.count("  wrote: ")


def test_batch_needs_a_partial_option(tmp_path):
    """(no GPU: refused before a file is opened)"""
    assert os.path.exists(DEC), "waverange_amd/bin/wrdec_mssg is not built"
    for options in (["--batch=4"], ["--batch=1"]):
        r, f = decode(str(tmp_path), "out", options, "wrs1")
        assert r.returncode == 2 and f is None, (r.returncode, r.stdout, r.stderr)
        assert "--batch" in r.stderr and "--level" in r.stderr
    for options in (["--batch=0", "--level=1"], ["--batch=x", "--level=1"]):
        r, f = decode(str(tmp_path), "out", options, "wrs1")
        assert r.returncode == 2 and f is None and "bad option" in r.stderr
    assert os.listdir(str(tmp_path)) == []


def test_batch_on_a_codec_library_without_the_call(tmp_path):
    """our front-end sources linked against the reference codec (or the oracle under its ABI): the new symbols are weak and null"""
    dec = build_cli("mssg_dec", codec_library(), str(tmp_path))
    work = tmp_path / "work"
    work.mkdir()
    argv = [SET["prefix"], ".enc", "out", "0", "1", "1", "0"]
    r = subprocess.run([dec, "--level=1", "--batch=4"] + argv, cwd=str(work), env=env_of("wrs1"), text=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 2, (r.returncode, r.stdout, r.stderr)
    assert "--batch is not supported by this codec library" in r.stderr
    assert os.listdir(str(work)) == []
