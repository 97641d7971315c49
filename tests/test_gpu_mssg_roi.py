"""wrdec_mssg --level / --roi / --planes: a region (or the low-resolution box) of every time record of MSSG regular output.  The
masked regular-output case of tests/mssg_cases.py (40 x 24 x 8, three records, two of them masked) encoded with
WR_STREAM_FORMAT=wrs1 and --mask=bits: the region's OUT.grd is the crop of the full wrdec_mssg output byte for byte (both
narrow the same fp64 bits), and at --level=1 the undefined points are exactly und[::2, ::2, ::2].  Without a GPU: the options
are refused with status 2, nothing written, on a set in the reference's stream format, for TYPE 1, and on a codec library
without the calls."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import mssg_cases
from util import ROOT, build_cli, codec_library

BINDIR = os.path.join(ROOT, "waverange_amd", "bin")
CASE = "regout_f32_be_masked"
ENV = dict(os.environ, WR_QUIET="1")


def run(exe, argv, cwd, stream_format=None, check=True):
    env = dict(ENV)
    env.pop("WR_STREAM_FORMAT", None)
    if stream_format:
        env["WR_STREAM_FORMAT"] = stream_format
    r = subprocess.run([exe] + argv, cwd=cwd, env=env, text=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    if check:
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def dec_argv(out_prefix=None, ftype=None):
    argv, _ = mssg_cases.dec_invocation(CASE, 0)
    if out_prefix:
        argv[2] = out_prefix
    if ftype is not None:
        argv[3] = str(ftype)
    return argv


@pytest.mark.gpu
def test_region_and_level_of_a_masked_set():
    enc, dec = os.path.join(BINDIR, "wrenc_mssg"), os.path.join(BINDIR, "wrdec_mssg")
    c = mssg_cases.CASES[CASE]
    nt, nz, ny, nx = c["nt"], c["nz"], c["ny"], c["nx"]
    und = np.stack(mssg_cases._regout_fields(c)) < -1e30
    assert und[0].any() and not und[1].any() and und[2].any()
    with tempfile.TemporaryDirectory() as d:
        mssg_cases.write_inputs(CASE, d)
        run(enc, ["--mask=bits"] + mssg_cases.enc_invocation(CASE, 0)[0], d, "wrs1")
        run(dec, dec_argv(), d)
        run(dec, ["--roi=5:29,2:20,1:7"] + dec_argv("roi"), d)
        r = run(dec, ["--level=1"] + dec_argv("low"), d)
        full = np.fromfile(os.path.join(d, "dec_%s.grd" % c["prefix"]), dtype=">f4").reshape(nt, nz, ny, nx)
        roi = np.fromfile(os.path.join(d, "roi.grd"), dtype=">f4")
        low = np.fromfile(os.path.join(d, "low.grd"), dtype=">f4")
        assert not os.path.exists(os.path.join(d, "roi.ctl")) and not os.path.exists(os.path.join(d, "low.ctl"))
    want = np.ascontiguousarray(full[:, 1:7, 2:20, 5:29])
    assert roi.tobytes() == want.tobytes()
    assert "nx=20 ny=12 nz=4" in r.stdout
    low = low.reshape(nt, 4, 12, 20)
    undef32 = np.float32(mssg_cases.UNDEF)
    coarse = und[:, ::2, ::2, ::2]
    assert np.array_equal(low == undef32, coarse)
    assert np.isfinite(low[~coarse].astype(np.float64)).all() and (np.abs(low[~coarse]) < 1e30).all()


def listing(d):
    return sorted(os.listdir(d))


def test_options_need_a_segmented_set_and_type_0(tmp_path):
    """(no GPU: the run is refused before a context is made)  The set comes from our encoder front-end on the CPU codec, which
    writes the reference's stream format."""
    dec = os.path.join(BINDIR, "wrdec_mssg")
    assert os.path.exists(dec), "waverange_amd/bin/wrdec_mssg is not built"
    enc = build_cli("mssg_enc", codec_library(), str(tmp_path))
    work = tmp_path / "work"
    work.mkdir()
    mssg_cases.write_inputs(CASE, str(work))
    run(enc, mssg_cases.enc_invocation(CASE, 0)[0], str(work))
    before = listing(str(work))
    for options in (["--roi=5:29,2:20,1:7"], ["--level=1"], ["--planes=1"]):
        r = run(dec, options + dec_argv(), str(work), check=False)
        assert r.returncode == 2, (r.returncode, r.stdout[-2000:], r.stderr)
        assert "mask record of the old kind" in r.stderr or "segmented stream format" in r.stderr
        assert listing(str(work)) == before, "a refused run writes nothing"
    # TYPE 1
    r = run(dec, ["--level=1"] + dec_argv(ftype=1), str(work), check=False)
    assert r.returncode == 2 and "TYPE 0" in r.stderr, (r.returncode, r.stderr)
    assert listing(str(work)) == before
    # an option that does not parse
    for bad in ("--level=5", "--roi=1:2,3:4", "--planes=x", "--nonsense=1"):
        r = run(dec, [bad] + dec_argv(), str(work), check=False)
        assert r.returncode == 2, (bad, r.returncode)
        assert listing(str(work)) == before


def test_options_on_a_codec_library_without_the_calls(tmp_path):
    """our front-end sources linked against the reference codec (or the oracle under its ABI): the new symbols are weak and null"""
    lib = codec_library()
    enc, dec = build_cli("mssg_enc", lib, str(tmp_path)), build_cli("mssg_dec", lib, str(tmp_path))
    work = tmp_path / "work"
    work.mkdir()
    mssg_cases.write_inputs(CASE, str(work))
    run(enc, mssg_cases.enc_invocation(CASE, 0)[0], str(work))
    before = listing(str(work))
    r = run(dec, ["--roi=5:29,2:20,1:7"] + dec_argv(), str(work), check=False)
    assert r.returncode == 2, (r.returncode, r.stdout[-2000:], r.stderr)
    assert "not supported by this codec library" in r.stderr
    assert listing(str(work)) == before
    # and without the options the same program still decodes the set
    run(dec, dec_argv(), str(work))
