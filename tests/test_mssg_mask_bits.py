"""wrenc_mssg --mask=bits / wrdec_mssg: the undefined points of MSSG regular output as a packed bit mask (a "mask" record whose
payload is a WRM1 blob) instead of a second coded field of doubles.  The masked regular-output case of tests/mssg_cases.py
(single precision, big endian, undefined points in two of three fields) through both paths in the WRS1 stream format: the
undefined points must come back as `undef` exactly, the defined ones within twice the run's tolabs of what the path without
the option restores (the two paths pad with means that differ in their last bits, so bit equality is not claimed), and the
payload file must be smaller.  The option is refused with status 2, nothing written, without a segmented stream format and on
a codec library that lacks the masked calls."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import mssg_cases
from util import ROOT, build_cli, codec_library

BINDIR = os.path.join(ROOT, "waverange_amd", "bin")
CASE = "regout_f32_be_masked"


def run_pair(workdir, enc, dec, options, stream_format):
    """encoder then decoder on the case's inputs in workdir; returns the encoder's CompletedProcess (the decoder only runs
    after an encoder that succeeded)"""
    env = dict(os.environ, WR_QUIET="1")
    env.pop("WR_STREAM_FORMAT", None)
    if stream_format:
        env["WR_STREAM_FORMAT"] = stream_format
    argv, _, _ = mssg_cases.enc_invocation(CASE, 0)
    e = subprocess.run([enc] + options + argv, cwd=workdir, env=env, text=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    if e.returncode == 0:
        argv, _ = mssg_cases.dec_invocation(CASE, 0)
        subprocess.run([dec] + argv, cwd=workdir, env=env, text=True, check=True, stdout=subprocess.DEVNULL, timeout=120)
    return e


def field_tolabs(header_text):
    """tolabs of every record that is not a mask record, in file order"""
    lines = header_text.splitlines()
    out = []
    for k, l in enumerate(lines):
        if l.startswith(" Data set name = ") and l.strip() != "Data set name = mask":
            out.append(float(lines[k + 2]))
    return out


def restored(workdir):
    c = mssg_cases.CASES[CASE]
    a = np.fromfile(os.path.join(workdir, "dec_%s.grd" % c["prefix"]), dtype=">f4")
    return a.reshape(c["nt"], c["nz"], c["ny"], c["nx"])


@pytest.mark.gpu
def test_mask_bits_round_trip_against_the_path_without_the_option():
    enc, dec = os.path.join(BINDIR, "wrenc_mssg"), os.path.join(BINDIR, "wrdec_mssg")
    assert os.path.exists(enc) and os.path.exists(dec)
    c = mssg_cases.CASES[CASE]
    originals = np.stack(mssg_cases._regout_fields(c))
    und = originals < -1e30
    assert und[0].any() and not und[1].any() and und[2].any()
    with tempfile.TemporaryDirectory() as plain, tempfile.TemporaryDirectory() as bits:
        for d, options in ((plain, []), (bits, ["--mask=bits"])):
            mssg_cases.write_inputs(CASE, d)
            e = run_pair(d, enc, dec, options, "wrs1")
            assert e.returncode == 0, e.stdout + e.stderr
        a, b = restored(plain), restored(bits)
        payload = "%s_f.enc" % c["prefix"]
        size_plain, size_bits = (os.path.getsize(os.path.join(d, payload)) for d in (plain, bits))
        with open(os.path.join(bits, "%s_h.enc" % c["prefix"])) as fh:
            header = fh.read()
    undef32 = np.float32(mssg_cases.UNDEF)
    assert (b[und] == undef32).all() and (a[und] == undef32).all()
    assert not (b[~und] == undef32).any()
    assert header.count("Data set name = mask") == 2
    tolabs = field_tolabs(header)
    assert len(tolabs) == c["nt"]
    for it in range(c["nt"]):
        diff = np.abs(a[it].astype(np.float64) - b[it].astype(np.float64))[~und[it]].max()
        print("field %d: max |plain path - bits path| on defined points %.3g, tolabs %.3g" % (it, diff, tolabs[it]))
        assert diff <= 2 * tolabs[it]
    print("payload: %d bytes without the option, %d with it" % (size_plain, size_bits))
    assert size_bits < size_plain


def test_mask_bits_needs_a_segmented_stream_format():
    """(no GPU: the option is refused before a context is made)"""
    enc = os.path.join(BINDIR, "wrenc_mssg")
    assert os.path.exists(enc), "waverange_amd/bin/wrenc_mssg is not built"
    c = mssg_cases.CASES[CASE]
    for fmt in (None, "ref"):
        with tempfile.TemporaryDirectory() as d:
            before = sorted(mssg_cases.write_inputs(CASE, d))
            e = run_pair(d, enc, enc, ["--mask=bits"], fmt)
            assert e.returncode == 2, (e.returncode, e.stdout, e.stderr)
            assert "segmented stream format" in e.stderr
            assert sorted(os.listdir(d)) == before, "a refused run writes nothing"
            assert not os.path.exists(os.path.join(d, "%s_h.enc" % c["prefix"]))


def test_mask_bits_on_a_codec_library_without_the_masked_calls(tmp_path):
    """our front-end sources linked against the reference codec (or the oracle under its ABI): the new symbols are weak and null"""
    enc = build_cli("mssg_enc", codec_library(), str(tmp_path))
    work = tmp_path / "work"
    work.mkdir()
    before = sorted(mssg_cases.write_inputs(CASE, str(work)))
    e = run_pair(str(work), enc, enc, ["--mask=bits"], "wrs1")
    assert e.returncode == 2, (e.returncode, e.stdout, e.stderr)
    assert "not supported by this codec library" in e.stderr
    assert sorted(os.listdir(str(work))) == before
