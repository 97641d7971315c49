"""wrenc / wrdec and the drop-in symbols on the segmented stream formats (WRS1 / WRS2 / WRS3), on the GPU.

Expected values are the reference's own: the decoded files have the golden SHA-256 of the compiled reference CLI
(tests/golden/cli.json), the header text is the golden text, and the coded bytes of a field are what the library's explicit
entry point returns for it.  Partial decodes are compared with Context.decode_host_seg_roi / _lowres.  Every comparison is
equality of bytes."""
import hashlib
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import cli_cases
from util import GOLDEN, ROOT
from waverange_amd import api, synth

pytestmark = pytest.mark.gpu

BINDIR = os.path.join(ROOT, "waverange_amd", "bin")
REFDIR = os.path.join(ROOT, "oracle", "_ref")
WRENC, WRDEC = os.path.join(BINDIR, "wrenc"), os.path.join(BINDIR, "wrdec")
FORMATS = ["wrs1", "wrs2:brick=8", "wrs3:strands=8:seg=4096"]
SEGMENTED_FIRST_LINE = " ===== Header file for compressed data (segmented plane streams) ====="


@pytest.fixture(scope="module")
def golden_cli():
    with open(os.path.join(GOLDEN, "cli.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def ctx():
    api.set_verbosity(0)
    with api.Context(0) as c:
        yield c


def sha(b):
    return hashlib.sha256(b).hexdigest()


def read(path):
    with open(path, "rb") as fh:
        return fh.read()


def run(exe, args, cwd, stdin=None, **env):
    e = dict(os.environ, WR_QUIET="1")
    e.pop("WR_STREAM_FORMAT", None)
    e.update(env)
    return subprocess.run([exe] + list(args), cwd=str(cwd), input=stdin, capture_output=True, text=True, env=e, timeout=300)


def parse_wrh(text):
    """The field records of a .wrh text: dicts of the header values plus `vary`, the indices of the lines that hold ntot_enc
    and len_enc_vec (the only ones that depend on the stream format, with line 0)."""
    lines = text.split("\n")
    at, out = 6, []
    while at < len(lines) and lines[at] == " -----":
        f = dict(id=int(lines[at + 1]), nbytes=int(lines[at + 3]), recl=lines[at + 4], nx=int(lines[at + 5]), ny=int(lines[at + 6]),
                 nz=int(lines[at + 7]), nh=int(lines[at + 8]), idinv=int(lines[at + 9]), icomp=int(lines[at + 10]), vary=[], ntot_enc=0, nlay=0)
        at += 11
        if f["icomp"]:
            f.update(tolabs=float(lines[at + 1]), midval=float(lines[at + 2]), halfspanval=float(lines[at + 3]), wlev=int(lines[at + 4]),
                     nlay=int(lines[at + 5]), ntot_enc=int(lines[at + 6]))
            f["vary"].append(at + 6)
            at += 7
            if f["ntot_enc"]:
                f["deps_vec"] = [float(v) for v in lines[at].split()]
                f["minval_vec"] = [float(v) for v in lines[at + 1].split()]
                f["len_enc_vec"] = [int(v) for v in lines[at + 2].split()]
                f["vary"].append(at + 2)
                at += 3
        f["wrb_bytes"] = f["ntot_enc"] if f["icomp"] else f["nbytes"] * f["nx"] * f["ny"] * f["nz"] * f["nh"]
        out.append(f)
    assert lines[at:] == [""], "unparsed tail of the header"
    return out


def same_header_but_the_lengths(text, golden_text):
    a, b = text.split("\n"), golden_text.split("\n")
    assert len(a) == len(b)
    vary = {0} | {i for f in parse_wrh(golden_text) for i in f["vary"]}
    assert vary == {0} | {i for f in parse_wrh(text) for i in f["vary"]}
    assert a[0] == SEGMENTED_FIRST_LINE
    diff = [i for i in range(len(a)) if a[i] != b[i] and i not in vary]
    assert not diff, [(i, a[i], b[i]) for i in diff[:3]]


def case_fields(case):
    """The fields of a case as the tool hands them to the codec: arrays shaped (nz * nh, ny, nx) of the record's precision."""
    out = []
    for fd in cli_cases.CASES[case]["fields"]:
        nbytes, nx, ny, nz, nh, idinv = fd["spec"]
        f = np.full((nz * nh, ny, nx), fd["constant"]) if "constant" in fd else synth.field(nx, ny, nz * nh, seed=fd["seed"])
        out.append(np.ascontiguousarray(f.astype(np.float32 if nbytes == 4 else np.float64)))
    return out


def format_args(fmt):
    """encode_host_seg's keywords for a format text."""
    f, seg, brick, strands = api.stream_format_parse(fmt)
    kw = dict(seg=seg)
    if f == api.FORMAT_WRS2 or (f == api.FORMAT_WRS3 and brick):
        kw["brick"] = brick
    if f == api.FORMAT_WRS3:
        kw["strands"] = strands
    return f, kw


_ENCODED = {}


def encoded(case, fmt, tmp_path_factory, through="option"):
    """One wrenc run per (case, format, way of saying the format): its directory, with data.bin / data.wrh / data.wrb."""
    key = (case, fmt, through)
    if key not in _ENCODED:
        d = tmp_path_factory.mktemp("enc")
        argv, stdin = cli_cases.write_inputs(case, str(d))
        r = run(WRENC, (["--format=" + fmt] if through == "option" else []) + argv, d, stdin,
                **({"WR_STREAM_FORMAT": fmt} if through == "env" else {}))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        if os.path.exists(d / "inmeta"):
            os.remove(d / "inmeta")
        _ENCODED[key] = d
    return _ENCODED[key]


# ---- 1. round trip per format -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(cli_cases.CASES))
@pytest.mark.parametrize("fmt", FORMATS)
def test_round_trip(fmt, case, golden_cli, ctx, tmp_path_factory):
    g = golden_cli[case]
    d = encoded(case, fmt, tmp_path_factory)
    assert sha(read(d / "data.bin")) == g["input_sha256"]
    text = read(d / "data.wrh").decode()
    same_header_but_the_lengths(text, g["wrh"])
    # the coded bytes of every field are the explicit entry point's
    wrb = np.frombuffer(read(d / "data.wrb"), dtype=np.uint8)
    records = parse_wrh(text)
    want_format, kw = format_args(fmt)
    tol = float(cli_cases.CASES[case]["fields"][-1]["tol"])  # (the tool applies the last field's tolerance to every field)
    at = 0
    for rec, f in zip(records, case_fields(case)):
        mine = wrb[at:at + rec["wrb_bytes"]]
        at += rec["wrb_bytes"]
        if not rec["icomp"]:
            assert mine.tobytes() == f.tobytes()
            continue
        enc, _ = (ctx.encode_host_seg_f32 if f.dtype == np.float32 else ctx.encode_host_seg)(f, tol, **kw)
        assert rec["ntot_enc"] == enc["ntot_enc"] and rec["nlay"] == enc["nlay"], rec["id"]
        if not rec["ntot_enc"]:
            continue
        assert rec["len_enc_vec"] == [int(v) for v in enc["len_enc_vec"]], rec["id"]
        assert np.array_equal(mine, enc["data"]), rec["id"]
        off = 0
        for ln in rec["len_enc_vec"]:  # every plane says the format
            assert api.stream_sniff(mine[off:off + ln]) == want_format
            off += ln
    assert at == wrb.size
    # and the decoded file is the reference's own reconstruction
    r = run(WRDEC, cli_cases.dec_argv(case), d)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rec_bytes = read(d / "datarec.bin")
    assert len(rec_bytes) == g["rec_size"] and sha(rec_bytes) == g["rec_sha256"]


# ---- 2. the same files through the environment ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(cli_cases.CASES))
@pytest.mark.parametrize("fmt", FORMATS)
def test_environment_variable_instead_of_the_option(fmt, case, tmp_path_factory):
    a, b = encoded(case, fmt, tmp_path_factory), encoded(case, fmt, tmp_path_factory, through="env")
    assert read(a / "data.wrb") == read(b / "data.wrb")
    assert read(a / "data.wrh") == read(b / "data.wrh")


def test_option_overrides_the_environment_and_a_bad_value_is_refused(golden_cli, tmp_path):
    argv, _ = cli_cases.write_inputs("config1_64cube", str(tmp_path))
    r = run(WRENC, ["--format=ref"] + argv, tmp_path, WR_STREAM_FORMAT="wrs1")
    assert r.returncode == 0
    assert read(tmp_path / "data.wrh").decode() == golden_cli["config1_64cube"]["wrh"]
    assert sha(read(tmp_path / "data.wrb")) == golden_cli["config1_64cube"]["wrb_sha256"]
    for name in ("data.wrb", "data.wrh"):
        os.remove(tmp_path / name)
    for args, env in ((["--format=wrs1:brick=8"], {}), ([], {"WR_STREAM_FORMAT": "wrs9"}), (["--bogus"], {})):
        r = run(WRENC, args + argv, tmp_path, **env)
        assert r.returncode == 2 and "usage:" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-500:])
        assert (args[0] if args and args[0] == "--bogus" else "brick=8" if args else "wrs9") in r.stdout
        assert not os.path.exists(tmp_path / "data.wrb") and not os.path.exists(tmp_path / "data.wrh")


# ---- 3. a file that mixes formats field by field --------------------------------------------------------------------------
def test_mixed_file(golden_cli, tmp_path, tmp_path_factory):
    case = "argv_two_fp32"
    ref, seg = encoded(case, "ref", tmp_path_factory), encoded(case, "wrs1", tmp_path_factory)
    assert read(ref / "data.wrh").decode() == golden_cli[case]["wrh"]
    parts = {}
    for name, d in (("ref", ref), ("seg", seg)):
        text = read(d / "data.wrh").decode()
        recs, lines, wrb = parse_wrh(text), text.split("\n"), read(d / "data.wrb")
        starts = [i for i, l in enumerate(lines) if l == " -----"] + [len(lines) - 1]
        parts[name] = dict(pre=lines[:starts[0]], rec=[lines[starts[k]:starts[k + 1]] for k in range(2)],
                           bytes=[wrb[:recs[0]["wrb_bytes"]], wrb[recs[0]["wrb_bytes"]:]])
    with open(tmp_path / "data.wrh", "w") as fh:
        fh.write("\n".join(parts["seg"]["pre"] + parts["ref"]["rec"][0] + parts["seg"]["rec"][1]) + "\n")
    with open(tmp_path / "data.wrb", "wb") as fh:
        fh.write(parts["ref"]["bytes"][0] + parts["seg"]["bytes"][1])
    assert api.stream_sniff(parts["ref"]["bytes"][0]) == 0 and api.stream_sniff(parts["seg"]["bytes"][1]) == 1
    r = run(WRDEC, cli_cases.dec_argv(case), tmp_path)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert sha(read(tmp_path / "datarec.bin")) == golden_cli[case]["rec_sha256"]


# ---- 4. the drop-in symbols from Python (a child process: the setting is process-wide) ------------------------------------
DROPIN = r"""
import sys; sys.path.insert(0, %r)
import numpy as np
from waverange_amd import api, synth
from oracle.loader import Oracle
api.set_verbosity(0)
o = Oracle()
f = synth.field(40, 36, 28, seed=77)
want = o.encode(f, 1e-6)
want_rec = o.decode(want, f.shape)
assert api.stream_format() == (0, 0, 0, 0)
api.set_stream_format("wrs2:brick=16")
enc = api.encoding_wrap(f, 1e-6)
with api.Context(0) as c:
    seg, _ = c.encode_host_seg(f, 1e-6, brick=16)
    assert enc["len_enc_vec"] == [int(v) for v in seg["len_enc_vec"]] and np.array_equal(enc["data"], seg["data"]), "coded bytes"
assert api.stream_sniff(enc["data"]) == api.FORMAT_WRS2
for k in ("tolabs", "midval", "halfspanval", "wlev", "nlay"):
    assert enc[k] == want[k], k
assert np.array_equal(enc["deps_vec"], want["deps_vec"]) and np.array_equal(enc["minval_vec"], want["minval_vec"])
rec = api.decoding_wrap(enc, f.shape)   # the decoder reads what the bytes say, whatever the setting
assert np.array_equal(rec.view(np.uint64), want_rec.view(np.uint64)), "reconstruction of the segmented stream"
rec = api.decoding_wrap(want, f.shape)
assert np.array_equal(rec.view(np.uint64), want_rec.view(np.uint64)), "reconstruction of the reference stream, setting wrs2"
api.set_stream_format(None)
back = api.encoding_wrap(f, 1e-6)
assert back["len_enc_vec"] == want["len_enc_vec"] and np.array_equal(back["data"], want["data"]), "the reference's bytes again"
assert np.array_equal(back["residual"].view(np.uint64), enc["residual"].view(np.uint64)), "the residual a segmented encode writes back"
assert not np.array_equal(back["residual"].view(np.uint64), f.view(np.uint64))
rec = api.decoding_wrap(enc, f.shape)
assert np.array_equal(rec.view(np.uint64), want_rec.view(np.uint64)), "reconstruction of the segmented stream, setting ref"
print("ok")
""" % ROOT


def test_drop_in_symbols_from_python(tmp_path):
    script = tmp_path / "child.py"
    script.write_text(DROPIN)
    env = dict(os.environ)
    env.pop("WR_STREAM_FORMAT", None)
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-3000:]


# ---- 5. partial decode -----------------------------------------------------------------------------------------------------
SHAPE = (24, 400, 40)                    # (nz, ny, nx) of synth.field(40, 400, 24)
ROI = ((0, 24), (0, 4), (0, 40))         # tests/test_gpu_roi.py::REGIONS[SHAPE]; on the command line x, y, z: 0:40,0:4,0:24
ROI_TEXT = "--roi=0:40,0:4,0:24"
PARTIAL_FORMATS = {"wrs1:seg=4096": (94, 72, 11), "wrs2:seg=4096:brick=8": (94, 38, 2)}   # nseg, needed by the region, by level 2


def test_pinned_segment_counts():
    """"Fewer than all" as a stated condition: what the geometry lists for the two partial decodes below (the WRS1 region count
    is tests/test_gpu_roi.py::CUT's)."""
    n = SHAPE[0] * SHAPE[1] * SHAPE[2]
    assert -(-n // 4096) == 94
    assert api.seg_roi_segments(SHAPE, 0, ROI, 4096).size == 72
    assert api.seg_lowres_segments(SHAPE, 2, 4096).size == 11
    assert api.seg_roi_segments_blocked(SHAPE, 0, ROI, seg=4096, brick=8).size == 38
    assert api.seg_lowres_segments_blocked(SHAPE, 2, seg=4096, brick=8).size == 2


def needed_ids(fmt, what):
    brick = api.stream_format_parse(fmt)[2]
    if what == "roi":
        return api.seg_roi_segments_blocked(SHAPE, 0, ROI, seg=4096, brick=brick) if brick else api.seg_roi_segments(SHAPE, 0, ROI, 4096)
    return api.seg_lowres_segments_blocked(SHAPE, 2, seg=4096, brick=brick) if brick else api.seg_lowres_segments(SHAPE, 2, 4096)


def masked(data, lens, need_of_plane):
    """The `masked` construction of tests/test_gpu_roi.py for WRS1 and WRS2 blobs: every byte of every segment that plane's list
    does not name is 0xFF; headers and indices stay."""
    data = data.copy()
    at = 0
    for l, ln in enumerate(lens):
        head = 12 if bytes(data[at:at + 4]) == b"WRS1" else 16
        nseg = int(data[at + 8:at + 12].view("<u4")[0])
        seglens = data[at + head:at + head + 4 * nseg].view("<u4").astype(np.int64)
        start = at + head + 4 * nseg + np.concatenate(([0], np.cumsum(seglens)))
        keep = np.zeros(nseg, dtype=bool)
        keep[need_of_plane(l)] = True
        for k in np.flatnonzero(~keep):
            data[start[k]:start[k + 1]] = 0xFF
        at += ln
    return data


def partial_file(fmt, dtype, file_type, tmp_path_factory):
    """data.bin / data.wrh / data.wrb of the one-field file, made by wrenc --format=fmt; cached per key."""
    key = ("partial", fmt, np.dtype(dtype).name, file_type)
    if key not in _ENCODED:
        d = tmp_path_factory.mktemp("partial")
        f = synth.field(40, 400, 24).astype(dtype)
        payload = f.tobytes()
        marker = struct.pack("<i", len(payload)) if file_type == 0 else b""
        with open(d / "data.bin", "wb") as fh:
            fh.write(marker + payload + marker)
        r = run(WRENC, ["--format=" + fmt, "data.bin", "data.wrb", "data.wrh", str(file_type), "0", "1", "1" if f.dtype == np.float32 else "2",
                        "40", "400", "24", "1e-6"], d)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        _ENCODED[key] = d
    return _ENCODED[key]


def records_of(path, file_type, dtype):
    """The records of an output file as flat arrays (file type 0: the markers are checked against the payload)."""
    raw = read(path)
    if file_type == 2:
        return [np.frombuffer(raw, dtype=dtype)]
    out, at = [], 0
    while at < len(raw):
        n = struct.unpack_from("<i", raw, at)[0]
        assert struct.unpack_from("<i", raw, at + 4 + n)[0] == n, "record markers differ"
        out.append(np.frombuffer(raw[at + 4:at + 4 + n], dtype=dtype))
        at += 8 + n
    return out


_WANT = {}


def expected_partial(ctx, fmt, dtype):
    """The field's stream from the explicit entry point and what the library's own partial decodes return for it: the expected
    bits, computed once per (format, precision) and never written to."""
    key = (fmt, np.dtype(dtype).name)
    if key not in _WANT:
        f = synth.field(40, 400, 24).astype(dtype)
        f32 = f.dtype == np.float32
        enc, _ = (ctx.encode_host_seg_f32 if f32 else ctx.encode_host_seg)(f, 1e-6, **format_args(fmt)[1])
        enc["data"] = enc["data"].copy()
        roi_call, low_call = (ctx.decode_host_seg_roi_f32, ctx.decode_host_seg_lowres_f32) if f32 else (ctx.decode_host_seg_roi, ctx.decode_host_seg_lowres)
        want = {}
        for planes in (0, 1):
            a, b = np.empty(api.roi_shape(ROI), dtype=dtype), np.empty(api.lowres_shape(SHAPE, 2), dtype=dtype)
            roi_call(a, SHAPE, 0, ROI, enc, planes)
            low_call(b, SHAPE, 2, enc, planes)
            want["roi", planes], want["level", planes] = a, b
        assert not np.array_equal(want["roi", 0], want["roi", 1]) and not np.array_equal(want["level", 0], want["level", 1])
        _WANT[key] = enc, want
    return _WANT[key]


VARIANTS = {"roi": ("roi", 0, [ROI_TEXT]), "level2": ("level", 0, ["--level=2"]), "roi_one_plane": ("roi", 1, [ROI_TEXT, "--planes=1"]),
            "level2_one_plane": ("level", 1, ["--planes=1", "--level=2", "--field=0"])}


def partial_run(d, work, options, file_type, dtype, wrb=None):
    work.mkdir()
    os.symlink(d / "data.wrh", work / "data.wrh")
    if wrb is None:
        os.symlink(d / "data.wrb", work / "data.wrb")
    else:
        wrb.tofile(work / "data.wrb")
    r = run(WRDEC, options + ["data.wrb", "data.wrh", "datarec.bin", str(file_type), "0"], work)
    assert r.returncode == 0, (options, r.stdout[-2000:], r.stderr[-2000:])
    assert "partial decode, field 0" in r.stdout and "idinv is not applied" in r.stdout
    recs = records_of(work / "datarec.bin", file_type, dtype)
    assert len(recs) == 1
    return recs[0]


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("fmt", sorted(PARTIAL_FORMATS))
def test_partial_decode(fmt, variant, ctx, tmp_path_factory, tmp_path):
    """wrdec's partial output is the library's, bit for bit -- also from a file in which only the segments that this decode
    needs survive, which a full decode refuses."""
    d = partial_file(fmt, np.float64, 2, tmp_path_factory)
    enc, want = expected_partial(ctx, fmt, np.float64)
    assert np.array_equal(np.frombuffer(read(d / "data.wrb"), dtype=np.uint8), enc["data"])
    nseg, need_roi, need_low = PARTIAL_FORMATS[fmt]
    what, planes, options = VARIANTS[variant]
    ids = needed_ids(fmt, what)
    assert ids.size == (need_roi if what == "roi" else need_low) and ids.size < nseg
    assert partial_run(d, tmp_path / "whole", options, 2, np.float64).tobytes() == want[what, planes].tobytes()
    bad = masked(enc["data"], [int(v) for v in enc["len_enc_vec"]], lambda l: ids if (planes == 0 or l < planes) else [])
    assert not np.array_equal(bad, enc["data"])
    assert partial_run(d, tmp_path / "damaged", options, 2, np.float64, bad).tobytes() == want[what, planes].tobytes()
    if variant == "roi":  # a full decode needs every segment: it fails, with a message and status 1
        r = run(WRDEC, ["data.wrb", "data.wrh", "full.bin", "2", "0"], tmp_path / "damaged")
        assert r.returncode == 1 and "field 0" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


@pytest.mark.parametrize("variant", ["roi", "level2"])
def test_partial_decode_fp32_record(variant, ctx, tmp_path_factory, tmp_path):
    """A 4-byte record goes through the _f32 calls and comes out as a 4-byte record."""
    fmt = "wrs1:seg=4096"
    d = partial_file(fmt, np.float32, 2, tmp_path_factory)
    enc, want = expected_partial(ctx, fmt, np.float32)
    assert np.array_equal(np.frombuffer(read(d / "data.wrb"), dtype=np.uint8), enc["data"])
    what, planes, options = VARIANTS[variant]
    got = partial_run(d, tmp_path / "whole", options, 2, np.float32)
    assert got.dtype == np.float32 and got.tobytes() == want[what, planes].tobytes()


def test_partial_decode_fortran_markers(ctx, tmp_path_factory, tmp_path):
    """File type 0: the record markers are recomputed for the region's byte count."""
    fmt = "wrs1:seg=4096"
    d = partial_file(fmt, np.float64, 0, tmp_path_factory)
    enc, want = expected_partial(ctx, fmt, np.float64)
    got = partial_run(d, tmp_path / "whole", [ROI_TEXT], 0, np.float64)   # (records_of checks the two markers against the payload)
    assert got.tobytes() == want["roi", 0].tobytes()
    raw = read(tmp_path / "whole" / "datarec.bin")
    nbytes = 40 * 4 * 24 * 8
    assert len(raw) == nbytes + 8 and struct.unpack("<i", raw[:4])[0] == nbytes == struct.unpack("<i", raw[-4:])[0]


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------
def test_partial_decode_refusals(golden_cli, tmp_path_factory, tmp_path):
    ref = encoded("config1_64cube", "ref", tmp_path_factory)
    seg = partial_file("wrs1:seg=4096", np.float64, 2, tmp_path_factory)
    many = encoded("inmeta_new_type0", "wrs1", tmp_path_factory)   # field 2 is stored uncompressed
    c = cli_cases.CASES["inmeta_new_type0"]
    for d, options, tail, field in ((ref, ["--roi=0:4,0:4,0:4"], ["2", "0"], 0),               # the reference's stream
                                    (many, ["--roi=0:1,0:1,0:1", "--field=2"], ["0", "0"], 2),   # icomp = 0
                                    (seg, ["--roi=0:41,0:4,0:24"], ["2", "0"], 0),               # past the box of level 0
                                    (seg, ["--roi=0:11,0:4,0:6", "--level=2"], ["2", "0"], 0),   # inside level 0's box, past level 2's (10 x 100 x 6)
                                    (seg, ["--roi=3:3,0:4,0:6"], ["2", "0"], 0),                 # empty
                                    (seg, ["--level=5"], ["2", "0"], 0),
                                    (seg, ["--planes=9"], ["2", "0"], 0),
                                    (seg, ["--level=1", "--field=1"], ["2", "0"], 1)):          # no such field
        out = tmp_path / "out.bin"
        r = run(WRDEC, options + ["data.wrb", "data.wrh", str(out)] + tail, d)
        assert r.returncode == 1, (options, r.returncode, r.stdout[-1000:], r.stderr[-1000:])
        assert "field %d" % field in r.stdout, (options, r.stdout[-1000:])
        assert not os.path.exists(out), options
    # the other fields of a file are written: three records for four fields, each the level-1 box of its field
    out = tmp_path / "three.bin"
    r = run(WRDEC, ["--level=1", "data.wrb", "data.wrh", str(out), "0", "0"], many)
    assert r.returncode == 1 and "field 2" in r.stdout
    raw, at, sizes = read(out), 0, []
    while at < len(raw):
        n = struct.unpack_from("<i", raw, at)[0]
        assert struct.unpack_from("<i", raw, at + 4 + n)[0] == n
        sizes.append(n)
        at += 8 + n
    want = []
    for fd in c["fields"]:
        nbytes, nx, ny, nz, nh, idinv = fd["spec"]
        if fd["icomp"]:
            want.append(nbytes * int(np.prod(api.lowres_shape((nz * nh, ny, nx), 1))))
    assert sizes == want


def test_constant_field_gives_midval(tmp_path_factory, tmp_path):
    d = encoded("stdin_trivial", "wrs1", tmp_path_factory)   # field 0 is the constant 2.5, 8^3
    out = tmp_path / "out.bin"
    r = run(WRDEC, ["--level=1", "--field=0", "data.wrb", "data.wrh", str(out), "2", "0"], d)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1000:]
    got = np.frombuffer(read(out), dtype=np.float64)
    assert got.size == 64 and np.all(got == 2.5)


# ---- 7. the other front-ends get the formats through the environment -------------------------------------------------------
def test_mssg_pair_under_the_environment_variable(monkeypatch, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_golden_mssg
    import mssg_cases
    case = "regout_f64_odd_inmeta"
    enc, dec = os.path.join(BINDIR, "wrenc_mssg"), os.path.join(BINDIR, "wrdec_mssg")
    monkeypatch.setenv("WR_QUIET", "1")
    files = {}
    for fmt in (None, "wrs1"):
        if fmt:
            monkeypatch.setenv("WR_STREAM_FORMAT", fmt)
        else:
            monkeypatch.delenv("WR_STREAM_FORMAT", raising=False)
        d = tmp_path / (fmt or "ref")
        d.mkdir()
        files[fmt] = make_golden_mssg.run_case(case, enc, dec, str(d))
    coded, decoded = mssg_cases.output_files(case)
    for name in decoded:
        assert files[None][name] == files["wrs1"][name], name
    payload = [n for n in coded if "_f" in n][0]
    assert api.stream_sniff(files[None][payload]) == api.FORMAT_REF
    assert api.stream_sniff(files["wrs1"][payload]) == api.FORMAT_WRS1


def test_reference_wrenc_on_this_library_under_the_environment_variable(golden_cli, tmp_path):
    enc = os.path.join(REFDIR, "wrenc_ref_dyn")
    if not os.path.exists(enc):
        pytest.skip("oracle/_ref/wrenc_ref_dyn not built")
    case = "config1_64cube"
    argv, stdin = cli_cases.write_inputs(case, str(tmp_path))
    r = run(enc, argv, tmp_path, stdin, WR_STREAM_FORMAT="wrs1")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    recs = parse_wrh(read(tmp_path / "data.wrh").decode())
    assert api.stream_sniff(read(tmp_path / "data.wrb")) == api.FORMAT_WRS1 and recs[0]["ntot_enc"] == os.path.getsize(tmp_path / "data.wrb")
    r = run(WRDEC, cli_cases.dec_argv(case), tmp_path)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert sha(read(tmp_path / "datarec.bin")) == golden_cli[case]["rec_sha256"]
