"""The stream format of the drop-in symbols (include/waverange_amd.h, "The stream format of the drop-in symbols") without a
GPU: the parser's grammar and refusals, set / get, the sniff on real streams of all four formats, and the `--` options of
wrenc / wrdec built against the CPU codec, which has none of the segmented entry points."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cli_cases
from util import GOLDEN, build_cli, codec_library
from waverange_amd import api, synth

SEG, BRICK, STRANDS = api.SEG_DEFAULT, api.BRICK_DEFAULT, api.STRANDS_DEFAULT

ACCEPTED = {
    "ref": (0, 0, 0, 0),
    "wrs1": (1, SEG, 0, 0),
    "wrs1:seg=4096": (1, 4096, 0, 0),
    "wrs1:seg=16": (1, 16, 0, 0),
    "wrs1:seg=59984": (1, 59984, 0, 0),
    "wrs2": (2, SEG, BRICK, 0),
    "wrs2:brick=8": (2, SEG, 8, 0),
    "wrs2:brick=64:seg=1008": (2, 1008, 64, 0),
    "wrs2:seg=1008:brick=16": (2, 1008, 16, 0),
    "wrs3": (3, SEG, 0, STRANDS),
    "wrs3:strands=8:seg=4096": (3, 4096, 0, 8),
    "wrs3:seg=4096:brick=16:strands=8": (3, 4096, 16, 8),
    "wrs3:strands=32:brick=32": (3, SEG, 32, 32),
    "wrs3:brick=0": (3, SEG, 0, STRANDS),
    "wrs3:strands=1:seg=16": (3, 16, 0, 1),
    "wrs3:seg=128": (3, 128, 0, STRANDS),       # 16 * 8 strands = 128: the smallest segment of the default strand count
}
# text -> the token the message has to name
REFUSED = {
    "": "''", "wrs4": "'wrs4'", "WRS1": "'WRS1'", "wrs1 ": "'wrs1 '", " wrs1": "' wrs1'", "seg=4096": "'seg=4096'",   # unknown names
    "wrs1:segs=4096": "'segs=4096'", "wrs2:bricks=8": "'bricks=8'", "wrs1:seg": "'seg'", "wrs3:4096": "'4096'",        # unknown keys
    "wrs1:seg=4096:seg=4096": "'seg=4096'", "wrs3:strands=2:seg=64:strands=4": "'strands=4'",                            # given twice
    "wrs2:brick=8:brick=16": "'brick=16'",
    "wrs1:brick=8": "'brick=8'", "ref:seg=4096": "'seg=4096'", "ref:brick=8": "'brick=8'", "ref:strands=8": "'strands=8'",
    "wrs1:strands=8": "'strands=8'", "wrs2:strands=2": "'strands=2'",                                                   # strands without wrs3
    "wrs1:seg=0": "'seg=0'", "wrs1:seg=8": "'seg=8'", "wrs1:seg=4100": "'seg=4100'", "wrs1:seg=60000": "'seg=60000'",   # seg_ok
    "wrs1:seg=99999999999": "'seg=99999999999'", "wrs1:seg=-16": "'seg=-16'", "wrs1:seg=": "'seg='", "wrs1:seg=4096x": "'seg=4096x'",
    "wrs2:brick=0": "'brick=0'", "wrs2:brick=12": "'brick=12'", "wrs3:brick=128": "'brick=128'",                        # brick_ok
    "wrs3:strands=0": "'strands=0'", "wrs3:strands=3": "'strands=3'", "wrs3:strands=64": "'strands=64'",                # strands_ok
    "wrs3:strands=8:seg=64": "'strands=8'", "wrs3:seg=112": "'strands=8'",                                              # 16 * strands > seg
    "wrs1:": "''", "wrs1:seg=4096:": "''", "wrs1::seg=4096": "''", "wrs1:seg=4096 ": "'seg=4096 '", "wrs1,seg=4096": "'wrs1,seg=4096'",  # trailing text
    "wrs1:seg=4096,brick=8": "'seg=4096,brick=8'",
}


@pytest.mark.parametrize("text", sorted(ACCEPTED))
def test_parser_accepts(text):
    assert api.stream_format_parse(text) == ACCEPTED[text]


@pytest.mark.parametrize("text", sorted(REFUSED))
def test_parser_refuses_and_names_the_token(text):
    f, seg = api.C.c_int(77), api.C.c_uint(77)
    assert api.lib().wr_stream_format_parse(text.encode(), api.C.byref(f), api.C.byref(seg), None, None) == -1
    assert (f.value, seg.value) == (77, 77), "outputs written on an error"
    msg = api.lib().wr_last_error().decode()
    assert REFUSED[text] in msg and repr(text)[1:-1] in msg, msg
    with pytest.raises(api.WaveRangeError) as e:
        api.stream_format_parse(text)
    assert "error -1" in str(e.value)


def test_parser_null_arguments():
    assert api.lib().wr_stream_format_parse(None, None, None, None, None) == -1
    assert api.lib().wr_stream_format_parse(b"wrs2", None, None, None, None) == 0


def test_set_and_get_round_trip_and_set_refuses_what_the_parser_refuses():
    L = api.lib()
    try:
        for text, want in ACCEPTED.items():
            api.set_stream_format(text)
            assert api.stream_format() == want, text
        # zeros are the defaults, as in the _seg calls
        for args, want in (((1, 0, 0, 0), (1, SEG, 0, 0)), ((2, 0, 0, 0), (2, SEG, BRICK, 0)), ((2, 1008, 0, 0), (2, 1008, BRICK, 0)),
                           ((3, 0, 0, 0), (3, SEG, 0, STRANDS)), ((3, 4096, 16, 0), (3, 4096, 16, STRANDS)), ((0, 0, 0, 0), (0, 0, 0, 0))):
            assert L.wr_set_stream_format(*args) == 0, args
            assert api.stream_format() == want, args
        api.set_stream_format("wrs2:brick=16")
        for args in ((-1, 0, 0, 0), (4, 0, 0, 0), (0, 4096, 0, 0), (0, 0, 8, 0), (0, 0, 0, 8), (1, 0, 8, 0), (1, 0, 0, 8), (2, 0, 0, 2),
                     (1, 8, 0, 0), (1, 4100, 0, 0), (1, 60000, 0, 0), (2, 0, 12, 0), (3, 0, 128, 0), (3, 0, 0, 3), (3, 0, 0, 64), (3, 64, 0, 8)):
            assert L.wr_set_stream_format(*args) == -1, args
            assert "wr_set_stream_format" in L.wr_last_error().decode()
            assert api.stream_format() == (2, SEG, 16, 0), "a refused set changed the setting"
        api.set_stream_format(None)
        assert api.stream_format() == (0, 0, 0, 0)
    finally:
        api.set_stream_format(None)


def test_sniff(oracle):
    f = synth.field(40, 36, 28, seed=77)
    enc = oracle.encode(f, 1e-6)
    assert enc["nlay"] == 4
    assert api.stream_sniff(enc["data"]) == api.FORMAT_REF
    at = 0
    for n in enc["len_enc_vec"]:  # every plane of a reference stream starts with byte 0: no ambiguity with a magic
        assert enc["data"][at] == 0 and api.stream_sniff(enc["data"][at:at + n]) == api.FORMAT_REF
        at += n
    plane = np.ascontiguousarray(enc["data"][:5000])  # any symbols will do
    shape = (5, 20, 50)
    assert api.stream_sniff(api.seg_encode_host_ref(plane, 1008)) == api.FORMAT_WRS1
    assert api.stream_sniff(api.seg_encode_host_ref_blocked(plane, shape, brick=8, seg=1008)) == api.FORMAT_WRS2
    assert api.stream_sniff(api.seg_encode_host_ref_strands(plane, shape, brick=8, seg=1008, strands=4)) == api.FORMAT_WRS3
    assert api.stream_sniff(api.seg_encode_host_ref_strands(plane, seg=1008)) == api.FORMAT_WRS3
    assert api.stream_sniff(b"WRS1") == 1 and api.stream_sniff(b"WRS3" + bytes(20)) == 3
    for junk in (b"WRS4....", b"WRS0....", b"WRSx", b"W", b"WR", b"WRS", b"wrs1....", b"", b"\x01\x00\x00\x00"):
        assert api.stream_sniff(junk) == -1, junk
    assert api.stream_sniff(b"\x00") == api.FORMAT_REF
    assert api.lib().wr_stream_sniff(None, 0) == -1 and api.lib().wr_stream_sniff(None, 8) == -1
    L = api.lib()
    buf = np.frombuffer(b"WRS2tail", dtype=np.uint8)
    assert [L.wr_stream_sniff(buf.ctypes.data, n) for n in range(9)] == [-1, -1, -1, -1, 2, 2, 2, 2, 2]


# ---- the tools on the CPU codec: options are taken out before the arguments are counted ------------------------------------
@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("cli_options"))
    so = codec_library()
    return build_cli("wrenc", so, d), build_cli("wrdec", so, d)


@pytest.fixture(scope="module")
def golden_case():
    with open(os.path.join(GOLDEN, "cli.json")) as fh:
        return json.load(fh)["config1_64cube"]


def run(exe, args, cwd):
    return subprocess.run([exe] + args, cwd=str(cwd), capture_output=True, text=True, env=dict(os.environ, WR_QUIET="1"))


def sha_file(p):
    return hashlib.sha256(open(p, "rb").read()).hexdigest()


@pytest.mark.parametrize("where", ["first", "last", "middle"])
def test_wrenc_format_ref_gives_the_golden_files(cli, golden_case, tmp_path, where):
    argv, _ = cli_cases.write_inputs("config1_64cube", str(tmp_path))
    at = dict(first=0, last=len(argv), middle=4)[where]
    r = run(cli[0], argv[:at] + ["--format=ref"] + argv[at:], tmp_path)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert "automatic mode." in r.stdout, "the option was counted as a positional argument"
    assert open(tmp_path / "data.wrh").read() == golden_case["wrh"]
    assert sha_file(tmp_path / "data.wrb") == golden_case["wrb_sha256"]
    r = run(cli[1], cli_cases.dec_argv("config1_64cube"), tmp_path)
    assert r.returncode == 0 and sha_file(tmp_path / "datarec.bin") == golden_case["rec_sha256"]


@pytest.mark.parametrize("option,say", [("--format=wrs1", "not supported by this codec library"),
                                        ("--format=wrs3:seg=4096:strands=8", "not supported by this codec library"),
                                        ("--bogus", "--bogus"), ("--format", "--format"), ("--formats=ref", "--formats=ref")])
def test_wrenc_refuses_before_it_writes(cli, tmp_path, option, say):
    argv, _ = cli_cases.write_inputs("config1_64cube", str(tmp_path))
    r = run(cli[0], [option] + argv, tmp_path)
    assert r.returncode == 2, (r.returncode, r.stdout[-2000:], r.stderr)
    assert say in r.stdout + r.stderr and "usage:" in r.stdout
    assert not os.path.exists(tmp_path / "data.wrb") and not os.path.exists(tmp_path / "data.wrh")


def test_wrenc_refusal_truncates_no_existing_file(cli, tmp_path):
    argv, _ = cli_cases.write_inputs("config1_64cube", str(tmp_path))
    for name in ("data.wrb", "data.wrh"):
        (tmp_path / name).write_bytes(b"keep me")
    assert run(cli[0], argv + ["--format=wrs2"], tmp_path).returncode == 2
    assert (tmp_path / "data.wrb").read_bytes() == b"keep me" and (tmp_path / "data.wrh").read_bytes() == b"keep me"


@pytest.mark.parametrize("options,status,say", [
    (["--roi=0:4,0:4,0:4"], 2, "not supported by this codec library"),
    (["--level=2"], 2, "not supported by this codec library"),
    (["--planes=1", "--field=0"], 2, "not supported by this codec library"),
    (["--bogus=1"], 2, "--bogus=1"),
    (["--roi=0:4,0:4"], 2, "--roi=0:4,0:4"),
    (["--roi=0:4,0:4,a:4"], 2, "--roi"),
    (["--level=x"], 2, "--level=x"),
    (["--field=0"], 2, "--field"),
    (["--level=0"], 0, "End of decompression"),     # level 0 alone is the full decode
])
def test_wrdec_options_on_the_golden_files(cli, golden_case, tmp_path, options, status, say):
    argv, _ = cli_cases.write_inputs("config1_64cube", str(tmp_path))
    assert run(cli[0], argv, tmp_path).returncode == 0
    r = run(cli[1], options + cli_cases.dec_argv("config1_64cube"), tmp_path)
    assert r.returncode == status, (r.returncode, r.stdout[-2000:], r.stderr)
    assert say in r.stdout + r.stderr
    if status:
        assert not os.path.exists(tmp_path / "datarec.bin")
    else:
        assert sha_file(tmp_path / "datarec.bin") == golden_case["rec_sha256"]


# ---- WR_STREAM_FORMAT: read once, in a child process each (none of this touches a GPU) -------------------------------------
CHILD = "import sys; sys.path.insert(0, %r)\nimport numpy as np\nfrom waverange_amd import api\n" % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(tmp_path, body, **env):
    script = tmp_path / "child.py"
    script.write_text(CHILD + body)
    e = dict(os.environ, **env)
    if "WR_STREAM_FORMAT" not in env:
        e.pop("WR_STREAM_FORMAT", None)
    return subprocess.run([sys.executable, str(script)], env=e, capture_output=True, text=True, timeout=120)


def test_environment_variable_sets_the_format_and_set_overrides_it(tmp_path):
    body = ("assert api.stream_format() == (3, 4096, 16, 8), api.stream_format()\n"
            "api.set_stream_format('wrs1')\nassert api.stream_format() == (1, api.SEG_DEFAULT, 0, 0)\n"
            "api.set_stream_format(None)\nassert api.stream_format() == (0, 0, 0, 0)\nprint('ok')\n")
    r = child(tmp_path, body, WR_STREAM_FORMAT="wrs3:seg=4096:brick=16:strands=8")
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    r = child(tmp_path, "assert api.stream_format() == (0, 0, 0, 0)\nprint('ok')\n")
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    # set before the variable was ever looked at: the variable is not looked at any more, good or bad
    r = child(tmp_path, "api.set_stream_format('wrs2')\nassert api.stream_format() == (2, api.SEG_DEFAULT, api.BRICK_DEFAULT, 0)\nprint('ok')\n",
              WR_STREAM_FORMAT="bogus")
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_a_bad_environment_value_is_fatal_at_the_first_encode(tmp_path):
    """No silent fall back to the reference's stream: the getter reports the parser's message, the encoder dies with it --
    before it asks for a device, so this runs anywhere."""
    body = ("try:\n    api.stream_format(); print('no error')\nexcept api.WaveRangeError as e:\n    print('getter:', e)\n"
            "sys.stdout.flush()\napi.encoding_wrap(np.zeros((4, 4, 4)), 1e-3)\nprint('survived')\n")
    r = child(tmp_path, body, WR_STREAM_FORMAT="wrs1:brick=8")
    assert r.returncode != 0 and "survived" not in r.stdout, r.stdout + r.stderr
    assert "getter:" in r.stdout and "WR_STREAM_FORMAT" in r.stdout and "'brick=8'" in r.stdout, r.stdout
    assert "encoding_wrap" in r.stderr and "WR_STREAM_FORMAT" in r.stderr and "'brick=8'" in r.stderr, r.stderr
