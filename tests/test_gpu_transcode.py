"""Transcoding between the four stream formats on the GPU (Context.transcode / wr_transcode_host, include/waverange_amd.h) and
the wrconv tool.  The expected bytes of every transcode are the target format's own encoder's for the original field, and the
host definition's (api.transcode_host_ref); decoding a transcoded stream gives the source's reconstruction bit for bit.  Every
comparison is equality: no tolerance appears anywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cli_cases
from util import ROOT, bits_equal
from waverange_amd import api, synth

pytestmark = pytest.mark.gpu

TOL = 1e-7
# name -> (format text of the target, how the product encodes a field that way)
FORMATS = {
    "ref": ("ref", lambda ctx, f, **kw: ctx.encode_host(f, kw.pop("tol", TOL), **kw)),
    "wrs1": ("wrs1:seg=4096", lambda ctx, f, **kw: ctx.encode_host_seg(f, kw.pop("tol", TOL), seg=4096, **kw)),
    "wrs2": ("wrs2:seg=4096:brick=8", lambda ctx, f, **kw: ctx.encode_host_seg(f, kw.pop("tol", TOL), seg=4096, brick=8, **kw)),
    "wrs3": ("wrs3:seg=4096:strands=8", lambda ctx, f, **kw: ctx.encode_host_seg(f, kw.pop("tol", TOL), seg=4096, strands=8, **kw)),
    "wrs3b": ("wrs3:seg=4096:strands=8:brick=8", lambda ctx, f, **kw: ctx.encode_host_seg(f, kw.pop("tol", TOL), seg=4096, brick=8, strands=8, **kw)),
}
HEADER_KEYS = ("tolabs", "midval", "halfspanval", "wlev", "nlay", "ntot_enc", "len_enc_vec")


@pytest.fixture(scope="module")
def ctx():
    api.set_verbosity(0)
    with api.Context(0) as c:
        yield c


def own(r):
    enc, _ = r
    enc["data"] = enc["data"].copy()
    return enc


_STREAMS = {}


def streams_of(ctx, shape, **kw):
    """The five streams of the synthetic field of that shape, each from the product's own encoder; computed once per shape,
    never written to."""
    key = (shape, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _STREAMS:
        nz, ny, nx = shape
        f = synth.field(nx, ny, nz, seed=7)
        _STREAMS[key] = (f, {name: own(encode(ctx, f, **dict(kw))) for name, (_, encode) in FORMATS.items()})
    return _STREAMS[key]


def same_info(a, b):
    return (all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in HEADER_KEYS)
            and bits_equal(np.asarray(a["deps_vec"]), np.asarray(b["deps_vec"])) and bits_equal(np.asarray(a["minval_vec"]), np.asarray(b["minval_vec"])))


def decode(ctx, shape, enc):
    out = np.empty(shape, np.float64)
    (ctx.decode_host if api.stream_sniff(enc["data"]) <= 0 else ctx.decode_host_seg)(out, enc)
    return out


def check_pair(ctx, shape, src, dst, streams, recon=None):
    s, want = streams[src], streams[dst]
    data, info = ctx.transcode(s, s["data"], FORMATS[dst][0], shape=shape)
    assert data.tobytes() == want["data"].tobytes(), (shape, src, dst, data.size, want["data"].size)
    assert same_info(info, want), (shape, src, dst)
    rdata, rinfo = api.transcode_host_ref(shape, s, s["data"], FORMATS[dst][0])
    assert rdata.tobytes() == data.tobytes() and same_info(rinfo, info), (shape, src, dst)
    if recon is not None:
        assert bits_equal(decode(ctx, shape, info), recon[src]), (shape, src, dst)


def test_all_pairs(ctx):
    shape = (28, 36, 40)
    f, streams = streams_of(ctx, shape)
    assert streams["ref"]["nlay"] == 4
    recon = {name: decode(ctx, shape, s) for name, s in streams.items()}
    for name in recon:
        assert bits_equal(recon[name], recon["ref"])
    for src in FORMATS:
        for dst in FORMATS:
            check_pair(ctx, shape, src, dst, streams, recon)
    # a recut, and the target's defaults
    data, info = ctx.transcode(streams["wrs1"], streams["wrs1"]["data"], "wrs1:seg=2048", shape=shape)
    want = own(ctx.encode_host_seg(f, TOL, seg=2048))
    assert data.tobytes() == want["data"].tobytes() and same_info(info, want)
    data, info = ctx.transcode(streams["ref"], streams["ref"]["data"], "wrs3", shape=shape)
    want = own(ctx.encode_host_seg(f, TOL, strands=0))
    assert data.tobytes() == want["data"].tobytes() and same_info(info, want)


@pytest.mark.parametrize("shape", [(30, 50, 40), (36, 40, 48)], ids=["n60000", "n69120"])
def test_ref_edges_on_block_boundaries(ctx, shape):
    """n = 60000: the reference stream ends with an empty block, the block histograms have an empty last record; n = 69120: two
    reference blocks."""
    f, streams = streams_of(ctx, shape)
    for other in FORMATS:
        check_pair(ctx, shape, "ref", other, streams)
        check_pair(ctx, shape, other, "ref", streams)
    data, info = ctx.transcode(streams["ref"], streams["ref"]["data"], "wrs1", shape=shape)  # the default seg: a last segment of 96 symbols at n = 60000
    want = own(ctx.encode_host_seg(f, TOL))
    assert data.tobytes() == want["data"].tobytes() and same_info(info, want)


def test_no_transform_trivial_local_cutoff(ctx):
    # wtflag = 0: the blocked order is one box, the field (order_of with wlev 0)
    shape = (28, 36, 40)
    f, streams = streams_of(ctx, shape, wtflag=0)
    assert streams["ref"]["wlev"] == 0
    for src, dst in (("ref", "wrs2"), ("wrs1", "wrs2"), ("wrs2", "ref"), ("wrs2", "wrs3b"), ("wrs3b", "wrs1")):
        check_pair(ctx, shape, src, dst, streams)
    # a trivial field passes through
    const = np.full(shape, 2.5)
    enc = own(ctx.encode_host(const, TOL))
    assert enc["ntot_enc"] == 0 and enc["nlay"] == 0
    for fmt in ("ref", "wrs1", "wrs2", "wrs3"):
        data, info = ctx.transcode(enc, enc["data"], fmt, shape=shape)
        assert data.size == 0 and same_info(info, enc) and info["midval"] == 2.5
        assert bits_equal(decode(ctx, shape, info), const)
    # a local-cutoff stream (the case of tests/test_gpu_seg.py::test_codec_level_local_cutoff)
    cutoff = np.array([1e-3, 1e-5, 1e-4, 1e-6, 1e-5, 1e-3, 1e-4, 1e-5], dtype=np.float64)
    shape = (40, 48, 64)
    f, streams = streams_of(ctx, shape, tol=None, cutoff=cutoff, m=(2, 2, 2))
    for src, dst in (("ref", "wrs3"), ("wrs3", "ref"), ("wrs1", "wrs2"), ("wrs2", "wrs1")):
        check_pair(ctx, shape, src, dst, streams)


def test_host_coder_configurations(ctx):
    """A reference side runs on the coder pool, on one thread per plane and on wr_set_threads(2) groups: the same bytes."""
    shape = (36, 40, 48)
    f, streams = streams_of(ctx, shape)
    try:
        for configure in (lambda: api.set_coder_pool(3, 4), lambda: (api.set_coder_pool(0), api.set_threads(8)), lambda: api.set_threads(2)):
            configure()
            for src, dst in (("ref", "wrs1"), ("wrs3", "ref"), ("ref", "ref"), ("ref", "wrs3b"), ("wrs2", "ref")):
                check_pair(ctx, shape, src, dst, streams)
    finally:
        api.set_coder_pool(0)
        api.set_threads(8)


CHUNKED = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
from waverange_amd import api, synth
import test_gpu_transcode as t
api.set_verbosity(0)
with api.Context(0) as ctx:
    shape = (128, 128, 128)
    f, streams = t.streams_of(ctx, shape, tol=1e-6)
    recon = {name: t.decode(ctx, shape, streams[name]) for name in ("ref", "wrs3", "wrs2")}
    for src, dst in (("ref", "wrs1"), ("wrs3", "ref"), ("wrs2", "wrs3")):
        t.check_pair(ctx, shape, src, dst, streams, recon)
    api.set_coder_pool(2, 4)
    for src, dst in (("ref", "wrs1"), ("wrs3", "ref")):
        t.check_pair(ctx, shape, src, dst, streams)
    api.set_coder_pool(0)
print("ok")
"""


def test_planes_in_chunks_and_windows(tmp_path):
    """WR_PLANE_CHUNK_MB=1 WR_WINDOW_BLOCKS=2: a 128^3 plane lives in two chunks of 1 MiB and passes the host coder in windows of
    120000 symbols, one of which straddles the chunks: a plane that the decoder of this call filled -- through upload windows,
    or by the segment decoder -- is drained chunk by chunk by the host encoder of the same call."""
    script = tmp_path / "child.py"
    script.write_text(CHUNKED % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, str(script)], env=dict(os.environ, WR_PLANE_CHUNK_MB="1", WR_WINDOW_BLOCKS="2"), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-3000:]


def rc_of(call):
    with pytest.raises(api.WaveRangeError) as e:
        call()
    msg = str(e.value)
    return int(msg.split("error ")[1].split(":")[0]), msg


def test_refusals_on_a_live_context(ctx):
    shape = (28, 36, 40)
    f, streams = streams_of(ctx, shape)
    good = lambda: check_pair(ctx, shape, "wrs3", "ref", streams) or check_pair(ctx, shape, "ref", "wrs2", streams)
    errors0 = api.stat(7)  # WR_STAT_HANDOVER_ERRORS
    # a flipped byte inside the first segment of plane 1 (in its model: the counts no longer add up), behind a valid index: the
    # kernels flag the segment, -4 naming the plane
    for name, head in (("wrs1", 12), ("wrs3", 20)):
        s = streams[name]
        bad = s["data"].copy()
        at1 = s["len_enc_vec"][0]
        nseg = int(bad[at1 + 8:at1 + 12].view("<u4")[0])
        bad[at1 + head + 4 * nseg + 3] ^= 0x55
        assert rc_of(lambda: api.transcode_host_ref(shape, s, bad, "ref"))[0] == -4
        rc, msg = rc_of(lambda: ctx.transcode(s, bad, "ref", shape=shape))
        assert rc == -4 and "plane 1:" in msg, msg
        good()
    # inconsistent lengths: refused on the host, before anything is launched
    s = streams["wrs2"]
    rc, msg = rc_of(lambda: ctx.transcode(dict(s, len_enc_vec=[s["len_enc_vec"][0] - 4] + s["len_enc_vec"][1:]), s["data"], "wrs1", shape=shape))
    assert rc == -4 and "plane 0:" in msg, msg
    good()
    assert rc_of(lambda: ctx.transcode(dict(s, ntot_enc=s["ntot_enc"] - 1), s["data"], "wrs1", shape=shape))[0] == -4
    # bad arguments
    assert rc_of(lambda: ctx.transcode(s, s["data"], (api.FORMAT_WRS1, 17, 0, 0), shape=shape))[0] == -1
    assert rc_of(lambda: ctx.transcode(dict(s, wlev=2), s["data"], "ref", shape=shape))[0] == -1
    good()
    # cap: the bytes produced succeed, one byte short is -5, for a segmented and for a reference target
    for src, dst in (("ref", "wrs3"), ("wrs1", "ref"), ("ref", "ref")):
        exact = streams[dst]["ntot_enc"]
        data, _ = ctx.transcode(streams[src], streams[src]["data"], FORMATS[dst][0], shape=shape, cap=exact)
        assert data.tobytes() == streams[dst]["data"].tobytes()
        rc, msg = rc_of(lambda: ctx.transcode(streams[src], streams[src]["data"], FORMATS[dst][0], shape=shape, cap=exact - 1))
        assert rc == -5 and "encoded array is too large" in msg, msg
        good()
    # a pending wr_decode_begin is discarded, and the context decodes afterwards
    ctx.decode_begin(shape, streams["ref"])
    good()
    out = np.empty(shape)
    with pytest.raises(api.WaveRangeError):
        ctx.decode_finish_host(out)
    ctx.decode_begin(shape, streams["ref"])
    ctx.decode_finish_host(out)
    assert bits_equal(out, decode(ctx, shape, streams["wrs1"]))
    assert api.stat(7) == errors0


# ---- wrconv ------------------------------------------------------------------------------------------------------------------
BINDIR = os.path.join(ROOT, "waverange_amd", "bin")
WRENC, WRDEC, WRCONV = (os.path.join(BINDIR, n) for n in ("wrenc", "wrdec", "wrconv"))
CASE = "argv_two_fp32"


def run(exe, args, cwd, **env):
    e = dict(os.environ, WR_QUIET="1")
    e.pop("WR_STREAM_FORMAT", None)
    e.update(env)
    return subprocess.run([exe] + list(args), cwd=str(cwd), capture_output=True, text=True, env=e, timeout=300)


def read(path):
    with open(path, "rb") as fh:
        return fh.read()


_ENCODED = {}


def encoded(case, fmt, tmp_path_factory):
    if (case, fmt) not in _ENCODED:
        d = tmp_path_factory.mktemp("enc")
        argv, stdin = cli_cases.write_inputs(case, str(d))
        e = dict(os.environ, WR_QUIET="1")
        e.pop("WR_STREAM_FORMAT", None)
        r = subprocess.run([WRENC, "--format=" + fmt] + argv, cwd=str(d), input=stdin, capture_output=True, text=True, env=e, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        if os.path.exists(d / "inmeta"):
            os.remove(d / "inmeta")
        _ENCODED[(case, fmt)] = d
    return _ENCODED[(case, fmt)]


def records(path, nf):
    """every record of a .wrh as read_field_header reads it: whitespace-separated tokens behind the preamble, with the numbers
    as numbers"""
    text = read(path).decode()
    body = text.split("\n", 6)[6]
    out = []
    for rec in body.split(" -----\n")[1:]:
        lines = rec.split("\n")
        out.append([lines[0]] + [[float(t) if i != 1 else t for t in ln.split()] for i, ln in enumerate(lines[2:])])
    assert len(out) == nf
    return out


def decoded(d, case, tmp_path_factory):
    r = run(WRDEC, cli_cases.dec_argv(case), d)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return read(d / "datarec.bin")


def check_conversion(src_dir, fmt, case, tmp_path_factory, wrh_name="data.wrh"):
    """wrconv of the container in src_dir to fmt against wrenc --format=fmt of the original input."""
    want = encoded(case, fmt, tmp_path_factory)
    out = tmp_path_factory.mktemp("conv")
    # (the header names data.wrb, which is not in the working directory: it is found beside the header)
    r = run(WRCONV, ["--format=" + fmt, os.path.join(str(src_dir), wrh_name), "data.wrh", "data.wrb"], out)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert read(out / "data.wrb") == read(want / "data.wrb")
    nf = len(cli_cases.CASES[case]["fields"])
    assert records(out / "data.wrh", nf) == records(want / "data.wrh", nf)
    assert read(out / "data.wrh") == read(want / "data.wrh")  # (the header's 19 digits round-trip a double)
    return out


@pytest.mark.parametrize("case", [CASE, "inmeta_new_type0", "stdin_trivial"])
def test_wrconv_both_directions(case, tmp_path_factory):
    ref, wrs3 = encoded(case, "ref", tmp_path_factory), encoded(case, "wrs3", tmp_path_factory)
    a = check_conversion(ref, "wrs3", case, tmp_path_factory)
    b = check_conversion(wrs3, "ref", case, tmp_path_factory)
    rec = decoded(ref, case, tmp_path_factory)
    assert decoded(a, case, tmp_path_factory) == rec and decoded(b, case, tmp_path_factory) == rec and decoded(wrs3, case, tmp_path_factory) == rec
    # and there and back again, with other parameters on the way
    c = check_conversion(a, "wrs2:brick=8:seg=4096", case, tmp_path_factory)
    check_conversion(c, "ref", case, tmp_path_factory)


def test_wrconv_mixed_file_and_errors(tmp_path_factory):
    ref, wrs3 = encoded(CASE, "ref", tmp_path_factory), encoded(CASE, "wrs3", tmp_path_factory)
    # field 0 as the reference's stream, field 1 as WRS3, in one container
    mixed = tmp_path_factory.mktemp("mixed")
    ha, hb = read(ref / "data.wrh").decode(), read(wrs3 / "data.wrh").decode()
    cut = lambda t: t.index(" -----\n1\n")
    (mixed / "data.wrh").write_text(ha[:cut(ha)] + hb[cut(hb):])
    len0 = lambda d, t: int(records(d / "data.wrh", 2)[0][15][0])
    wa, wb = read(ref / "data.wrb"), read(wrs3 / "data.wrb")
    (mixed / "data.wrb").write_bytes(wa[:len0(ref, ha)] + wb[len0(wrs3, hb):])
    assert decoded(mixed, CASE, tmp_path_factory) == decoded(ref, CASE, tmp_path_factory)
    for fmt in ("wrs1", "ref", "wrs3"):
        check_conversion(mixed, fmt, CASE, tmp_path_factory)
    # options are judged before any output file is created
    out = tmp_path_factory.mktemp("bad")
    for args in (["--format=wrs9", str(ref / "data.wrh"), "o.wrh", "o.wrb"], ["--format=wrs1:seg=17", str(ref / "data.wrh"), "o.wrh", "o.wrb"],
                 [str(ref / "data.wrh"), "o.wrh", "o.wrb"], ["--format=ref", "--what=1", str(ref / "data.wrh"), "o.wrh", "o.wrb"]):
        r = run(WRCONV, args, out)
        assert r.returncode == 2 and not os.listdir(out), (args, r.stdout[-500:])
    # a damaged field: "field K: ...", exit status 1
    bad = tmp_path_factory.mktemp("damaged")
    (bad / "data.wrh").write_bytes(read(wrs3 / "data.wrh"))
    blob = bytearray(wb)
    blob[len0(wrs3, hb) + 3] ^= 0x10  # the magic of field 1's first plane
    (bad / "data.wrb").write_bytes(bytes(blob))
    r = run(WRCONV, ["--format=ref", str(bad / "data.wrh"), "o.wrh", "o.wrb"], out)
    assert r.returncode == 1 and "Error: field 1: " in r.stdout, r.stdout[-1000:]
