"""The three drivers of the reference stream format (encode, decode, transcode) on the same small fields, under every way the
host coder can be run: what the stages they share do through each.

The drivers place coded planes by their histogram bounds, pass the pool's admission gate, gather their planes one decode at a
time and hand the planes to the coder pool or to threads of their own.  This file drives three small fields and a constant one
through all of them and pins the streams and reconstructions (against the CPU oracle and the segmented encoders, bit for bit),
WR_STAT_EARLY_DECODES, the relations between the wr_timings fields that the drivers guarantee by construction, and code and
text of the refusals.  The expected texts are the library's as they were before the drivers were folded onto one set of
stages; they are literals here on purpose.  The one text that changed with the fold: of several planes that do not decode, every
driver names the first (wr_decode_* named the last one before)."""
import numpy as np
import pytest

from util import ROOT, bits_equal  # noqa: F401
from test_gpu_transcode import FORMATS, own, same_info
from waverange_amd import api, synth

pytestmark = pytest.mark.gpu

TOL = 1e-6
# n = 60000: exactly one coder block (the stream ends with an empty block); n = 69120: a block and a short one; nothing divides
SHAPES = [(30, 50, 40), (36, 40, 48), (21, 19, 37)]
CONFIGS = {
    "pool": lambda: api.set_coder_pool(3, 4),
    "threads8": lambda: (api.set_coder_pool(0), api.set_threads(8)),
    "threads2": lambda: (api.set_coder_pool(0), api.set_threads(2)),  # fewer threads than planes
}
HEADER_KEYS = ("tolabs", "midval", "halfspanval", "wlev", "nlay", "ntot_enc", "len_enc_vec")
SHORT = "libwaverange_amd error -4: plane %d: stream does not decode to nx*ny*nz symbols"
# the plane each driver names when planes 1 and 3 are both cut in half
NAMED_OF_TWO = {"decode": 1, "transcode": 1}


@pytest.fixture(scope="module")
def ctx():
    api.set_verbosity(0)
    with api.Context(0) as c:
        yield c


@pytest.fixture(params=list(CONFIGS))
def coder(request):
    try:
        CONFIGS[request.param]()
        yield request.param
    finally:
        api.set_coder_pool(0)
        api.set_threads(8)


_CASES = {}


def case(ctx, oracle, shape):
    """The field of that shape in fp64 and fp32, the oracle's stream and reconstruction of each, and the segmented streams of
    the fp64 field from their own encoders.  Computed once per shape, never written to."""
    if shape not in _CASES:
        nz, ny, nx = shape
        f = synth.field(nx, ny, nz, seed=7)
        f32 = f.astype(np.float32)
        want, want32 = oracle.encode(f, TOL), oracle.encode(f32.astype(np.float64), TOL)
        assert want["nlay"] >= 3 and want32["nlay"] >= 3
        streams = {name: own(FORMATS[name][1](ctx, f, tol=TOL)) for name in ("wrs1", "wrs2", "wrs3")}
        streams["ref"] = want
        _CASES[shape] = dict(f=f, f32=f32, want=want, want32=want32, rec=np.asarray(oracle.decode(want, shape)).reshape(shape),
                             rec32=np.asarray(oracle.decode(want32, shape)).reshape(shape).astype(np.float32), streams=streams)
    return _CASES[shape]


def same_stream(enc, want):
    return (np.array_equal(enc["data"], want["data"]) and all(np.array_equal(np.asarray(enc[k]), np.asarray(want[k])) for k in HEADER_KEYS)
            and bits_equal(enc["deps_vec"], want["deps_vec"]) and bits_equal(enc["minval_vec"], want["minval_vec"]))


def same_f32(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def host_half(tm, nlay):
    """plane_coder_s is positive in its first nlay entries and zero behind them, rangecoder is the largest of them"""
    s = tm["plane_coder_s"]
    return all(v > 0 for v in s[:nlay]) and all(v == 0 for v in s[nlay:]) and tm["rangecoder"] == max(s[:nlay]) and tm["transfer"] >= 0


def device_half(tm, begin):
    """a finish reports the coder seconds of its begin, and a total that is not below the begin's"""
    return tm["plane_coder_s"] == begin["plane_coder_s"] and tm["rangecoder"] == begin["rangecoder"] and tm["total"] >= begin["total"] and tm["transfer"] >= 0


class EarlyDecodes:
    def __enter__(self):
        self.at = api.stat(api.STAT_EARLY_DECODES)
        return self

    def __exit__(self, *exc):
        self.delta = api.stat(api.STAT_EARLY_DECODES) - self.at


def message(call):
    with pytest.raises(api.WaveRangeError) as e:
        call()
    return str(e.value)


def cut(enc, planes):
    """The stream with the listed planes cut in half; len_enc_vec, ntot_enc and the buffer agree on the shorter lengths."""
    parts, lens, off = [], [], 0
    for l, ln in enumerate(enc["len_enc_vec"]):
        keep = ln // 2 if l in planes else ln
        parts.append(np.asarray(enc["data"][off:off + keep]))
        lens.append(keep)
        off += ln
    return dict(enc, len_enc_vec=lens, ntot_enc=sum(lens), data=np.concatenate(parts))


# ---- streams and fields ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=["n60000", "n69120", "odd"])
def test_encode_and_decode(ctx, oracle, coder, shape):
    s = case(ctx, oracle, shape)
    f, f32, want, want32 = s["f"], s["f32"], s["want"], s["want32"]
    nlay, n = want["nlay"], f.size
    enc, _ = ctx.encode_host(f, TOL)
    assert same_stream(enc, want)
    enc32, _ = ctx.encode_host_f32(f32, TOL)
    assert same_stream(enc32, want32)
    buf = ctx.to_device(f)
    try:
        encd, _ = ctx.encode(buf, shape, TOL)
        assert same_stream(encd, want)
        with EarlyDecodes() as k:
            h64, h32 = np.empty(shape), np.empty(shape, dtype=np.float32)
            tm = ctx.decode_host(h64, want)
            tm32 = ctx.decode_host_f32(h32, want32)
            tmd = ctx.decode(buf, shape, want)
            d64 = buf.download(np.float64, n)
        assert k.delta == 3
        assert bits_equal(h64, s["rec"]) and same_f32(h32, s["rec32"]) and bits_equal(d64, s["rec"])
        assert all(host_half(t, nlay) for t in (tm, tm32, tmd)), (tm, tm32, tmd)
        assert tmd["d2h_ms"] == 0
        # the two halves on their own
        for finish in ("host", "host_f32", "device"):
            src = want32 if finish == "host_f32" else want
            with EarlyDecodes() as k:
                tb = ctx.decode_begin(shape, src)
            assert k.delta == 1 and host_half(tb, src["nlay"]), (finish, tb)
            with EarlyDecodes() as k:
                if finish == "host":
                    out = np.empty(shape)
                    tf = ctx.decode_finish_host(out)
                    assert bits_equal(out, s["rec"])
                elif finish == "host_f32":
                    out = np.empty(shape, dtype=np.float32)
                    tf = ctx.decode_finish_host_f32(out)
                    assert same_f32(out, s["rec32"])
                else:
                    tf = ctx.decode_finish(buf)
                    assert bits_equal(buf.download(np.float64, n), s["rec"]) and tf["d2h_ms"] == 0
            assert k.delta == 0 and device_half(tf, tb), (finish, tb, tf)
    finally:
        buf.free()


@pytest.mark.parametrize("shape", SHAPES, ids=["n60000", "n69120", "odd"])
def test_transcode(ctx, oracle, coder, shape):
    s = case(ctx, oracle, shape)
    streams, nlay = s["streams"], s["want"]["nlay"]
    with EarlyDecodes() as k:
        for src, dst in (("ref", "ref"), ("ref", "wrs1"), ("wrs2", "ref"), ("wrs3", "ref")):
            tm = {}
            data, info = ctx.transcode(streams[src], streams[src]["data"], FORMATS[dst][0], shape=shape, timings=tm)
            assert data.tobytes() == streams[dst]["data"].tobytes() and same_info(info, streams[dst]), (src, dst)
            assert all(v > 0 for v in tm["plane_coder_s"][:nlay]) and all(v == 0 for v in tm["plane_coder_s"][nlay:]) and tm["rangecoder"] > 0, (src, dst, tm)
            assert tm["transfer"] >= 0
    assert k.delta == 0


@pytest.mark.parametrize("shape", SHAPES, ids=["n60000", "n69120", "odd"])
def test_small_cap(ctx, oracle, coder, shape):
    """cap one byte above the stream: the sum of the histogram bounds (and the block of slack behind the last plane) does not
    fit under it, so at least the last plane is coded into the context's buffer and copied into place"""
    s = case(ctx, oracle, shape)
    want = s["want"]
    cap = want["ntot_enc"] + 1
    enc, _ = ctx.encode_host(s["f"], TOL, out=np.empty(cap, dtype=np.uint8))
    assert same_stream(enc, want)
    for src in ("ref", "wrs1"):
        data, info = ctx.transcode(s["streams"][src], s["streams"][src]["data"], "ref", shape=shape, cap=cap)
        assert data.tobytes() == want["data"].tobytes() and same_info(info, want), src


def test_constant_field(ctx, oracle, coder):
    shape = (21, 19, 37)
    f = np.full(shape, 3.25)
    want = oracle.encode(f, TOL)
    assert want["nlay"] == 0 and want["ntot_enc"] == 0
    enc, _ = ctx.encode_host(f, TOL)
    enc32, _ = ctx.encode_host_f32(f.astype(np.float32), TOL)
    assert same_stream(enc, want) and same_stream(enc32, want)
    buf = ctx.to_device(f)
    try:
        encd, _ = ctx.encode(buf, shape, TOL)
        assert same_stream(encd, want)
        with EarlyDecodes() as k:  # the header is the field: no plane is decoded
            h64, h32 = np.zeros(shape), np.zeros(shape, dtype=np.float32)
            ctx.decode_host(h64, want)
            ctx.decode_host_f32(h32, want)
            ctx.decode(buf, shape, want)
            assert np.all(h64 == 3.25) and np.all(h32 == np.float32(3.25)) and np.all(buf.download(np.float64, f.size) == 3.25)
            ctx.decode_begin(shape, want)
            out = np.zeros(shape)
            ctx.decode_finish_host(out)
            assert np.all(out == 3.25)
            data, info = ctx.transcode(want, want["data"], "ref", shape=shape)
            assert data.size == 0 and same_info(info, want)
        assert k.delta == 0
    finally:
        buf.free()


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_finish_without_begin(ctx, oracle):
    s = case(ctx, oracle, SHAPES[2])
    out = np.empty(SHAPES[2])
    text = "libwaverange_amd error -1: wr_decode_finish without a wr_decode_begin on this context"
    ctx.decode_host(out, s["want"])  # (whatever an earlier test left pending is gone)
    assert message(lambda: ctx.decode_finish_host(out)) == text
    assert message(lambda: ctx.decode_finish_host_f32(np.empty(SHAPES[2], dtype=np.float32))) == text
    buf = ctx.alloc(out.nbytes)
    try:
        assert message(lambda: ctx.decode_finish(buf)) == text
    finally:
        buf.free()
    ctx.decode_begin(SHAPES[2], s["want"])
    ctx.decode_finish_host(out)
    assert message(lambda: ctx.decode_finish_host(out)) == text  # a finish consumes its begin
    assert bits_equal(out, s["rec"])


@pytest.mark.parametrize("shape", SHAPES[1:], ids=["n69120", "odd"])
def test_planes_cut_in_half(ctx, oracle, coder, shape):
    """A plane cut in half comes back short (checked on the host coder first: at these inputs the halves of planes 1 and 3 do,
    while some other halves happen to decode to n symbols of something)"""
    s = case(ctx, oracle, shape)
    want, n = s["want"], s["f"].size
    assert want["nlay"] == 4
    off = np.concatenate(([0], np.cumsum(want["len_enc_vec"])))
    for l in (1, 3):
        assert api.range_decode(want["data"][off[l]:off[l] + want["len_enc_vec"][l] // 2].copy(), n)[1] != n
    out = np.empty(shape)
    last, two = cut(want, {3}), cut(want, {1, 3})
    with EarlyDecodes() as k:
        assert message(lambda: ctx.decode_host(out, last)) == SHORT % 3
        assert message(lambda: ctx.decode_host(out, two)) == SHORT % NAMED_OF_TWO["decode"]
        assert message(lambda: ctx.decode_begin(shape, two)) == SHORT % NAMED_OF_TWO["decode"]
    assert k.delta == 3
    assert message(lambda: ctx.decode_finish_host(out)).endswith("wr_decode_finish without a wr_decode_begin on this context")
    assert message(lambda: ctx.transcode(last, last["data"], FORMATS["wrs1"][0], shape=shape)) == SHORT % 3
    assert message(lambda: ctx.transcode(two, two["data"], FORMATS["wrs1"][0], shape=shape)) == SHORT % NAMED_OF_TWO["transcode"]
    # the context decodes and transcodes afterwards
    ctx.decode_host(out, want)
    assert bits_equal(out, s["rec"])
    data, _ = ctx.transcode(want, want["data"], FORMATS["wrs1"][0], shape=shape)
    assert data.tobytes() == s["streams"]["wrs1"]["data"].tobytes()
