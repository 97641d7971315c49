"""Low-resolution decode of segmented streams on the GPU (include/waverange_amd.h, "Low-resolution decode").

The expected result D(r, p) is built here on the CPU exactly as the header defines it, from the oracle's dequantiser and
transform (oracle.loader.Oracle) and from planes recovered with api.seg_split / api.range_decode; every comparison of values
is equality of bit patterns.  The one exception is the accuracy condition at the end, whose bound is the codec's own:
tolrel * max|f|."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from util import ROOT
from test_lowres_cpu import SQRT_HALF, box_and_exponent, brute_force_segments
from oracle.loader import Oracle
from waverange_amd import api, synth

pytestmark = pytest.mark.gpu

SHAPES = [(77, 129, 200), (64, 64, 64), (1, 50, 70)]  # (nz, ny, nx)
TOLS = [1e-3, 1e-6]
LEVELS = range(5)


@pytest.fixture(scope="module")
def ctx():
    api.set_verbosity(0)
    with api.Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


def field(shape, seed=41):
    return synth.field(shape[2], shape[1], shape[0], seed=seed)


def scale(shape, level):
    _, e = box_and_exponent(shape[::-1], level)
    return math.ldexp(SQRT_HALF if e % 2 else 1.0, -(e // 2))


def expected(oracle, planes, info, shape, level, p):
    """D(level, p) of the definition: dequantise-accumulate p planes, cut the box, invert the remaining levels, scale."""
    acc = np.zeros(int(np.prod(shape)))
    for l in range(p):
        acc = oracle.dequant_accum(acc, planes[l], float(info["deps_vec"][l]), float(info["minval_vec"][l]))
    (bx, by, bz), _ = box_and_exponent(shape[::-1], level)
    box = np.ascontiguousarray(acc.reshape(shape)[:bz, :by, :bx])
    if info["wlev"] - level > 0:
        box = oracle.cdf97_3d(box, -(info["wlev"] - level))
    return box * scale(shape, level)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = np.uint64 if a.dtype == np.float64 else np.uint32
    return np.array_equal(a.view(u), b.view(u))


def split_planes(enc):
    out, at = [], 0
    for ln in enc["len_enc_vec"]:
        out.append(enc["data"][at:at + ln])
        at += ln
    return out


def planes_of(enc, n):
    """The symbols of every plane of a segmented stream: api.seg_split, then api.range_decode segment by segment."""
    out = []
    for blob in split_planes(enc):
        seg, streams = api.seg_split(blob)
        parts = []
        for k, s in enumerate(streams):
            bs = min(seg, n - k * seg)
            sym, got = api.range_decode(np.frombuffer(s, dtype=np.uint8), bs)
            assert got == bs
            parts.append(sym)
        out.append(np.concatenate(parts))
    return out


def encode_seg(ctx, f, tol, seg, wtflag=1):
    enc, _ = ctx.encode_host_seg(f, tol, wtflag, seg)
    enc["data"] = enc["data"].copy()
    return enc


def recut(enc, planes, segs):
    """The same field with plane l cut at segs[l % len(segs)], built from the host reference's blobs."""
    blobs = [api.seg_encode_host_ref(p, segs[l % len(segs)]) for l, p in enumerate(planes)]
    out = dict(enc, data=np.concatenate(blobs), len_enc_vec=[int(b.size) for b in blobs])
    out["ntot_enc"] = int(out["data"].size)
    return out


def decode_all_ways(ctx, shape, level, enc, p):
    """(float64 from the host call, float32 from the fp32 call, float64 from the device-output call)"""
    bshape = api.lowres_shape(shape, level)
    h64, h32 = np.empty(bshape), np.empty(bshape, dtype=np.float32)
    ctx.decode_host_seg_lowres(h64, shape, level, enc, p)
    ctx.decode_host_seg_lowres_f32(h32, shape, level, enc, p)
    buf = ctx.alloc(max(h64.nbytes, 16))
    try:
        ctx.decode_seg_lowres(buf, shape, level, enc, p)
        d64 = buf.download(np.float64, h64.size).reshape(bshape)
    finally:
        buf.free()
    return h64, h32, d64


# ---- stage level ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tol", TOLS)
@pytest.mark.parametrize("shape", SHAPES)
def test_stage_level(ctx, oracle, shape, tol):
    f = field(shape)
    n = f.size
    pitch = api.lib().wr_plane_pitch(n)
    buf, d_planes, d_out = ctx.to_device(f), ctx.alloc(pitch * api.NLAYMAX), ctx.alloc(max(f.nbytes, 16))
    try:
        info = ctx.encode_planes(buf, shape, tol, d_planes)
        planes = [d_planes.download(np.uint8, n, offset=l * pitch).copy() for l in range(info.nlay)]
        meta = info.as_dict()
        assert info.wlev == 4 and info.nlay >= 1
        for level in LEVELS:
            bshape = api.lowres_shape(shape, level)
            for p in sorted({1, info.nlay}):
                want = expected(oracle, planes, meta, shape, level, p)
                ctx.decode_planes_lowres(d_out, shape, level, d_planes, info, p)
                got = d_out.download(np.float64, want.size).reshape(bshape)
                assert same_bits(got, want), (shape, tol, level, p)
                if p == info.nlay:  # max_planes = 0 means all of them
                    ctx.decode_planes_lowres(d_out, shape, level, d_planes, info)
                    assert same_bits(d_out.download(np.float64, want.size).reshape(bshape), want), (shape, tol, level, "all")
        # level 0 with every plane is what decode_planes gives
        ctx.decode_planes_lowres(d_out, shape, 0, d_planes, info, info.nlay)
        full = d_out.download(np.float64, n).reshape(shape)
        ctx.decode_planes(buf, shape, d_planes, info)
        assert same_bits(full, buf.download(np.float64, n).reshape(shape)), (shape, tol)
        for level, p in ((5, 0), (-1, 0), (1, info.nlay + 1), (1, -1)):
            with pytest.raises(api.WaveRangeError) as e:
                ctx.decode_planes_lowres(d_out, shape, level, d_planes, info, p)
            assert "error -1" in str(e.value), str(e.value)
    finally:
        buf.free()
        d_planes.free()
        d_out.free()


# ---- codec level ------------------------------------------------------------------------------------------------------
def check_stream(ctx, oracle, shape, enc, planes, what):
    for level in LEVELS:
        for p in sorted({1, enc["nlay"]}):
            want = expected(oracle, planes, enc, shape, level, p)
            h64, h32, d64 = decode_all_ways(ctx, shape, level, enc, p)
            assert same_bits(h64, want), (what, level, p, "host")
            assert same_bits(d64, want), (what, level, p, "device")
            assert same_bits(h32, want.astype(np.float32)), (what, level, p, "fp32")


@pytest.mark.parametrize("shape,tol", [(SHAPES[0], 1e-6), (SHAPES[1], 1e-3), (SHAPES[2], 1e-6)])
def test_codec_level(ctx, oracle, shape, tol):
    f = field(shape)
    planes = None
    for seg in (4096, 59904):
        enc = encode_seg(ctx, f, tol, seg)
        got = planes_of(enc, f.size)
        if planes is not None:
            assert all(np.array_equal(a, b) for a, b in zip(planes, got))
        planes = got
        check_stream(ctx, oracle, shape, enc, planes, (shape, tol, seg))
        if seg == 59904:  # level 0 with every plane is the full decode
            full, low = np.empty_like(f), np.empty_like(f)
            ctx.decode_host_seg(full, enc)
            ctx.decode_host_seg_lowres(low, shape, 0, enc)
            assert same_bits(low, full)
    # planes cut at different segment lengths
    mixed = recut(enc, planes, (59904, 4096, 1024, 16))
    check_stream(ctx, oracle, shape, mixed, planes, (shape, tol, "mixed"))


def test_full_decode_is_level_zero(ctx, oracle):
    """D(0, nlay) on the GPU equals the oracle's decode of the reference-format stream of the same field."""
    for shape in SHAPES:
        f = field(shape)
        enc = encode_seg(ctx, f, 1e-6, 4096)
        low = np.empty_like(f)
        ctx.decode_host_seg_lowres(low, shape, 0, enc)
        assert same_bits(low, oracle.decode(oracle.encode(f, 1e-6), shape)), shape


def test_without_transform_and_constant_field(ctx, oracle):
    shape = SHAPES[1]
    f = field(shape)
    enc = encode_seg(ctx, f, 1e-6, 4096, wtflag=0)
    assert enc["wlev"] == 0
    planes = planes_of(enc, f.size)
    for p in sorted({1, enc["nlay"]}):
        want = expected(oracle, planes, enc, shape, 0, p)
        h64, h32, d64 = decode_all_ways(ctx, shape, 0, enc, p)
        assert same_bits(h64, want) and same_bits(d64, want) and same_bits(h32, want.astype(np.float32)), p
    out = np.empty(api.lowres_shape(shape, 1))
    with pytest.raises(api.WaveRangeError) as e:
        ctx.decode_host_seg_lowres(out, shape, 1, enc)
    assert "error -1" in str(e.value), str(e.value)
    # a constant field comes back as midval at the box's size
    flat = np.full((8, 6, 10), 3.25)
    enc, _ = ctx.encode_host_seg(flat, 1e-6)
    assert enc["nlay"] == 0 and enc["ntot_enc"] == 0
    for level in LEVELS:
        h64, h32, d64 = decode_all_ways(ctx, flat.shape, level, enc, 0)
        assert h64.shape == api.lowres_shape(flat.shape, level)
        assert np.all(h64 == 3.25) and np.all(d64 == 3.25) and np.all(h32 == np.float32(3.25)), level


# ---- only what is needed is read ---------------------------------------------------------------------------------------
def needed_sets(enc, shape, level):
    """Per plane: (seg, needed ids by brute force, segment lengths from the index)."""
    out = []
    for blob in split_planes(enc):
        seg, nseg = (int(v) for v in blob[4:12].view("<u4"))
        lens = blob[12:12 + 4 * nseg].view("<u4").astype(np.int64)
        out.append((seg, brute_force_segments(shape[2], shape[1], shape[0], level, seg), lens))
    return out


def masked(enc, shape, level):
    """A copy of the stream in which every byte of every segment the level does not need is 0xFF; the indices stay."""
    data = enc["data"].copy()
    at = 0
    for (seg, need, lens), ln in zip(needed_sets(enc, shape, level), enc["len_enc_vec"]):
        start = at + 12 + 4 * lens.size + np.concatenate(([0], np.cumsum(lens)))
        keep = np.zeros(lens.size, dtype=bool)
        keep[need] = True
        for k in np.flatnonzero(~keep):
            data[start[k]:start[k + 1]] = 0xFF
        at += ln
    return dict(enc, data=data)


@pytest.mark.parametrize("seg", [4096, 59904])
def test_only_needed_segments_are_read(ctx, oracle, seg):
    shape = SHAPES[0]
    f = field(shape)
    enc = encode_seg(ctx, f, 1e-6, seg)
    if seg == 4096:
        enc = recut(enc, planes_of(enc, f.size), (4096, 59904, 1024))
    planes = planes_of(enc, f.size)
    other = encode_seg(ctx, field(shape, seed=77), 1e-6, seg)
    for level in range(1, 5):
        bshape = api.lowres_shape(shape, level)
        want = expected(oracle, planes, enc, shape, level, enc["nlay"])
        clean, dirty, stale = np.empty(bshape), np.empty(bshape), np.empty(bshape)
        ctx.decode_host_seg_lowres(clean, shape, level, enc)
        bad = masked(enc, shape, level)
        assert not np.array_equal(bad["data"], enc["data"])
        s0, b0 = api.stat(api.STAT_LOWRES_SEGMENTS), api.stat(api.STAT_LOWRES_BYTES_UP)
        ctx.decode_host_seg_lowres(dirty, shape, level, bad)
        ds, db = api.stat(api.STAT_LOWRES_SEGMENTS) - s0, api.stat(api.STAT_LOWRES_BYTES_UP) - b0
        assert same_bits(clean, want) and same_bits(dirty, want), (seg, level)
        sets = needed_sets(enc, shape, level)
        assert ds == sum(need.size for _, need, _ in sets), (seg, level, ds)
        runs = sum(1 + int(np.count_nonzero(np.diff(need) != 1)) for _, need, _ in sets)
        payload = sum(int(lens[need].sum()) for _, need, lens in sets)
        assert 0 < db <= payload + 32 * runs, (seg, level, db, payload, runs)
        # the plane buffers of the context hold another field's symbols now
        full = np.empty_like(f)
        ctx.decode_host_seg(full, other)
        ctx.decode_host_seg_lowres(stale, shape, level, bad)
        assert same_bits(stale, want), (seg, level, "stale planes")
        # fewer planes: fewer segments
        s0 = api.stat(api.STAT_LOWRES_SEGMENTS)
        ctx.decode_host_seg_lowres(dirty, shape, level, bad, 1)
        assert api.stat(api.STAT_LOWRES_SEGMENTS) - s0 == sets[0][1].size
        assert same_bits(dirty, expected(oracle, planes, enc, shape, level, 1)), (seg, level, "one plane")


CHUNKED = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
from oracle.loader import Oracle
from waverange_amd import api, synth
import test_gpu_lowres as t
api.set_verbosity(0)
shape = (128, 128, 128)
with api.Context(0) as ctx:
    f = synth.field(128, 128, 128, seed=13)
    enc = t.encode_seg(ctx, f, 1e-6, 59904)
    t.check_stream(ctx, Oracle(), shape, enc, t.planes_of(enc, f.size), "chunked")
print("ok")
"""


def test_planes_in_chunks(tmp_path):
    """WR_PLANE_CHUNK_MB=1: a 128^3 plane lives in two chunks, so the listed segments and the box's runs go through the
    chunk table."""
    script = tmp_path / "child.py"
    script.write_text(CHUNKED % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, str(script)], env=dict(os.environ, WR_PLANE_CHUNK_MB="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-3000:]


# ---- errors -------------------------------------------------------------------------------------------------------------
def test_flipped_count_table_then_next_call(ctx, oracle):
    """A flipped count-table byte inside a needed segment: WR_ERR_STREAM, and the context goes on working.  Run once."""
    shape = SHAPES[1]
    f = field(shape)
    enc = encode_seg(ctx, f, 1e-6, 4096)
    planes = planes_of(enc, f.size)
    level = 2
    want = expected(oracle, planes, enc, shape, level, enc["nlay"])
    out = np.empty(api.lowres_shape(shape, level))
    ctx.decode_host_seg_lowres(out, shape, level, enc)
    assert same_bits(out, want)
    sets = needed_sets(enc, shape, level)
    seg, need, lens = sets[0]
    k = int(need[len(need) // 2])
    at = 12 + 4 * lens.size + int(lens[:k].sum()) + 40  # inside the 256 counts at the head of segment k's stream
    bad = dict(enc, data=enc["data"].copy())
    bad["data"][at] ^= 0x55
    with pytest.raises(api.WaveRangeError):  # (the host reference refuses the segment too: its counts no longer add up)
        api.seg_decode_host_ref(split_planes(bad)[0], f.size)
    with pytest.raises(api.WaveRangeError) as e:
        ctx.decode_host_seg_lowres(out, shape, level, bad)
    assert "error -4" in str(e.value), str(e.value)
    out[:] = 0
    ctx.decode_host_seg_lowres(out, shape, level, enc)
    assert same_bits(out, want)
    # the same byte in a segment the level does not need changes nothing
    other = np.setdiff1d(np.arange(lens.size), need)
    assert other.size
    k = int(other[0])
    ok = dict(enc, data=enc["data"].copy())
    ok["data"][12 + 4 * lens.size + int(lens[:k].sum()) + 40] ^= 0x55
    out[:] = 0
    ctx.decode_host_seg_lowres(out, shape, level, ok)
    assert same_bits(out, want)


def test_refusals(ctx):
    shape = SHAPES[1]
    f = field(shape)
    enc = encode_seg(ctx, f, 1e-3, 4096)
    out = np.empty(api.lowres_shape(shape, 1))
    # a malformed index is refused before anything is launched
    for plane in (0, enc["nlay"] - 1):
        first = sum(enc["len_enc_vec"][:plane])
        for at, what in ((0, "magic"), (4, "segment"), (8, "segment count"), (12, "add up")):
            bad = dict(enc, data=enc["data"].copy())
            bad["data"][first + at] ^= 1
            s0 = api.stat(api.STAT_LOWRES_SEGMENTS)
            with pytest.raises(api.WaveRangeError) as e:
                ctx.decode_host_seg_lowres(out, shape, 1, bad, 1)  # (the index of an unused plane is validated too)
            assert "error -4" in str(e.value) and what in str(e.value), str(e.value)
            assert api.stat(api.STAT_LOWRES_SEGMENTS) == s0
    info = api.EncInfo.from_dict(enc)
    data = enc["data"]
    fn = api.lib().wr_decode_host_seg_lowres
    nz, ny, nx = shape
    big = np.empty(shape)
    for level, p in ((5, 0), (-1, 0), (1, enc["nlay"] + 1), (1, -1)):
        assert fn(ctx.h, big.ctypes.data, nx, ny, nz, level, p, api.C.byref(info), data.ctypes.data, data.size, None) == -1, (level, p)
    ctx.decode_host_seg_lowres(out, shape, 1, enc)  # and the context goes on working


# ---- accuracy: a condition, not a measurement --------------------------------------------------------------------------
@pytest.mark.parametrize("tol", TOLS)
@pytest.mark.parametrize("shape", SHAPES)
def test_accuracy(ctx, oracle, shape, tol):
    """max |D(r, nlay) - s * box_r(forward_r(f))| <= tolrel * max|f|: the bound the full decode keeps.  The oracle alone
    meets it at <= 0.30 of the bound on these inputs."""
    f = field(shape)
    enc = encode_seg(ctx, f, tol, 59904)
    bound = tol * np.abs(f).max()
    for level in range(1, 5):
        bz, by, bx = api.lowres_shape(shape, level)
        truth = oracle.cdf97_3d(f, level)[:bz, :by, :bx] * scale(shape, level)
        got = np.empty((bz, by, bx))
        ctx.decode_host_seg_lowres(got, shape, level, enc)
        err = np.abs(got - truth).max()
        print("accuracy shape=%s tol=%g level=%d: %.3f of the bound" % (shape, tol, level, err / bound))
        assert err <= bound, (shape, tol, level, err / bound)
