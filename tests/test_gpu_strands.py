"""Stranded segments ("WRS3") on the GPU: the coder kernels against the host reference of the format, the codec-level entry
points, the low-resolution and region decodes against the same calls on the WRS1 stream of the same field.  Every comparison
is equality: no tolerance appears anywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest

from util import ROOT, bits_equal, kat_plane
from waverange_amd import api, synth

pytestmark = pytest.mark.gpu

SEGS = [4096, 59904]
KS = [1, 8, 32]


@pytest.fixture(scope="module")
def ctx():
    api.set_verbosity(0)
    with api.Context(0) as c:
        yield c


def quantizer_planes(ctx, f, tol, wtflag=1):
    n = f.size
    pitch = api.lib().wr_plane_pitch(n)
    buf, planes = ctx.to_device(f), ctx.alloc(pitch * api.NLAYMAX)
    try:
        info = ctx.encode_planes(buf, f.shape, tol, planes, wtflag)
        return [planes.download(np.uint8, n, offset=l * pitch).copy() for l in range(info.nlay)]
    finally:
        buf.free()
        planes.free()


_PLANES = []


def stage_planes(ctx):
    """Computed once, shared by the parametrised cases, never written to."""
    if not _PLANES:
        for kind in ("uniform", "skewed", "sparse"):
            for n in (2, 4097, 200000, 3 * 59904 + 7):
                _PLANES.append(("%s/%d" % (kind, n), kat_plane(kind, n)))
        for shape in ((64, 64, 64), (77, 129, 200)):
            f = synth.field(shape[2], shape[1], shape[0], seed=31)
            _PLANES.extend(("synth%s/plane%d" % (shape, l), p) for l, p in enumerate(quantizer_planes(ctx, f, 1e-6)))
    return _PLANES


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("seg", SEGS)
def test_stage_level_matches_host_ref(ctx, seg, K):
    for name, p in stage_planes(ctx):
        want = api.seg_encode_host_ref_strands(p, seg=seg, strands=K)
        got = ctx.seg_encode_plane(p, seg, strands=K)
        assert got.size == want.size and np.array_equal(got, want), (name, seg, K, got.size, want.size)
        sym, bad = ctx.seg_decode_plane(want, p.size)
        assert bad == 0 and np.array_equal(sym, p), (name, seg, K)


def test_stage_level_edges(ctx):
    empty = np.zeros(0, np.uint8)
    blob = ctx.seg_encode_plane(empty, 16, strands=1)
    assert blob.tobytes() == api.seg_encode_host_ref_strands(empty, seg=16, strands=1).tobytes() and blob.size == 20
    sym, bad = ctx.seg_decode_plane(blob, 0)
    assert sym.size == 0 and bad == 0
    for n in (1, 15, 16, 17):
        p = (np.arange(n) * 37 % 256).astype(np.uint8)
        want = api.seg_encode_host_ref_strands(p, seg=16, strands=1)
        assert np.array_equal(ctx.seg_encode_plane(p, 16, strands=1), want), n
        assert np.array_equal(ctx.seg_decode_plane(want, n)[0], p), n
    for seg, K in ((4096, 8), (4096, 32), (59904, 8)):  # a last segment of 17 symbols: one strand of 16, one of 1, empty ones
        p = kat_plane("skewed", seg + 17)
        want = api.seg_encode_host_ref_strands(p, seg=seg, strands=K)
        assert np.array_equal(ctx.seg_encode_plane(p, seg, strands=K), want), (seg, K)
        assert np.array_equal(ctx.seg_decode_plane(want, p.size)[0], p), (seg, K)
    assert np.array_equal(ctx.seg_encode_plane(kat_plane("skewed", 10000), 4096, strands=0), api.seg_encode_host_ref_strands(kat_plane("skewed", 10000), seg=4096, strands=8))
    for seg, K in ((4096, 3), (4096, 64), (16, 2), (60000, 8)):
        with pytest.raises(api.WaveRangeError):
            ctx.seg_encode_plane(kat_plane("uniform", 100), seg, strands=K)
    # a malformed header or index is refused before anything is launched
    p = kat_plane("skewed", 10000)
    good = api.seg_encode_host_ref_strands(p, seg=4096, strands=8)
    for at, what in ((0, "magic"), (4, "segment"), (8, "segment count"), (13, "brick"), (16, "strand"), (20, "multiple of 4"), (21, "add up")):
        bad_blob = good.copy()
        bad_blob[at] ^= 1
        with pytest.raises(api.WaveRangeError) as e:
            ctx.seg_decode_plane(bad_blob, 10000)
        assert what in str(e.value), str(e.value)
    # a record whose length words do not add up is flagged by the kernel, and only that one
    bad_blob = good.copy()
    bad_blob[20 + 12 + 4] ^= 4  # slen[0] of record 0
    d_blob, d_sym = ctx.to_device(bad_blob), ctx.alloc(10000 + 16)
    try:
        nbad = api.C.c_size_t(0)
        rc = api.lib().wr_dev_seg_decode(ctx.h, d_blob.ptr, bad_blob.size, d_sym.ptr, 10000, api.C.byref(nbad))
        assert rc == -4 and nbad.value == 1, (rc, nbad.value)  # WR_ERR_STREAM
    finally:
        d_blob.free()
        d_sym.free()
    # the stage-level encoder refuses a buffer that is one byte short
    d_sym, d_blob = ctx.to_device(p), ctx.alloc(good.size + 16)
    try:
        got = api.C.c_size_t(0)
        rc = api.lib().wr_dev_seg_encode_strands(ctx.h, d_sym.ptr, p.size, 4096, 8, d_blob.ptr, good.size - 1, api.C.byref(got))
        assert rc == -5, rc  # WR_ERR_OVERFLOW
        assert api.lib().wr_dev_seg_encode_strands(ctx.h, d_sym.ptr, p.size, 4096, 8, d_blob.ptr, good.size, api.C.byref(got)) == 0
        assert got.value == good.size and np.array_equal(d_blob.download(np.uint8, good.size), good)
    finally:
        d_sym.free()
        d_blob.free()


def split_planes(enc):
    out, at = [], 0
    for ln in enc["len_enc_vec"]:
        out.append(enc["data"][at:at + ln])
        at += ln
    return out


def check_codec(ctx, f, tol, wtflag, seg, K, brick, cutoff=None, m=(1, 1, 1), f32=False):
    """One field through the WRS3 pair and through the WRS1 pair; everything must agree."""
    what = (f.shape, tol, wtflag, seg, K, brick, m, f32)
    if f32:
        f = f.astype(np.float32)
    encode = ctx.encode_host_seg_f32 if f32 else ctx.encode_host_seg
    decode = ctx.decode_host_seg_f32 if f32 else ctx.decode_host_seg
    ref, _ = encode(f, tol, wtflag, seg, cutoff=cutoff, m=m)
    ref["data"] = ref["data"].copy()
    enc, tm = encode(f, tol, wtflag, seg, cutoff=cutoff, m=m, brick=brick, strands=K)
    enc["data"] = enc["data"].copy()
    # header scalars bit-identical to encode_host_seg's
    for k in ("tolabs", "midval", "halfspanval"):
        assert float(enc[k]).hex() == float(ref[k]).hex(), (what, k)
    assert enc["wlev"] == ref["wlev"] and enc["nlay"] == ref["nlay"], what
    assert bits_equal(enc["deps_vec"], ref["deps_vec"]) and bits_equal(enc["minval_vec"], ref["minval_vec"]), what
    assert enc["ntot_enc"] == sum(enc["len_enc_vec"]) == enc["data"].size, what
    # every plane blob is the host reference's blob of that plane
    for l, (blob, b1) in enumerate(zip(split_planes(enc), split_planes(ref))):
        plane = api.seg_decode_host_ref(b1, f.size)
        assert np.array_equal(blob, api.seg_encode_host_ref_strands(plane, f.shape, enc["wlev"], brick, seg, K)), (what, "plane %d" % l)
    # reconstruction bit-identical to decode_host_seg of the WRS1 stream
    want, rec = np.empty_like(f), np.empty_like(f)
    decode(want, ref)
    decode(rec, enc)
    assert np.array_equal(rec.view(np.uint8), want.view(np.uint8)), what
    assert tm["rangecoder"] > 0 and all(t > 0 for t in tm["plane_coder_s"][:enc["nlay"]]), tm
    # one byte short: WR_ERR_OVERFLOW
    short = np.empty(enc["ntot_enc"] - 1, dtype=np.uint8)
    with pytest.raises(api.WaveRangeError) as e:
        encode(f, tol, wtflag, seg, out=short, cutoff=cutoff, m=m, brick=brick, strands=K)
    assert "error -5" in str(e.value), str(e.value)
    return ref, enc


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("wtflag", [0, 1])
def test_codec_level(ctx, wtflag, f32):
    f = synth.field(200, 129, 77, seed=7)
    check_codec(ctx, f, 1e-6, wtflag, 59904, 8, 0, f32=f32)
    check_codec(ctx, f, 1e-6, wtflag, 59904, 32, 8, f32=f32)
    g = synth.field(64, 64, 64, seed=8)
    check_codec(ctx, g, 1e-3, wtflag, 4096, 32, 0, f32=f32)
    check_codec(ctx, g, 1e-3, wtflag, 4096, 1, 8, f32=f32)


def test_codec_level_local_cutoff(ctx):
    f = synth.field(64, 48, 40, seed=9)
    cutoff = np.array([1e-3, 1e-5, 1e-4, 1e-6, 1e-5, 1e-3, 1e-4, 1e-5], dtype=np.float64)
    check_codec(ctx, f, None, 1, 4096, 8, 0, cutoff=cutoff, m=(2, 2, 2))
    check_codec(ctx, f, None, 1, 4096, 8, 8, cutoff=cutoff, m=(2, 2, 2))


def test_codec_level_device_field_and_trivial(ctx):
    f = synth.field(96, 80, 72, seed=10)
    for brick in (0, 8):
        want_enc, _ = ctx.encode_host_seg(f, 1e-5, 1, 0, brick=brick, strands=0)
        want_enc["data"] = want_enc["data"].copy()
        assert bytes(want_enc["data"][:4]) == b"WRS3" and tuple(want_enc["data"][12:20].view("<u4")) == (brick, api.STRANDS_DEFAULT)
        buf = ctx.to_device(f)
        try:
            enc, _ = ctx.encode_seg(buf, f.shape, 1e-5, 1, 0, brick=brick, strands=0)
            assert np.array_equal(enc["data"], want_enc["data"]) and enc["len_enc_vec"] == want_enc["len_enc_vec"]
            ctx.decode_seg(buf, f.shape, enc)
            rec = buf.download(np.float64, f.size).reshape(f.shape)
        finally:
            buf.free()
        want = np.empty_like(f)
        ctx.decode_host_seg(want, want_enc)
        assert np.array_equal(rec.view(np.uint64), want.view(np.uint64))
    # a constant field: no planes at all
    flat = np.full((8, 8, 8), 3.25)
    enc, _ = ctx.encode_host_seg(flat, 1e-6, strands=8)
    assert enc["nlay"] == 0 and enc["ntot_enc"] == 0
    out = np.empty_like(flat)
    ctx.decode_host_seg(out, enc)
    assert np.array_equal(out, flat)
    # a bad strand count is WR_ERR_ARG
    with pytest.raises(api.WaveRangeError) as e:
        ctx.encode_host_seg(f, 1e-5, 1, 4096, strands=3)
    assert "error -1" in str(e.value) or "strands" in str(e.value), str(e.value)


# ---- low-resolution and region decode ----------------------------------------------------------------------------------------
def index_of(blob):
    """(bytes in front of the records, the records' lengths) of a WRS1 / WRS2 / WRS3 blob"""
    head = {b"WRS1": 12, b"WRS2": 16, b"WRS3": 20}[bytes(blob[:4])]
    nseg = int(blob[8:12].view("<u4")[0])
    return head + 4 * nseg, blob[head:head + 4 * nseg].view("<u4").astype(np.int64)


def masked(enc, needs):
    """A copy of the stream in which every payload byte outside the needed segments / records is 0xFF; the indices stay."""
    data = enc["data"].copy()
    at = 0
    for blob, need, ln in zip(split_planes(enc), needs, enc["len_enc_vec"]):
        front, lens = index_of(blob)
        start = at + front + np.concatenate(([0], np.cumsum(lens)))
        keep = np.zeros(lens.size, dtype=bool)
        keep[need] = True
        for k in np.flatnonzero(~keep):
            data[start[k]:start[k + 1]] = 0xFF
        at += ln
    assert not np.array_equal(data, enc["data"])
    return dict(enc, data=data)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def lowres_all_ways(ctx, shape, level, enc, p):
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


def roi_all_ways(ctx, shape, level, roi, enc, p):
    rshape = api.roi_shape(roi)
    h64, h32 = np.empty(rshape), np.empty(rshape, dtype=np.float32)
    ctx.decode_host_seg_roi(h64, shape, level, roi, enc, p)
    ctx.decode_host_seg_roi_f32(h32, shape, level, roi, enc, p)
    buf = ctx.alloc(max(h64.nbytes, 16))
    try:
        ctx.decode_seg_roi(buf, shape, level, roi, enc, p)
        d64 = buf.download(np.float64, h64.size).reshape(rshape)
    finally:
        buf.free()
    return h64, h32, d64


def stats():
    return np.array([api.stat(k) for k in (api.STAT_LOWRES_SEGMENTS, api.STAT_ROI_SEGMENTS)])


@pytest.mark.parametrize("brick", [0, 8])
@pytest.mark.parametrize("shape,roi", [((24, 400, 40), ((0, 24), (0, 4), (0, 40))), ((64, 64, 64), ((30, 34), (5, 6), (60, 64))),
                                       ((1, 50, 70), ((0, 1), (10, 20), (30, 41)))], ids=["24x400x40", "64x64x64", "1x50x70"])
def test_lowres_and_roi_match_the_wrs1_stream(ctx, shape, roi, brick):
    seg, K = 4096, 8
    f = synth.field(shape[2], shape[1], shape[0], seed=41)
    wrs1, _ = ctx.encode_host_seg(f, 1e-6, 1, seg)
    wrs1["data"] = wrs1["data"].copy()
    same, _ = ctx.encode_host_seg(f, 1e-6, 1, seg, brick=brick) if brick else (wrs1, None)  # the same order without strands
    same["data"] = same["data"].copy()
    enc, _ = ctx.encode_host_seg(f, 1e-6, 1, seg, brick=brick, strands=K)
    enc["data"] = enc["data"].copy()
    nlay = enc["nlay"]
    for level in (0, 2, 4):
        for p in sorted({1, nlay}):
            # low resolution
            need = api.seg_lowres_segments_blocked(shape, level, seg, 4, brick) if brick else api.seg_lowres_segments(shape, level, seg)
            want = lowres_all_ways(ctx, shape, level, wrs1, p)
            s0 = stats()
            lowres_all_ways(ctx, shape, level, same, p)
            s1 = stats()
            got = lowres_all_ways(ctx, shape, level, masked(enc, [need] * nlay) if need.size < index_of(split_planes(enc)[0])[1].size else enc, p)
            s2 = stats()
            assert all(same_bits(a, b) for a, b in zip(got, want)), (shape, brick, level, p, "lowres")
            assert np.array_equal(s2 - s1, s1 - s0) and (s1 - s0)[0] == 3 * need.size * p and (s1 - s0)[1] == 0, (shape, brick, level, p, s0, s1, s2)
            # the region, carried to the level's box
            box = api.lowres_shape(shape, level)
            r = tuple((lo >> level, min(n, max((lo >> level) + 1, -(-hi >> level)))) for (lo, hi), n in zip(roi, box))
            need = (api.seg_roi_segments_blocked(shape, level, r, seg, 4, brick) if brick else api.seg_roi_segments(shape, level, r, seg, wlev=4))
            want = roi_all_ways(ctx, shape, level, r, wrs1, p)
            s0 = stats()
            roi_all_ways(ctx, shape, level, r, same, p)
            s1 = stats()
            got = roi_all_ways(ctx, shape, level, r, masked(enc, [need] * nlay) if need.size < index_of(split_planes(enc)[0])[1].size else enc, p)
            s2 = stats()
            assert all(same_bits(a, b) for a, b in zip(got, want)), (shape, brick, level, p, "roi")
            assert np.array_equal(s2 - s1, s1 - s0) and (s1 - s0)[1] == 3 * need.size * p and (s1 - s0)[0] == 0, (shape, brick, level, p, s0, s1, s2)


# ---- chunks, corruption --------------------------------------------------------------------------------------------------------
CHUNKED = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
from waverange_amd import api, synth
import test_gpu_strands as t
api.set_verbosity(0)
with api.Context(0) as ctx:
    f = synth.field(128, 128, 128, seed=13)
    t.check_codec(ctx, f, 1e-6, 1, 59904, 8, 0)
    t.check_codec(ctx, f, 1e-6, 1, 4096, 8, 8, f32=True)
print("ok")
"""


def test_strands_straddle_plane_chunks(tmp_path):
    """WR_PLANE_CHUNK_MB=1: a 128^3 plane lives in two chunks of 1 MiB; at seg 59904 and K = 8 the strand length 7488 does not
    divide a chunk, so a strand straddles the chunk boundary, in the encoder's loads and in the decoder's stores."""
    script = tmp_path / "child.py"
    script.write_text(CHUNKED % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, str(script)], env=dict(os.environ, WR_PLANE_CHUNK_MB="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-3000:]


def test_flipped_payload_then_next_field(ctx):
    """Payload bytes flipped behind a valid index: WR_ERR_STREAM or a field, and the context goes on working.  Run once."""
    f = synth.field(64, 64, 64, seed=11)
    enc, _ = ctx.encode_host_seg(f, 1e-6, 1, 4096, strands=8)
    enc["data"] = enc["data"].copy()
    good = np.empty_like(f)
    ctx.decode_host_seg(good, enc)
    bad = dict(enc, data=enc["data"].copy())
    rng = np.random.default_rng(3)
    at = 0
    for blob, ln in zip(split_planes(enc), enc["len_enc_vec"]):
        front, _ = index_of(blob)
        idx = rng.integers(at + front, at + ln, 64)
        bad["data"][idx] ^= rng.integers(1, 256, 64).astype(np.uint8)
        at += ln
    out = np.empty_like(f)
    try:
        ctx.decode_host_seg(out, bad)
    except api.WaveRangeError as e:
        assert "error -4" in str(e), str(e)  # WR_ERR_STREAM
    # the next field on the same context
    g = synth.field(72, 56, 40, seed=12)
    check_codec(ctx, g, 1e-5, 1, 4096, 8, 0)
    again = np.empty_like(f)
    ctx.decode_host_seg(again, enc)
    assert np.array_equal(again.view(np.uint64), good.view(np.uint64))
