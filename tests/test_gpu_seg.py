"""Segmented plane streams ("WRS1") on the GPU: the coder kernels against the host reference of the format, the codec-level
entry points against the reference-format path.  Every comparison is equality against code that is pinned to the reference
(wr_range_encode through wr_seg_encode_host_ref, encode_host / decode_host): no tolerance appears anywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest

from util import ROOT, bits_equal, kat_plane, sha_big
from waverange_amd import api, synth

pytestmark = pytest.mark.gpu

SEGS = [4096, 59904]


@pytest.fixture(scope="module")
def ctx():
    api.set_verbosity(0)
    with api.Context(0) as c:
        yield c


def quantizer_planes(ctx, f, tol, wtflag=1):
    """The quantized planes of a field as wr_dev_encode_planes leaves them, as numpy arrays, and the header record."""
    n = f.size
    pitch = api.lib().wr_plane_pitch(n)
    buf, planes = ctx.to_device(f), ctx.alloc(pitch * api.NLAYMAX)
    try:
        info = ctx.encode_planes(buf, f.shape, tol, planes, wtflag)
        return [planes.download(np.uint8, n, offset=l * pitch).copy() for l in range(info.nlay)], info
    finally:
        buf.free()
        planes.free()


def stage_planes(ctx):
    out = []
    for kind in ("uniform", "skewed", "sparse"):
        for n in (2, 4097, 200000, 3 * 59904 + 7):
            out.append(("%s/%d" % (kind, n), kat_plane(kind, n)))
    for shape in ((64, 64, 64), (77, 129, 200)):
        f = synth.field(shape[2], shape[1], shape[0], seed=31)
        ps, _ = quantizer_planes(ctx, f, 1e-6)
        out += [("synth%s/plane%d" % (shape, l), p) for l, p in enumerate(ps)]
    return out


@pytest.mark.parametrize("seg", SEGS)
def test_stage_level_matches_host_ref(ctx, seg):
    for name, p in stage_planes(ctx):
        want = api.seg_encode_host_ref(p, seg)
        got = ctx.seg_encode_plane(p, seg)
        assert got.size == want.size and np.array_equal(got, want), (name, seg, got.size, want.size)
        sym, bad = ctx.seg_decode_plane(want, p.size)
        assert bad == 0 and np.array_equal(sym, p), (name, seg)


def test_stage_level_edges(ctx):
    blob = ctx.seg_encode_plane(np.zeros(0, np.uint8), 4096)
    assert blob.tobytes() == api.seg_encode_host_ref(np.zeros(0, np.uint8), 4096).tobytes() and blob.size == 12
    sym, bad = ctx.seg_decode_plane(blob, 0)
    assert sym.size == 0 and bad == 0
    for n in (1, 15, 16, 17):
        p = (np.arange(n) * 37 % 256).astype(np.uint8)
        assert np.array_equal(ctx.seg_encode_plane(p, 16), api.seg_encode_host_ref(p, 16)), n
        assert np.array_equal(ctx.seg_decode_plane(api.seg_encode_host_ref(p, 16), n)[0], p), n
    with pytest.raises(api.WaveRangeError):
        ctx.seg_encode_plane(kat_plane("uniform", 100), 60000)
    # a malformed index is refused before anything is launched
    good = api.seg_encode_host_ref(kat_plane("skewed", 10000), 4096)
    for at, what in ((0, "magic"), (4, "segment"), (8, "segment count"), (12, "add up")):
        bad_blob = good.copy()
        bad_blob[at] ^= 1
        with pytest.raises(api.WaveRangeError) as e:
            ctx.seg_decode_plane(bad_blob, 10000)
        assert what in str(e.value), str(e.value)
    # the stage-level encoder refuses a buffer that is one byte short
    p = kat_plane("skewed", 10000)
    d_sym, d_blob = ctx.to_device(p), ctx.alloc(good.size + 16)
    try:
        got = api.C.c_size_t(0)
        rc = api.lib().wr_dev_seg_encode(ctx.h, d_sym.ptr, p.size, 4096, d_blob.ptr, good.size - 1, api.C.byref(got))
        assert rc == -5, rc  # WR_ERR_OVERFLOW
        assert api.lib().wr_dev_seg_encode(ctx.h, d_sym.ptr, p.size, 4096, d_blob.ptr, good.size, api.C.byref(got)) == 0 and got.value == good.size
    finally:
        d_sym.free()
        d_blob.free()


def split_planes(enc):
    out, at = [], 0
    for ln in enc["len_enc_vec"]:
        out.append(enc["data"][at:at + ln])
        at += ln
    return out


def check_codec(ctx, f, tol, wtflag, seg, cutoff=None, m=(1, 1, 1), f32=False):
    """One field through the segmented pair and through the reference-format pair; everything must agree."""
    what = (f.shape, tol, wtflag, seg, m, f32)
    if f32:
        f = f.astype(np.float32)
        ref, _ = ctx.encode_host_f32(f, tol, wtflag, cutoff=cutoff, m=m)
        enc, tm = ctx.encode_host_seg_f32(f, tol, wtflag, seg, cutoff=cutoff, m=m)
    else:
        ref, _ = ctx.encode_host(f, tol, wtflag, cutoff=cutoff, m=m)
        enc, tm = ctx.encode_host_seg(f, tol, wtflag, seg, cutoff=cutoff, m=m)
    ref["data"], enc["data"] = ref["data"].copy(), enc["data"].copy()
    # header scalars bit-identical to encode_host's
    for k in ("tolabs", "midval", "halfspanval"):
        assert float(enc[k]).hex() == float(ref[k]).hex(), (what, k)
    assert enc["wlev"] == ref["wlev"] and enc["nlay"] == ref["nlay"], what
    assert bits_equal(enc["deps_vec"], ref["deps_vec"]) and bits_equal(enc["minval_vec"], ref["minval_vec"]), what
    assert enc["ntot_enc"] == sum(enc["len_enc_vec"]) == enc["data"].size, what
    # every plane blob is the host reference's blob of that plane
    if cutoff is None:
        planes, info = quantizer_planes(ctx, np.ascontiguousarray(f, dtype=np.float64), tol, wtflag)
        assert info.nlay == enc["nlay"], what
        for l, (blob, p) in enumerate(zip(split_planes(enc), planes)):
            assert np.array_equal(blob, api.seg_encode_host_ref(p, seg)), (what, "plane %d" % l)
    else:  # (the stage-level call has no local cutoff: the planes come from the reference-format streams instead)
        for l, (blob, stream) in enumerate(zip(split_planes(enc), split_planes(ref))):
            p, got = api.range_decode(stream, f.size)
            assert got == f.size and np.array_equal(blob, api.seg_encode_host_ref(p, seg)), (what, "plane %d" % l)
    # reconstruction bit-identical to decode_host of the reference-format stream
    want, rec = np.empty_like(f), np.empty_like(f)
    if f32:
        ctx.decode_host_f32(want, ref)
        ctx.decode_host_seg_f32(rec, enc)
        assert np.array_equal(rec.view(np.uint32), want.view(np.uint32)), what
    else:
        ctx.decode_host(want, ref)
        ctx.decode_host_seg(rec, enc)
        assert np.array_equal(rec.view(np.uint64), want.view(np.uint64)), what
    assert tm["rangecoder"] > 0 and all(t > 0 for t in tm["plane_coder_s"][:enc["nlay"]]), tm
    # one byte short: WR_ERR_OVERFLOW
    short = np.empty(enc["ntot_enc"] - 1, dtype=np.uint8)
    with pytest.raises(api.WaveRangeError) as e:
        (ctx.encode_host_seg_f32 if f32 else ctx.encode_host_seg)(f, tol, wtflag, seg, out=short, cutoff=cutoff, m=m)
    assert "error -5" in str(e.value), str(e.value)
    return enc, rec


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("wtflag", [0, 1])
def test_codec_level(ctx, wtflag, f32):
    f = synth.field(200, 129, 77, seed=7)
    check_codec(ctx, f, 1e-6, wtflag, 59904, f32=f32)
    check_codec(ctx, synth.field(64, 64, 64, seed=8), 1e-3, wtflag, 4096, f32=f32)


def test_codec_level_local_cutoff(ctx):
    f = synth.field(64, 48, 40, seed=9)
    cutoff = np.array([1e-3, 1e-5, 1e-4, 1e-6, 1e-5, 1e-3, 1e-4, 1e-5], dtype=np.float64)
    check_codec(ctx, f, None, 1, 4096, cutoff=cutoff, m=(2, 2, 2))


def test_codec_level_device_field_and_trivial(ctx):
    f = synth.field(96, 80, 72, seed=10)
    want_enc, _ = ctx.encode_host_seg(f, 1e-5, 1, 0)
    want_enc["data"] = want_enc["data"].copy()
    buf = ctx.to_device(f)
    try:
        enc, _ = ctx.encode_seg(buf, f.shape, 1e-5, 1, 0)
        assert np.array_equal(enc["data"], want_enc["data"]) and enc["len_enc_vec"] == want_enc["len_enc_vec"]
        ctx.decode_seg(buf, f.shape, enc)
        rec = buf.download(np.float64, f.size).reshape(f.shape)
    finally:
        buf.free()
    want = np.empty_like(f)
    ctx.decode_host_seg(want, want_enc)
    assert np.array_equal(rec.view(np.uint64), want.view(np.uint64))
    # a constant field: no planes at all, as the reference-format path
    flat = np.full((8, 8, 8), 3.25)
    enc, _ = ctx.encode_host_seg(flat, 1e-6)
    assert enc["nlay"] == 0 and enc["ntot_enc"] == 0
    out = np.empty_like(flat)
    ctx.decode_host_seg(out, enc)
    assert np.array_equal(out, flat)


def test_flipped_payload_then_next_field(ctx):
    """Payload bytes flipped behind a valid index: WR_ERR_STREAM or a field, and the context goes on working.  Run once."""
    f = synth.field(64, 64, 64, seed=11)
    enc, _ = ctx.encode_host_seg(f, 1e-6, 1, 4096)
    enc["data"] = enc["data"].copy()
    good = np.empty_like(f)
    ctx.decode_host_seg(good, enc)
    bad = dict(enc, data=enc["data"].copy())
    rng = np.random.default_rng(3)
    at = 0
    for ln in enc["len_enc_vec"]:
        seg, streams = api.seg_split(bad["data"][at:at + ln])
        first = at + 12 + 4 * len(streams)
        idx = rng.integers(first, at + ln, 64)
        bad["data"][idx] ^= rng.integers(1, 256, 64).astype(np.uint8)
        at += ln
    out = np.empty_like(f)
    try:
        ctx.decode_host_seg(out, bad)
    except api.WaveRangeError as e:
        assert "error -4" in str(e), str(e)  # WR_ERR_STREAM
    # the next field on the same context
    g = synth.field(72, 56, 40, seed=12)
    check_codec(ctx, g, 1e-5, 1, 4096)
    again = np.empty_like(f)
    ctx.decode_host_seg(again, enc)
    assert np.array_equal(again.view(np.uint64), good.view(np.uint64))


CHUNKED = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
from waverange_amd import api, synth
import test_gpu_seg as t
api.set_verbosity(0)
with api.Context(0) as ctx:
    f = synth.field(128, 128, 128, seed=13)
    t.check_codec(ctx, f, 1e-6, 1, 59904)
    t.check_codec(ctx, f, 1e-6, 1, 4096, f32=True)
print("ok")
"""


def test_segments_straddle_plane_chunks(tmp_path):
    """WR_PLANE_CHUNK_MB=1: a 128^3 plane lives in two chunks of 1 MiB and 59904 does not divide a chunk, so segments
    straddle the chunk boundary, in the encoder's loads and in the decoder's stores."""
    script = tmp_path / "child.py"
    script.write_text(CHUNKED % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, str(script)], env=dict(os.environ, WR_PLANE_CHUNK_MB="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-3000:]


def test_512_cubed_round_trip(ctx):
    f = api.pinned_array((512, 512, 512))
    for z in range(0, 512, 64):
        f[z:z + 64] = synth.field(512, 512, 512, seed=2024, z0=z, z1=z + 64)
    ref, _ = ctx.encode_host(f, 1e-3)
    ref["data"] = ref["data"].copy()
    enc, _ = ctx.encode_host_seg(f, 1e-3)
    enc["data"] = enc["data"].copy()
    assert enc["nlay"] == ref["nlay"] and bits_equal(enc["deps_vec"], ref["deps_vec"]) and bits_equal(enc["minval_vec"], ref["minval_vec"])
    out = api.pinned_array((512, 512, 512))
    ctx.decode_host(out, ref)
    want = sha_big(out)
    out[:] = 0
    ctx.decode_host_seg(out, enc)
    assert sha_big(out) == want
