"""The segment and strand coder kernels (csrc/wr_segcoder.hip) on the planes that break coders: tests/coder_cases.py, whose
claims tests/test_coder_cases_cpu.py checks without a GPU.  Stage level: every case against the host reference of the format,
byte for byte, both ways.  Guard bands: the entry points on sub-ranges of larger buffers, capacity and symbol range exact.
Codec level: fields that carry a chosen plane through the quantizer (wtflag = 0), for the list decodes behind the region
decode.  Every comparison is equality; all inputs are well-formed planes and blobs."""
import os
import subprocess
import sys

import numpy as np
import pytest

import coder_cases as cc
from util import ROOT
from waverange_amd import api

pytestmark = pytest.mark.gpu

BAND, FILL = 256, 0xA5


@pytest.fixture(scope="module")
def ctx():
    api.set_verbosity(0)
    with api.Context(0) as c:
        yield c


_HOST = {}


def host_blob(c):
    """the host reference's blob of a case: computed once, shared by the tests, never written to"""
    if c not in _HOST:
        _, seg, K, _ = c
        p = cc.case_plane(c)
        blob = api.seg_encode_host_ref_strands(p, seg=seg, strands=K) if K else api.seg_encode_host_ref(p, seg)
        blob.flags.writeable = False
        _HOST[c] = blob
    return _HOST[c]


GRID_IDS = ["seg%d-%s" % (seg, "K%d" % K if K else "wrs1") for seg, K in cc.grid()]


@pytest.mark.parametrize("seg,K", cc.grid(), ids=GRID_IDS)
def test_stage_level_matches_host_ref(ctx, seg, K):
    for c in cc.stage_cases(seg, K):
        p, want = cc.case_plane(c), host_blob(c)
        got = ctx.seg_encode_plane(p, seg, strands=K or None)
        assert got.size == want.size and np.array_equal(got, want), (cc.case_id(c), got.size, want.size)
        sym, bad = ctx.seg_decode_plane(want, p.size)
        assert bad == 0 and np.array_equal(sym, p), cc.case_id(c)


def up16(v):
    return (v + 15) & ~15


def banded(ctx, payload, room):
    """a device buffer of BAND | room rounded up to 16 | BAND bytes, all FILL except `payload` at BAND; and its host image"""
    image = np.full(BAND + up16(room) + BAND, FILL, np.uint8)
    image[BAND:BAND + payload.size] = payload
    return ctx.to_device(image), image


@pytest.mark.parametrize("seg,K", cc.grid(), ids=GRID_IDS)
def test_guard_bands(ctx, seg, K):
    """Encoder: cap is the bound exactly.  Decoder: a symbol range of exactly n bytes.  Nothing outside the blob's bytes and the
    n symbols changes: both bands of both buffers, the bytes behind the blob up to the next multiple of 16, and the bytes
    [n, n rounded up to 16) of the symbol buffer."""
    lib = api.lib()
    for c in cc.guard_cases(seg, K):
        p, want = cc.case_plane(c), host_blob(c)
        n = p.size
        bound = api.seg_bound_strands(n, seg, K) if K else api.seg_bound(n, seg)
        # ---- encode
        d_sym, sym_image = banded(ctx, p, n)
        d_blob, blob_image = banded(ctx, np.zeros(0, np.uint8), bound)
        try:
            got = api.C.c_size_t(0)
            if K:
                rc = lib.wr_dev_seg_encode_strands(ctx.h, d_sym.ptr + BAND, n, seg, K, d_blob.ptr + BAND, bound, api.C.byref(got))
            else:
                rc = lib.wr_dev_seg_encode(ctx.h, d_sym.ptr + BAND, n, seg, d_blob.ptr + BAND, bound, api.C.byref(got))
            assert rc == 0 and got.value == want.size, (cc.case_id(c), rc, got.value, want.size)
            out = d_blob.download(np.uint8, blob_image.size)
            assert np.array_equal(out[BAND:BAND + want.size], want), cc.case_id(c)
            assert np.all(out[:BAND] == FILL) and np.all(out[BAND + bound:] == FILL), (cc.case_id(c), "the blob's bands")
            assert np.array_equal(d_sym.download(np.uint8, sym_image.size), sym_image), (cc.case_id(c), "the encoder wrote symbols")
        finally:
            d_sym.free()
            d_blob.free()
        # ---- decode
        d_blob, blob_image = banded(ctx, want, want.size)
        d_sym, sym_image = banded(ctx, np.zeros(0, np.uint8), n)
        try:
            bad = api.C.c_size_t(0)
            rc = lib.wr_dev_seg_decode(ctx.h, d_blob.ptr + BAND, want.size, d_sym.ptr + BAND, n, api.C.byref(bad))
            assert rc == 0 and bad.value == 0, (cc.case_id(c), rc, bad.value)
            out = d_sym.download(np.uint8, sym_image.size)
            assert np.array_equal(out[BAND:BAND + n], p), cc.case_id(c)
            assert np.all(out[:BAND] == FILL) and np.all(out[BAND + n:] == FILL), (cc.case_id(c), "the symbols' bands")
            assert np.array_equal(d_blob.download(np.uint8, blob_image.size), blob_image), (cc.case_id(c), "the decoder wrote to the blob")
        finally:
            d_sym.free()
            d_blob.free()


# ---- codec level: the list-decode kernels on hard planes ---------------------------------------------------------------------
def split_planes(enc):
    out, at = [], 0
    for ln in enc["len_enc_vec"]:
        out.append(enc["data"][at:at + ln])
        at += ln
    return out


def boxes(shape):
    """a corner voxel, an interior 4 x 1 x 4 box (as thick as the field if that is thinner), a full x-row, the last z-plane"""
    nz, ny, nx = shape
    return [((0, 1), (0, 1), (0, 1)), ((min(2, nz - 1), min(6, nz)), (20, 21), (60, 64)), ((nz - 1, nz), (33, 34), (0, nx)), ((nz - 1, nz), (0, ny), (0, nx))]


def crop(a, roi):
    (z0, z1), (y0, y1), (x0, x1) = roi
    return np.ascontiguousarray(a[z0:z1, y0:y1, x0:x1])


def check_hard_field(ctx, shape, seg, K, brick, kind, pi, rois=True):
    what = (shape, seg, K, brick, kind)
    n = int(np.prod(shape))
    want_plane = cc.codec_plane(kind, n, seg, K or 0)
    f = cc.codec_field(want_plane, shape, pi)
    enc, _ = ctx.encode_host_seg(f, 1e-3, 0, seg, brick=brick if K is not None else (brick or None), strands=K)
    enc["data"] = enc["data"].copy()
    assert enc["wlev"] == 0 and enc["nlay"] >= 1 and enc["deps_vec"][0] == 1.0 and enc["minval_vec"][0] == 0.0, what
    # every plane blob is the host reference's blob of that plane, and plane 0 is the chosen plane
    for l, blob in enumerate(split_planes(enc)):
        natural = api.seg_decode_host_ref_blocked(blob, shape, 0)
        if l == 0:
            assert np.array_equal(natural if pi is None else natural[pi], want_plane), what
        if K is not None:
            ref = api.seg_encode_host_ref_strands(natural, shape, 0, brick, seg, K)
        else:
            ref = api.seg_encode_host_ref_blocked(natural, shape, 0, brick, seg) if brick else api.seg_encode_host_ref(natural, seg)
        assert np.array_equal(blob, ref), (what, "plane %d" % l)
    # the reconstruction is decode_host's of the reference-format stream of the same field
    plain, _ = ctx.encode_host(f, 1e-3, 0)
    plain["data"] = plain["data"].copy()
    want, rec = np.empty_like(f), np.empty_like(f)
    ctx.decode_host(want, plain)
    ctx.decode_host_seg(rec, enc)
    assert np.array_equal(rec.view(np.uint64), want.view(np.uint64)), what
    if not rois:
        return
    # regions at level 0: the crop of the full decode, from the listed segments alone
    nseg = -(-n // seg)
    for roi in boxes(shape):
        need = api.seg_roi_segments_blocked(shape, 0, roi, seg, 0, brick) if brick else api.seg_roi_segments(shape, 0, roi, seg, wlev=0)
        got = np.empty(api.roi_shape(roi))
        s0 = api.stat(api.STAT_ROI_SEGMENTS)
        ctx.decode_host_seg_roi(got, shape, 0, roi, enc)
        launched = api.stat(api.STAT_ROI_SEGMENTS) - s0
        assert np.array_equal(got.view(np.uint64), crop(want, roi).view(np.uint64)), (what, roi)
        # The geometry decides how many segments a box needs: the last z-plane of a field one brick (or one voxel) thick
        # touches every brick, so there -- and only there -- the list is all of them.
        assert launched == need.size * enc["nlay"] <= nseg * enc["nlay"], (what, roi, launched, need.size)
        whole_by_geometry = roi == boxes(shape)[3] and (brick or shape[0] == 1)
        assert (need.size < nseg) == (not whole_by_geometry), (what, roi, need.size, nseg)
        if not whole_by_geometry:
            assert launched < nseg * enc["nlay"], (what, roi, launched)


@pytest.mark.parametrize("brick", cc.CODEC_BRICKS)
@pytest.mark.parametrize("shape", cc.CODEC_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_codec_level_hard_planes(ctx, shape, brick):
    pi = api.blocked_order(shape, 0, brick).astype(np.int64) if brick else None
    for seg in cc.CODEC_SEGS:
        for K in cc.CODEC_KS:
            for kind in cc.CODEC_KINDS:
                check_hard_field(ctx, shape, seg, K, brick, kind, pi)


# ---- plane chunks ------------------------------------------------------------------------------------------------------------
CHUNKED = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
from waverange_amd import api
import coder_cases as cc
import test_gpu_coder_cases as t
api.set_verbosity(0)
shape, seg = (16, 256, 512), 59904
n = 16 * 256 * 512
at = (1 << 20) // seg  # the segment that straddles the first chunk boundary
with api.Context(0) as ctx:
    for K in (None, 8, 32):
        L = cc.strand_len(seg, cc.plane_K(seg, K or 0))
        j = ((1 << 20) - at * seg) // L  # and its strand that does
        assert at * seg + j * L < (1 << 20) < at * seg + (j + 1) * L
        p = cc.plane("patchwork", n, seg, K or 0).copy()
        p[at * seg:(at + 1) * seg] = cc._adversarial(seg, L, None, j)
        plane = lambda kind, n_, seg_, K_: p
        cc.codec_plane = plane
        t.check_hard_field(ctx, shape, seg, K, 0, "patchwork+adversarial", None, rois=False)
print("ok")
"""


def test_hard_planes_straddle_plane_chunks(tmp_path):
    """WR_PLANE_CHUNK_MB=1: a 16 x 256 x 512 plane lives in two chunks of 1 MiB.  The patchwork plane at seg 59904, with the
    segment across the chunk boundary made adversarial in the strand that crosses it, through the codec as WRS1 and as WRS3 with
    K = 8 and 32: the encoder's loads and the decoder's stores of one lane change chunks inside a segment and inside a strand."""
    script = tmp_path / "child.py"
    script.write_text(CHUNKED % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, str(script)], env=dict(os.environ, WR_PLANE_CHUNK_MB="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-3000:]
