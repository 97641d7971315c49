"""The masked batch calls through the whole path on the GPU, against the loop of the single masked calls, which
test_gpu_masked_codec.py pins against numpy and the host definition of the blob.
Encode: wr_encode_*_seg_batch_masked -- for every field the info, every byte of the record (field part, then the WRM1 blob),
undefined, the bits of pad and mask_len are wr_encode_host_seg_masked's for that field alone, whatever else is in the batch and
in whatever order; the coder launches are counted.  One batch holds masked fields at two tolerances (different nlay), a field
without an undefined sample and one whose padded field is constant.
Decode: wr_decode_*_seg_batch_masked -- WRS1, WRS2 and WRS3 records, an unmasked one, constants with and without a blob in one
call, compared on integer views with wr_decode_host_seg_masked's output for each record alone; at most two coder launches.
Refusals and damage: every output buffer is pre-filled with a sentinel and must keep it."""
import struct

import numpy as np
import pytest

from waverange_amd import api, synth

pytestmark = pytest.mark.gpu

STAT_LAUNCHES = 18  # WR_STAT_BATCH_CODER_LAUNCHES
BELOW = -1e30
UNDEF = -9.99e33
SENTINEL = 4242.0
TOLS = (1e-7, 1e-2, 1e-5, 1e-5)  # per field of the batch below: the first two far apart, so that their plane counts differ
WRS1 = dict(brick=0, strands=0)
# (shape (nx, ny, nz), seg, format): the small boxes with the mask plane cut into several segments and a short last one
CASES = [
    ((33, 17, 9), 16, WRS1), ((33, 17, 9), 48, WRS1), ((37, 21, 13), 16, WRS1), ((37, 21, 13), 48, WRS1),
    ((64, 64, 64), 0, WRS1), ((64, 64, 64), 0, dict(brick=32, strands=0)), ((64, 64, 64), 0, dict(brick=0, strands=8)),
]


def cid(c):
    shape, seg, fmt = c
    return "%s.seg%d.%s" % ("x".join(map(str, shape)), seg, "wrs3" if fmt["strands"] else "wrs2" if fmt["brick"] else "wrs1")


@pytest.fixture(scope="module")
def ctx():
    api.set_verbosity(0)
    with api.Context(0) as c:
        yield c


def ints(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def u64(x):
    return np.float64(x).view(np.uint64)


def same_info(a, b):  # (test_gpu_masked_codec.same_info)
    for k in ("tolabs", "midval", "halfspanval"):
        assert u64(a[k]) == u64(b[k]), k
    assert (a["wlev"], a["nlay"], a["ntot_enc"], a["len_enc_vec"]) == (b["wlev"], b["nlay"], b["ntot_enc"], b["len_enc_vec"])
    for k in ("deps_vec", "minval_vec"):
        assert np.array_equal(np.asarray(a[k]).view(np.uint64), np.asarray(b[k]).view(np.uint64)), k


def same_record(got, want):
    same_info(got, want)
    assert np.array_equal(got["data"], want["data"])
    assert got["mask"]["undefined"] == want["mask"]["undefined"] and got["mask"]["mask_len"] == want["mask"]["mask_len"]
    assert u64(got["mask"]["pad"]) == u64(want["mask"]["pad"])
    for k in ("split_ms", "fill_ms", "mask_coder_ms"):
        assert np.isfinite(got["mask"][k]) and got["mask"][k] >= 0, k


_fields, _singles = {}, {}


def batch_fields(shape, dtype):
    """[masked, masked with another undefined set, no undefined sample, constant where defined]; read-only, built once"""
    key = (shape, np.dtype(dtype).name)
    if key not in _fields:
        nx, ny, nz = shape
        z, y, x = np.meshgrid(np.arange(nz) / nz, np.arange(ny) / ny, np.arange(nx) / nx, indexing="ij")
        g = np.sin(5.0 * x + 1.0) + np.cos(4.0 * y) + np.sin(3.0 * z + 2.0 * x)
        a = synth.field(nx, ny, nz, seed=31 + nx).astype(dtype)
        a[g > np.quantile(g, 0.7)] = dtype(UNDEF)
        a.reshape(-1)[[3, a.size // 2]] = [np.nan, np.inf]
        b = synth.field(nx, ny, nz, seed=77 + ny).astype(dtype)
        b[g < np.quantile(g, 0.2)] = np.nan
        c = synth.field(nx, ny, nz, seed=5).astype(dtype)
        d = np.full((nz, ny, nx), 2.5, dtype)
        d[g > np.quantile(g, 0.9)] = -np.inf
        out = [a, b, c, d]
        for f in out:
            f.setflags(write=False)
        _fields[key] = out
    return _fields[key]


def singles(ctx, case, dtype):
    """the loop of the single masked call over the fields of a case: the yardstick, encoded once"""
    shape, seg, fmt = case
    key = (cid(case), np.dtype(dtype).name)
    if key not in _singles:
        enc = ctx.encode_host_seg_masked if np.dtype(dtype) == np.float64 else ctx.encode_host_seg_masked_f32
        recs = []
        for f, tol in zip(batch_fields(shape, dtype), TOLS):
            rec, _ = enc(f, tol, BELOW, seg=seg, **fmt)
            rec["data"] = rec["data"].copy()
            rec["data"].setflags(write=False)
            recs.append(rec)
        assert recs[0]["nlay"] != recs[1]["nlay"] and recs[0]["mask"]["mask_len"] and recs[1]["mask"]["mask_len"]
        assert recs[2]["mask"]["undefined"] == 0 and recs[2]["mask"]["mask_len"] == 0 and recs[2]["nlay"] > 0
        assert recs[3]["nlay"] == 0 and recs[3]["ntot_enc"] == 0 and recs[3]["mask"]["mask_len"] > 0
        _singles[key] = recs
    return _singles[key]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", CASES, ids=cid)
def test_encode_batch_is_the_loop_of_the_single_call(ctx, case, dtype):
    shape, seg, fmt = case
    fields, want = batch_fields(shape, dtype), singles(ctx, case, dtype)
    enc = ctx.encode_host_seg_batch_masked if dtype is np.float64 else ctx.encode_host_seg_batch_masked_f32
    before = api.stat(STAT_LAUNCHES)
    recs, _ = enc(fields, list(TOLS), BELOW, seg=seg, **fmt)
    delta = api.stat(STAT_LAUNCHES) - before
    for got, w in zip(recs, want):
        same_record(got, w)
    assert delta == max(w["nlay"] for w in want) + 1
    # permuting the batch permutes the records
    order = [3, 1, 0, 2]
    recs, _ = enc([fields[i] for i in order], [TOLS[i] for i in order], BELOW, seg=seg, **fmt)
    for got, i in zip(recs, order):
        same_record(got, want[i])


@pytest.mark.parametrize("case", CASES, ids=cid)
def test_encode_batch_device_fields(ctx, case):
    shape, seg, fmt = case
    fields, want = batch_fields(shape, np.float64), singles(ctx, case, np.float64)
    bufs = [ctx.to_device(f) for f in fields]
    try:
        before = api.stat(STAT_LAUNCHES)
        recs, _ = ctx.encode_seg_batch_masked(bufs, fields[0].shape, list(TOLS), BELOW, seg=seg, **fmt)
        delta = api.stat(STAT_LAUNCHES) - before
    finally:
        for b in bufs:
            b.free()
    for got, w in zip(recs, want):
        same_record(got, w)
    assert delta == max(w["nlay"] for w in want) + 1


@pytest.mark.parametrize("case", [CASES[0], CASES[4], CASES[6]], ids=cid)
def test_batch_without_an_undefined_sample_is_the_plain_batch(ctx, case):
    shape, seg, fmt = case
    nx, ny, nz = shape
    fields = [synth.field(nx, ny, nz, seed=s) for s in (5, 6, 7)]
    tols = [1e-5, 1e-3, 1e-5]
    before = api.stat(STAT_LAUNCHES)
    recs, _ = ctx.encode_host_seg_batch_masked(fields, tols, BELOW, seg=seg, **fmt)
    delta = api.stat(STAT_LAUNCHES) - before
    if fmt["strands"]:
        want, _ = ctx.encode_host_seg_batch_strands(fields, tols, seg=seg, brick=fmt["brick"], strands=fmt["strands"])
    else:
        want, _ = ctx.encode_host_seg_batch(fields, tols, seg=seg, brick=fmt["brick"] or None)
    assert delta == max(w["nlay"] for w in want)
    for got, w in zip(recs, want):
        same_info(got, w)
        assert np.array_equal(got["data"], w["data"])
        assert got["mask"]["undefined"] == 0 and got["mask"]["mask_len"] == 0


# ---- decode
def decode_mix(ctx, shape, dtype):
    """records of one shape: WRS1 (mask cut at 16), WRS2, WRS3, an unmasked one, a constant with its blob, a constant without"""
    s1 = singles(ctx, (shape, 16, WRS1), dtype)
    s2 = singles(ctx, (shape, 0, dict(brick=32, strands=0)), dtype)
    s3 = singles(ctx, (shape, 0, dict(brick=0, strands=8)), dtype)
    bare = dict(s1[3], data=s1[3]["data"][:0])
    return [s1[0], s2[1], s3[0], s3[2], s1[3], bare, s2[0], s1[1]]


@pytest.mark.parametrize("fill", [np.nan, -9.99e33], ids=["nan", "finite"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", [(33, 17, 9), (64, 64, 64)], ids=lambda s: "x".join(map(str, s)))
def test_decode_batch_is_the_loop_of_the_single_call(ctx, shape, dtype, fill):
    recs = decode_mix(ctx, shape, dtype)
    nx, ny, nz = shape
    single = ctx.decode_host_seg_masked if dtype is np.float64 else ctx.decode_host_seg_masked_f32
    batch = ctx.decode_host_seg_batch_masked if dtype is np.float64 else ctx.decode_host_seg_batch_masked_f32
    want, want_masks = [], []
    for r in recs:
        out = np.full((nz, ny, nx), SENTINEL, dtype)
        want_masks.append(single(out, r, fill)[0])
        want.append(out)
    outs = [np.full((nz, ny, nx), SENTINEL, dtype) for _ in recs]
    before = api.stat(STAT_LAUNCHES)
    masks, _ = batch(outs, recs, fill)
    assert api.stat(STAT_LAUNCHES) - before <= 2
    for f, (o, w) in enumerate(zip(outs, want)):
        assert np.array_equal(ints(o), ints(w)), f
        assert masks[f]["undefined"] == want_masks[f]["undefined"] and masks[f]["mask_len"] == want_masks[f]["mask_len"], f
        assert u64(masks[f]["pad"]) == u64(want_masks[f]["pad"]), f
    if dtype is np.float64:  # the device form
        bufs = [ctx.to_device(np.full((nz, ny, nx), SENTINEL)) for _ in recs]
        try:
            before = api.stat(STAT_LAUNCHES)
            ctx.decode_seg_batch_masked(bufs, (nz, ny, nx), recs, fill)
            assert api.stat(STAT_LAUNCHES) - before <= 2
            got = [b.download(np.float64, nx * ny * nz).reshape(nz, ny, nx) for b in bufs]
        finally:
            for b in bufs:
                b.free()
        for f, (o, w) in enumerate(zip(got, want)):
            assert np.array_equal(ints(o), ints(w)), f


def test_decode_batch_of_constants_only(ctx):
    """no field has a plane: the masks are the call's only jobs"""
    shape = (33, 17, 9)
    s1 = singles(ctx, (shape, 16, WRS1), np.float64)
    recs = [s1[3], dict(s1[3], data=s1[3]["data"][:0]), s1[3]]
    want = []
    for r in recs:
        out = np.full((9, 17, 33), SENTINEL)
        ctx.decode_host_seg_masked(out, r, np.nan)
        want.append(out)
    outs = [np.full((9, 17, 33), SENTINEL) for _ in recs]
    ctx.decode_host_seg_batch_masked(outs, recs, np.nan)
    for o, w in zip(outs, want):
        assert np.array_equal(ints(o), ints(w))


# ---- refusals and damage
def test_encode_refusals(ctx):
    case = CASES[0]
    shape, seg, fmt = case
    fields, want = batch_fields(shape, np.float64), singles(ctx, case, np.float64)
    caps = [w["data"].size for w in want]
    room = max(caps) + 64

    def outs():
        return [np.full(room, 0xEE, np.uint8) for _ in fields]

    # a field with no defined sample
    bad = list(fields)
    bad[2] = np.full(fields[0].shape, np.nan)
    o = outs()
    with pytest.raises(api.WaveRangeError) as e:
        ctx.encode_host_seg_batch_masked(bad, list(TOLS), BELOW, seg=seg, outs=o, **fmt)
    assert "error -1" in str(e.value) and "field 2: no defined sample" in str(e.value), str(e.value)
    assert all((x == 0xEE).all() for x in o)
    bufs = [ctx.to_device(f) for f in bad]
    try:
        with pytest.raises(api.WaveRangeError) as e:
            ctx.encode_seg_batch_masked(bufs, fields[0].shape, list(TOLS), BELOW, seg=seg, outs=o, **fmt)
    finally:
        for b in bufs:
            b.free()
    assert "error -1" in str(e.value) and "field 2: no defined sample" in str(e.value), str(e.value)
    assert all((x == 0xEE).all() for x in o)
    # a NaN threshold
    with pytest.raises(api.WaveRangeError) as e:
        ctx.encode_host_seg_batch_masked(fields, list(TOLS), np.nan, seg=seg, outs=o, **fmt)
    assert "error -1" in str(e.value)
    assert all((x == 0xEE).all() for x in o)
    # caps[1] one byte short of field part + blob; exactly enough everywhere else
    o = outs()
    short = [x[:c] for x, c in zip(o, caps)]
    short[1] = short[1][:caps[1] - 1]
    with pytest.raises(api.WaveRangeError) as e:
        ctx.encode_host_seg_batch_masked(fields, list(TOLS), BELOW, seg=seg, outs=short, **fmt)
    assert "error -5" in str(e.value) and "field 1: " in str(e.value), str(e.value)
    assert (o[1] == 0xEE).all(), "the field whose buffer is too small was written"
    # ... and exactly enough is enough
    o = outs()
    recs, _ = ctx.encode_host_seg_batch_masked(fields, list(TOLS), BELOW, seg=seg, outs=[x[:c] for x, c in zip(o, caps)], **fmt)
    for got, w in zip(recs, want):
        same_record(got, w)


def damaged(rec, n, und_count):
    """{name: the record with its blob damaged}"""
    nt = rec["ntot_enc"]
    planes, blob = rec["data"][:nt], rec["data"][nt:].copy()

    def head(n_, count_, magic=b"WRM1"):
        return np.frombuffer(magic + struct.pack("<IQQ", 0, n_, count_) + bytes(blob[24:32]), dtype=np.uint8)

    seg, nseg = struct.unpack("<II", bytes(blob[36:44]))
    flipped = blob.copy()
    flipped[32 + 12 + 4 * nseg + 2] ^= 0x40
    bits = api.mask_parse_host_ref(blob, n)[0].astype(bool)
    assert n % 8
    beyond = np.packbits(bits, bitorder="little")
    last = int(np.flatnonzero(bits)[-1])
    beyond[last >> 3] = int(beyond[last >> 3]) & (0xFF ^ (1 << (last & 7)))
    beyond[-1] |= 0x80  # (the population count stays the header's)
    out = {
        "truncated": blob[:-1],
        "magic": np.concatenate([head(n, und_count, b"WRM2"), blob[32:]]),
        "flipped": flipped,
        "beyond n": np.concatenate([head(n, und_count), api.seg_encode_host_ref(beyond, seg)]),
        "count": np.concatenate([head(n, und_count + 1), blob[32:]]),
    }
    return {k: dict(rec, data=np.concatenate([planes, v])) for k, v in out.items()}


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_damaged_blob_is_refused_and_no_field_is_written(ctx, dtype):
    shape = (33, 17, 9)
    nx, ny, nz = shape
    recs = decode_mix(ctx, shape, dtype)
    batch = ctx.decode_host_seg_batch_masked if dtype is np.float64 else ctx.decode_host_seg_batch_masked_f32
    at = 6  # a masked record behind constants and plain records: those would be written first
    bad = damaged(recs[at], nx * ny * nz, recs[at]["mask"]["undefined"])
    assert sorted(bad) == ["beyond n", "count", "flipped", "magic", "truncated"]
    for name, rec in bad.items():
        outs = [np.full((nz, ny, nx), SENTINEL, dtype) for _ in recs]
        with pytest.raises(api.WaveRangeError) as e:
            batch(outs, recs[:at] + [rec] + recs[at + 1:], np.nan)
        assert "error -4" in str(e.value) and "field %d: " % at in str(e.value), (name, str(e.value))
        assert all((o == SENTINEL).all() for o in outs), name
        if dtype is np.float64:
            bufs = [ctx.to_device(np.full((nz, ny, nx), SENTINEL)) for _ in recs]
            try:
                with pytest.raises(api.WaveRangeError) as e:
                    ctx.decode_seg_batch_masked(bufs, (nz, ny, nx), recs[:at] + [rec] + recs[at + 1:], np.nan)
                assert "error -4" in str(e.value) and "field %d: " % at in str(e.value), (name, str(e.value))
                assert all((b.download(np.float64, nx * ny * nz) == SENTINEL).all() for b in bufs), name
            finally:
                for b in bufs:
                    b.free()
