"""Parity of the HIP path (through the C ABI) with the CPU oracle, bit for bit.
Run on the GPU box: python -m pytest tests -m gpu"""
import numpy as np
import pytest

from util import bits_equal, check_enc_record, sha
from waverange_amd import synth

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64, 64), (13, 9, 7), (37, 21, 13), (33, 5, 1), (2, 2, 2), (3, 3, 3), (17, 1, 1),
          (9, 1, 40), (1, 4, 1), (100, 3, 2), (130, 70, 34), (256, 8, 4), (1030, 6, 5), (257, 129, 65),
          # multiples of 16 and >= 64: the fused single-pass-per-level kernels
          (128, 64, 80), (96, 64, 64), (64, 128, 64), (272, 96, 64), (64, 64, 144),
          # even at the finest levels only: fused levels on top, general kernels for the coarse rest
          (200, 120, 72), (136, 88, 40), (260, 132, 68), (72, 200, 104)]


@pytest.fixture(scope="module")
def api():
    from waverange_amd import api as a
    a.set_verbosity(0)
    return a


@pytest.fixture(scope="module")
def ctx(api):
    c = api.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("shape", SHAPES)
def test_transform_bit_exact(ctx, oracle, shape):
    nx, ny, nz = shape
    f = synth.field(nx, ny, nz, seed=nx * 131 + ny)
    buf = ctx.to_device(f)
    for lvl in (4, 1, 2):
        buf.upload(f)
        ctx.transform(buf, f.shape, lvl)
        ctx.sync()
        fw = buf.download(np.float64, f.size)
        want = oracle.cdf97_3d(f, lvl)
        assert bits_equal(fw, want), ("fwd", shape, lvl)
        ctx.transform(buf, f.shape, -lvl)
        ctx.sync()
        assert bits_equal(buf.download(np.float64, f.size), oracle.cdf97_3d(want, -lvl)), ("inv", shape, lvl)
    buf.free()


def test_transform_golden(ctx, golden):
    for name in ("64x64x64", "37x21x13", "5x1x33", "2x3x1", "130x70x34"):
        nx, ny, nz = (int(v) for v in name.split("x"))
        g = golden["G2"][name]
        f = synth.field(nx, ny, nz, seed=g["seed"])
        buf = ctx.to_device(f)
        ctx.transform(buf, f.shape, 4)
        ctx.sync()
        assert sha(buf.download(np.float64, f.size)) == g["fwd_sha256"], name
        ctx.transform(buf, f.shape, -4)
        ctx.sync()
        assert sha(buf.download(np.float64, f.size)) == g["inv_sha256"], name
        buf.free()


def test_synth_field_device_matches_numpy(ctx):
    for (nx, ny, nz, seed) in ((64, 64, 64, 12345), (37, 21, 13, 7), (128, 32, 16, 99)):
        buf = ctx.alloc(nx * ny * nz * 8)
        ctx.synth_field(buf, nx, ny, nz, seed)
        ctx.sync()
        assert bits_equal(buf.download(np.float64, nx * ny * nz), synth.field(nx, ny, nz, seed=seed))
        buf.free()


def test_minmax_and_zero_sign(ctx, oracle):
    rs = np.random.RandomState(0)
    for n in (1, 2, 3, 1000, 65537, 1 << 20):
        x = rs.standard_normal(n)
        buf = ctx.to_device(x)
        assert ctx.minmax(buf, n) == oracle.minmax(x)
        buf.free()
    # minimum is a zero: the sign of the LAST zero in memory order wins (reference fmin scan)
    for zeros in ([0.0, -0.0], [-0.0, 0.0], [-0.0, 0.0, -0.0]):
        x = np.abs(rs.standard_normal(5000)) + 1.0
        pos = sorted(rs.choice(5000, len(zeros), replace=False))
        for p, z in zip(pos, zeros):
            x[p] = z
        buf = ctx.to_device(x)
        mn, mx = ctx.minmax(buf, x.size)
        omn, omx = oracle.minmax(x)
        assert mn == 0 and np.signbit(mn) == np.signbit(omn) and mx == omx
        buf.free()
    # NaNs are skipped, as the reference's fmin/fmax do
    x = rs.standard_normal(1000)
    x[::17] = np.nan
    buf = ctx.to_device(x)
    assert ctx.minmax(buf, x.size) == oracle.minmax(x)
    buf.free()


@pytest.mark.parametrize("n", [1, 2, 7, 4096, 100003])
def test_quantize_plane_bit_exact(ctx, oracle, n):
    rs = np.random.RandomState(n)
    x = rs.standard_normal(n) * 3.0
    lo, hi = oracle.minmax(x)
    deps = (hi - lo) / 255.0 if n > 1 else 0.5
    q_want, r_want = oracle.quantize_plane(x, deps, lo)
    buf = ctx.to_device(x)
    qbuf = ctx.alloc(n + 16)
    nlo, nhi = ctx.quantize_plane(buf, n, deps, lo, qbuf)
    assert np.array_equal(qbuf.download(np.uint8, n), q_want)
    assert bits_equal(buf.download(np.float64, n), r_want)
    assert (nlo, nhi) == oracle.minmax(r_want)
    buf.free()
    qbuf.free()


def test_dequant_accum_bit_exact(ctx, oracle):
    rs = np.random.RandomState(2)
    for n in (1, 5, 4096, 100003):
        for nlay in (1, 3, 8):
            planes = [rs.randint(0, 256, n).astype(np.uint8) for _ in range(nlay)]
            deps = [10.0 ** (-2 * i) * 0.37 for i in range(nlay)]
            mins = [-(10.0 ** (-2 * i)) * 1.1 for i in range(nlay)]
            want = np.zeros(n)
            for q, d, m in zip(planes, deps, mins):
                want = oracle.dequant_accum(want, q, d, m)
            bufs = [ctx.to_device(q) for q in planes]
            acc = ctx.alloc(n * 8)
            ctx.dequant_accum(acc, n, bufs, deps, mins)
            ctx.sync()
            assert bits_equal(acc.download(np.float64, n), want)
            for b in bufs + [acc]:
                b.free()


def _device_encode(ctx, f, tol, wtflag=1):
    buf = ctx.to_device(f)
    ctx.set_keep_residual(True)
    enc, tm = ctx.encode(buf, f.shape, tol, wtflag=wtflag)
    resid = buf.download(np.float64, f.size)
    enc["data"] = enc["data"].copy()
    dec_buf = ctx.alloc(f.nbytes)
    ctx.decode(dec_buf, f.shape, enc)
    rec = dec_buf.download(np.float64, f.size).reshape(f.shape)
    buf.free()
    dec_buf.free()
    ctx.set_keep_residual(False)
    return enc, resid, rec


@pytest.mark.parametrize("tol", ["1e-3", "1e-5", "1e-7", "1e-16"])
def test_codec_golden_64(ctx, golden, tol):
    """Config 1 shape (64^3 fp64): every output of encoding_wrap, the coded bytes, the
    residual left in the field and the reconstruction equal the reference's."""
    f = synth.field(64, 64, 64, seed=12345)
    enc, resid, rec = _device_encode(ctx, f, float(tol))
    g = golden["G1"][tol]
    check_enc_record(enc, g, tol)
    assert sha(resid) == g["residual_sha256"]
    assert sha(rec) == g["decoded_sha256"]
    s = enc["data"]
    off = 0
    for ln in enc["len_enc_vec"]:   # structural anchors: first byte 0, 24-bit length trailer
        assert s[off] == 0
        assert (int(s[off + ln - 3]) << 16 | int(s[off + ln - 2]) << 8 | int(s[off + ln - 1])) == ln % (1 << 24)
        off += ln


@pytest.mark.parametrize("shape,tol,wtflag", [((37, 21, 13), 1e-6, 1), ((64, 64, 8), 1e-4, 0),
                                              ((60, 50, 40), 1e-10, 1), ((5, 1, 33), 1e-3, 1),
                                              ((128, 128, 128), 1e-5, 1), ((2, 1, 1), 1e-3, 1),
                                              ((200, 120, 72), 1e-6, 1), ((260, 132, 68), 1e-4, 1)])
def test_codec_vs_oracle(ctx, oracle, shape, tol, wtflag):
    nx, ny, nz = shape
    f = synth.field(nx, ny, nz, seed=4242)
    enc, resid, rec = _device_encode(ctx, f, tol, wtflag)
    want = oracle.encode(f, tol, wtflag=wtflag)
    for k in ("tolabs", "midval", "halfspanval", "wlev", "nlay", "ntot_enc", "len_enc_vec"):
        assert enc[k] == want[k], k
    assert bits_equal(enc["deps_vec"], want["deps_vec"]) and bits_equal(enc["minval_vec"], want["minval_vec"])
    assert np.array_equal(enc["data"], want["data"])
    assert bits_equal(resid, want["residual"])
    assert bits_equal(rec, oracle.decode(want, f.shape))


def test_trivial_field(ctx, golden):
    g = golden["G4"]
    f = np.full((4, 5, 6), g["value"])
    enc, _, rec = _device_encode(ctx, f, 1e-6)
    assert (enc["ntot_enc"], enc["nlay"], enc["wlev"]) == (g["ntot_enc"], g["nlay"], g["wlev"])
    assert float(enc["midval"]).hex() == g["midval"] and float(enc["halfspanval"]).hex() == g["halfspanval"]
    assert np.array_equal(rec, f)


def test_device_only_planes(ctx, api, oracle):
    """wr_dev_encode_planes / wr_dev_decode_planes (no range coder): planes equal the
    oracle's quantized planes, reconstruction equals the oracle's."""
    f = synth.field(48, 40, 24, seed=3)
    n = f.size
    want = oracle.encode(f, 1e-6)
    pitch = api.lib().wr_plane_pitch(n)
    buf = ctx.to_device(f)
    planes = ctx.alloc(pitch * 8)
    info = ctx.encode_planes(buf, f.shape, 1e-6, planes)
    assert info.nlay == want["nlay"]
    off = 0
    for l in range(info.nlay):
        q = planes.download(np.uint8, n, offset=l * pitch)
        stream = want["data"][off:off + want["len_enc_vec"][l]]
        off += want["len_enc_vec"][l]
        back, got = oracle.range_decode(stream, n)
        assert got == n and np.array_equal(q, back), l
    out = ctx.alloc(f.nbytes)
    ctx.decode_planes(out, f.shape, planes, info)
    assert bits_equal(out.download(np.float64, n), oracle.decode(want, f.shape))
    for b in (buf, planes, out):
        b.free()


def test_host_pointer_drop_in_api(api, golden):
    """encoding_wrap / decoding_wrap with host buffers (the libwaverange drop-in symbols)."""
    f = synth.field(64, 64, 64, seed=12345)
    enc = api.encoding_wrap(f, 1e-7)
    g = golden["G1"]["1e-7"]
    check_enc_record(enc, g)
    assert sha(api.decoding_wrap(enc, f.shape)) == g["decoded_sha256"]
    g2 = golden["G2"]["64x64x64"]
    assert sha(api.waveletcdf97_3d(f, 4)) == g2["fwd_sha256"]


def test_large_roundtrip_properties(ctx, oracle):
    """256^3 against the oracle bit for bit; 512^3 (config 2: tol 1e-5) through size-independent
    properties: stream anchors, decode(encode(f)) within the tolerance band the reference
    itself achieves, and transform round trip at round-off level."""
    f = synth.field(256, 256, 256, seed=12345)
    buf = ctx.to_device(f)
    enc, _ = ctx.encode(buf, f.shape, 1e-5)
    enc["data"] = enc["data"].copy()
    want = oracle.encode(f, 1e-5)
    assert np.array_equal(enc["data"], want["data"]) and enc["len_enc_vec"] == want["len_enc_vec"]
    ctx.decode(buf, f.shape, enc)
    assert bits_equal(buf.download(np.float64, f.size), oracle.decode(want, f.shape))
    buf.free()

    n = 512
    buf = ctx.alloc(n ** 3 * 8)
    ctx.synth_field(buf, n, n, n, 12345)
    ctx.sync()
    orig = buf.download(np.float64, n ** 3)
    ctx.transform(buf, (n, n, n), 4)
    ctx.transform(buf, (n, n, n), -4)
    ctx.sync()
    back = buf.download(np.float64, n ** 3)
    assert np.abs(back - orig).max() < 1e-12 * np.abs(orig).max()
    buf.upload(orig)
    enc, tm = ctx.encode(buf, (n, n, n), 1e-5)
    assert 1 <= enc["nlay"] <= 8 and sum(enc["len_enc_vec"]) == enc["ntot_enc"]
    # config 2 (512^3, tol 1e-5) against the oracle: header scalars and every coded byte
    want = oracle.encode(orig.reshape(n, n, n), 1e-5)
    assert enc["len_enc_vec"] == want["len_enc_vec"] and enc["tolabs"] == want["tolabs"]
    assert bits_equal(enc["deps_vec"], want["deps_vec"]) and bits_equal(enc["minval_vec"], want["minval_vec"])
    assert np.array_equal(enc["data"], want["data"])
    del want
    off = 0
    for ln in enc["len_enc_vec"]:
        assert enc["data"][off] == 0
        off += ln
    ctx.decode(buf, (n, n, n), enc)
    rec = buf.download(np.float64, n ** 3)
    linf = np.abs(rec - orig).max() / np.abs(orig).max()
    assert linf < 1.05e-5, linf     # the reference itself may exceed tol by ~1 %
    buf.free()


@pytest.mark.parametrize("shape,m", [((32, 16, 8), (2, 2, 2)), ((64, 64, 64), (4, 2, 1)), ((37, 21, 13), (3, 2, 2))])
def test_local_cutoff_branch(ctx, oracle, shape, m):
    """mx*my*mz > 1: the reference's non-uniform cutoff (wrappers.cpp:343-379) on the GPU."""
    nx, ny, nz = shape
    f = synth.field(nx, ny, nz, seed=77)
    rs = np.random.RandomState(3)
    cut = 10.0 ** rs.uniform(-6, -2, size=m[0] * m[1] * m[2])
    want = oracle.encode(f, None, cutoff=list(cut), m=m)
    buf = ctx.to_device(f)
    enc, _ = ctx.encode_local(buf, f.shape, cut, m)
    for k in ("tolabs", "midval", "halfspanval", "wlev", "nlay", "ntot_enc", "len_enc_vec"):
        assert enc[k] == want[k], k
    assert bits_equal(enc["deps_vec"], want["deps_vec"]) and bits_equal(enc["minval_vec"], want["minval_vec"])
    assert np.array_equal(enc["data"], want["data"])
    ctx.decode(buf, f.shape, enc)
    assert bits_equal(buf.download(np.float64, f.size), oracle.decode(want, f.shape))
    buf.free()


def test_full_size_1024_fused_vs_general_and_roundtrip(ctx, api):
    """BASELINE full size (1024^3 fp64, 8 GiB): the two device implementations against each other (the coded
    bytes against the oracle at this size: test_gpu_host_api.py::test_full_size_1024_coded_bytes_vs_oracle).
    (1) the fused single-pass kernels and the general 3-pass kernels -- two independent device
        implementations, each pinned to the oracle at small sizes -- must agree bit for bit,
        forward and inverse (compared on the device, max|a-b| == 0);
    (2) encode -> decode at tol 1e-3 reconstructs within the tolerance band, the plane streams
        carry the format anchors and their lengths add up."""
    import os
    n = 1024
    shape = (n, n, n)
    a = ctx.alloc(n ** 3 * 8)
    b = ctx.alloc(n ** 3 * 8)
    ctx.synth_field(a, n, n, n, 12345)
    ctx.copy(b, a, n ** 3 * 8)
    ctx.transform(a, shape, 4)                 # fused
    os.environ["WR_NO_FUSED"] = "1"
    try:
        ctx.transform(b, shape, 4)             # general
        diff, amax = ctx.linf(a, b, n ** 3)
        assert diff == 0.0 and amax > 0
        ctx.transform(b, shape, -4)            # general inverse
    finally:
        del os.environ["WR_NO_FUSED"]
    ctx.transform(a, shape, -4)                # fused inverse
    diff, _ = ctx.linf(a, b, n ** 3)
    assert diff == 0.0
    ctx.synth_field(b, n, n, n, 12345)
    diff, amax = ctx.linf(b, a, n ** 3)        # forward + inverse is the identity up to round-off
    assert diff < 1e-12 * amax
    enc, tm = ctx.encode(a, shape, 1e-3)
    assert 1 <= enc["nlay"] <= 8 and sum(enc["len_enc_vec"]) == enc["ntot_enc"]
    off = 0
    for ln in enc["len_enc_vec"]:
        s = enc["data"]
        assert s[off] == 0
        assert (int(s[off + ln - 3]) << 16 | int(s[off + ln - 2]) << 8 | int(s[off + ln - 1])) == ln % (1 << 24)
        off += ln
    ctx.decode(a, shape, enc)
    diff, amax = ctx.linf(b, a, n ** 3)
    # The reference's own error control is approximate (1.013e-3 at 256^3 for tol
    # 1e-3; WAV_ACC_COEF = 1.75 is an empirical allowance for the 4-level synthesis gain).  At
    # 1024^3 the same arithmetic gives 1.09e-3 -- the reference's own figure: the coded bytes at this
    # size equal the oracle's (tests/test_gpu_host_api.py::test_full_size_1024_coded_bytes_vs_oracle).
    assert diff / amax < 1.1e-3
    a.free()
    b.free()


def test_api_error_paths(ctx, api):
    """Part-2 functions return error codes (never crash, never fall back): too small an output buffer,
    a corrupted / truncated stream, bad arguments."""
    import ctypes as C
    f = synth.field(32, 32, 32, seed=1)
    buf = ctx.to_device(f)
    enc, _ = ctx.encode(buf, f.shape, 1e-6)
    enc["data"] = enc["data"].copy()
    # output capacity too small -> WR_ERR_OVERFLOW (the reference throws here, wrappers.cpp:422-426)
    buf.upload(f)
    small = np.empty(enc["ntot_enc"] // 2, dtype=np.uint8)
    with pytest.raises(api.WaveRangeError, match="encoded array is too large"):
        ctx.encode(buf, f.shape, 1e-6, out=small)
    # truncated last plane (header and buffer agree on the shorter length): the plane does not decode
    # to nx*ny*nz symbols -> WR_ERR_STREAM.  (A buffer shorter than ntot_enc says would be a caller bug
    # the library cannot see.)
    bad = dict(enc)
    bad["len_enc_vec"] = list(enc["len_enc_vec"])
    bad["len_enc_vec"][-1] //= 2
    bad["ntot_enc"] = sum(bad["len_enc_vec"])
    bad["data"] = enc["data"][: bad["ntot_enc"]].copy()
    with pytest.raises(api.WaveRangeError):
        ctx.decode(buf, f.shape, bad)
    # corrupted bytes in the middle of a plane: must not crash; either an error or a wrong field
    bad = dict(enc)
    d = enc["data"].copy()
    d[len(d) // 3: len(d) // 3 + 64] ^= 0x5A
    bad["data"] = d
    try:
        ctx.decode(buf, f.shape, bad)
    except api.WaveRangeError:
        pass
    # nlay out of range, misaligned device pointer
    bad = dict(enc)
    bad["nlay"] = 9
    with pytest.raises(Exception):
        ctx.decode(buf, f.shape, bad)
    info, tm = api.EncInfo(), api.Timings()
    rc = api.lib().wr_encode_device(ctx.h, buf.ptr + 8, 32, 32, 32, 1, 1e-6, C.byref(info), small.ctypes.data, small.size, C.byref(tm))
    assert rc != 0 and b"aligned" in api.lib().wr_last_error()
    # after all these failures the context still works
    buf.upload(f)
    again, _ = ctx.encode(buf, f.shape, 1e-6)
    assert np.array_equal(again["data"], enc["data"])
    buf.free()


def test_concurrent_contexts_are_bit_exact(api, oracle):
    """Several contexts on one GPU driven from concurrent host threads (what bench.py and the FluSI
    front-end do): device phases serialise inside the library, host coding overlaps; every stream
    and reconstruction must still equal the oracle's."""
    import threading
    jobs = [((64, 64, 64), 1e-7, 12345), ((96, 64, 64), 1e-4, 7), ((37, 21, 13), 1e-6, 9), ((128, 64, 80), 1e-5, 3)]
    want = {}
    for shape, tol, seed in jobs:
        f = synth.field(*shape, seed=seed)
        e = oracle.encode(f, tol)
        want[(shape, tol, seed)] = (f, e, oracle.decode(e, f.shape))
    errors = []

    def worker(job):
        try:
            f, e, rec = want[job]
            with api.Context(0) as c:
                for _ in range(3):
                    buf = c.to_device(f)
                    enc, _ = c.encode(buf, f.shape, job[1])
                    assert np.array_equal(enc["data"], e["data"]) and enc["len_enc_vec"] == e["len_enc_vec"]
                    enc["data"] = enc["data"].copy()
                    c.decode(buf, f.shape, enc)
                    assert bits_equal(buf.download(np.float64, f.size), rec)
                    buf.free()
        except Exception as exc:  # noqa: BLE001
            errors.append((job, exc))

    ths = [threading.Thread(target=worker, args=(j,)) for j in jobs]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errors, errors


@pytest.mark.parametrize("threads,tol", [(1, 1e-7), (2, 1e-7), (3, 1e-7), (1, 1e-16), (3, 1e-16)])
def test_grouped_coder_threads_same_bytes(ctx, api, oracle, threads, tol):
    """wr_set_threads(k) with k < nlay: the planes are coded in k groups with their symbol loops
    interleaved (wr_rangecoder.cpp encode_planes / decode_planes).  Streams and reconstruction must
    not depend on the grouping.  200x190x180 gives > 100 coding blocks per plane, so the unchecked
    interleaved loops and the padded-tail path both run; tol 1e-16 gives 8 planes (groups larger than
    one loop interleaves are split)."""
    f = synth.field(180, 190, 200, seed=21)
    e = oracle.encode(f, tol)
    assert e["nlay"] >= (8 if tol < 1e-12 else 3)
    rec = oracle.decode(e, f.shape)
    api.set_threads(threads)
    try:
        buf = ctx.to_device(f)
        enc, _ = ctx.encode(buf, f.shape, tol)
        assert enc["len_enc_vec"] == e["len_enc_vec"] and np.array_equal(enc["data"], e["data"])
        enc["data"] = enc["data"].copy()
        ctx.decode(buf, f.shape, enc)
        assert bits_equal(buf.download(np.float64, f.size), rec)
        buf.free()
    finally:
        api.set_threads(8)


def test_random_shapes_tolerances_and_field_kinds_vs_oracle(ctx, oracle):
    """Seeded sweep over odd / thin / prime shapes, tolerances from 1e-2 to 1e-14 and several kinds of
    field (smooth, noisy, piecewise constant, huge offset, tiny amplitude): coded bytes, header scalars
    and reconstruction against the oracle."""
    rs = np.random.RandomState(20261003)
    for case in range(24):
        nx, ny, nz = (int(rs.choice([1, 2, 3, 5, 8, 13, 16, 17, 31, 32, 33, 48, 64, 70])) for _ in range(3))
        tol = float(10.0 ** -rs.randint(2, 15))
        kind = case % 5
        f = synth.field(nx, ny, nz, seed=1000 + case)
        if kind == 1:
            f = f + rs.standard_normal(f.shape) * 1e-3
        elif kind == 2:
            f = np.floor(f * 4.0) / 4.0
        elif kind == 3:
            f = f + 1.0e6
        elif kind == 4:
            f = f * 1.0e-12
        f = np.ascontiguousarray(f, dtype=np.float64)
        want = oracle.encode(f, tol)
        buf = ctx.to_device(f)
        enc, _ = ctx.encode(buf, f.shape, tol)
        tag = "case %d shape %s tol %g kind %d" % (case, (nx, ny, nz), tol, kind)
        for k in ("tolabs", "midval", "halfspanval", "wlev", "nlay", "ntot_enc", "len_enc_vec"):
            assert enc[k] == want[k], (tag, k)
        assert np.array_equal(enc["data"], want["data"]), tag
        enc["data"] = enc["data"].copy()
        ctx.decode(buf, f.shape, enc)
        assert bits_equal(buf.download(np.float64, f.size), oracle.decode(want, f.shape)), tag
        buf.free()


@pytest.mark.parametrize("shape", [(64, 64, 64), (128, 64, 80), (200, 120, 72)])
def test_zero_minimum_and_nans_on_the_fused_minmax_path(ctx, oracle, shape):
    """All four levels fused: min/max of the field and of the coefficients come out of the forward kernels.  The
    reference's scan semantics must survive that: the sign of a zero minimum is the sign of the LAST zero in
    memory order (it shows in midval / minval_vec).  (No NaN sample here: it would spread through the transform into
    a float-to-byte cast that the reference leaves undefined, so nothing could be pinned; min/max alone skip NaNs
    as fmin / fmax do, test_minmax_and_zero_sign.)"""
    nx, ny, nz = shape
    rs = np.random.RandomState(nx)
    f = np.abs(synth.field(nx, ny, nz, seed=8)) + 0.25
    flat = f.reshape(-1)
    pos = np.sort(rs.choice(flat.size, 3, replace=False))
    for zeros in ([0.0, -0.0, 0.0], [-0.0, 0.0, -0.0]):
        flat[pos] = zeros
        want = oracle.encode(f, 1e-6)
        buf = ctx.to_device(f)
        enc, _ = ctx.encode(buf, f.shape, 1e-6)
        buf.free()
        assert float(enc["midval"]).hex() == float(want["midval"]).hex()
        assert bits_equal(enc["minval_vec"], want["minval_vec"]) and bits_equal(enc["deps_vec"], want["deps_vec"])
        assert np.array_equal(enc["data"], want["data"])
    # a field that is zero almost everywhere: the coefficient minimum of later planes is a zero as well
    g = np.zeros_like(f)
    g.reshape(-1)[pos] = [1.0, -0.0, 2.0]
    want = oracle.encode(g, 1e-4)
    buf = ctx.to_device(g)
    enc, _ = ctx.encode(buf, g.shape, 1e-4)
    buf.free()
    assert enc["nlay"] == want["nlay"] and bits_equal(enc["minval_vec"], want["minval_vec"])
    assert np.array_equal(enc["data"], want["data"])


def test_fortran_example_field(ctx, golden):
    """G7: the reference's Fortran example (examples/fortran/example_fort.f90:82-120: 64^3 field 10 sin x sin^2 y cos z, tolrel
    1e-6, encode + decode, relative L-inf error) on the GPU path: every output equals the compiled reference's."""
    from util import g7_field
    rec = golden["G7_fortran_example_64"]
    f = g7_field(rec)
    buf = ctx.to_device(f)
    enc, _ = ctx.encode(buf, f.shape, rec["tolrel"])
    enc["data"] = enc["data"].copy()
    check_enc_record(enc, rec, "G7")
    ctx.decode(buf, f.shape, enc)
    dec = buf.download(np.float64, f.size).reshape(f.shape)
    buf.free()
    assert sha(dec) == rec["decoded_sha256"]
    assert np.abs(dec - f).max() / np.abs(f).max() == rec["linf_rel"] < rec["tolrel"]


QUANT_PATH_WORKER = r'''
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import numpy as np
from util import bits_equal
from waverange_amd import api, synth
from oracle.loader import Oracle
api.set_verbosity(0)
o = Oracle()
with api.Context(0) as c:
    for shape, tol in (((130, 70, 34), 1e-10), ((128, 64, 80), 1e-16), ((200, 120, 72), 1e-6), ((37, 21, 13), 1e-9), ((61, 1, 1), 1e-7),
                       ((128, 128, 256), 1e-6), ((64, 64, 144), 1e-4),
                       # whole numbers of 60000-symbol coding blocks (an empty final block), and a plane shorter than one 16-byte piece
                       ((100, 60, 10), 1e-8), ((200, 60, 10), 1e-5), ((3, 2, 2), 1e-9)):
        f = synth.field(*shape, seed=99)
        want = o.encode(f, tol)
        rec_want = o.decode(want, f.shape)
        for keep in (True, False):
            buf = c.to_device(f)
            c.set_keep_residual(keep)
            enc, _ = c.encode(buf, f.shape, tol)
            assert enc["nlay"] == want["nlay"] and list(enc["len_enc_vec"]) == list(want["len_enc_vec"]), (shape, tol)
            assert bits_equal(enc["deps_vec"], want["deps_vec"]) and bits_equal(enc["minval_vec"], want["minval_vec"]), (shape, tol)
            assert np.array_equal(enc["data"], want["data"]), (shape, tol, "coded bytes")
            if keep:
                assert bits_equal(buf.download(np.float64, f.size), want["residual"]), (shape, tol, "residual")
            buf.free()
        # host entry point (block histograms from the quantizer, planes through the windows)
        enc, _ = c.encode_host(f, tol)
        assert np.array_equal(enc["data"], want["data"]), (shape, tol, "host entry point")
        # and back
        out = np.empty_like(f); enc["data"] = enc["data"].copy()
        c.decode_host(out, enc)
        assert bits_equal(out, rec_want), (shape, tol, "reconstruction")
print("ok")
'''


@pytest.mark.parametrize("env", [{}, {"WR_TEST_ZERO_MIN_PATH": "1"}, {"WR_QUANT_INPLACE": "1"}, {"WR_PLANE_CHUNK_MB": "1"}],
                         ids=["recompute", "rare_path_after_every_plane", "in_place", "chunked_planes"])
def test_quantizer_without_a_residual_array(env, tmp_path):
    """The quantizer planes are cut from residuals that are recomputed from the coefficient array (k_quant_blk: 9 instead of
    17 bytes per element and plane), with the block histograms written on the way; the reference updates the array in place
    after every plane (wrappers.cpp:397-398).  Same header scalars, coded bytes and final residual as the oracle -- for up to
    eight planes, odd sizes (tails of coding blocks and of 16-byte pieces), planes in 1 MiB chunks (blocks that straddle
    two), with the residual wanted and not; when the rare path that needs the residual in memory between two planes is taken
    after EVERY plane (sign of a zero minimum: residual_apply, then in place); and with the in-place kernels alone.
    The way back likewise (planes as one array and in chunks): reconstruction == oracle."""
    import os, subprocess, sys
    from util import ROOT
    script = tmp_path / "quant_paths.py"
    script.write_text(QUANT_PATH_WORKER % dict(root=ROOT))
    r = subprocess.run([sys.executable, str(script)], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
