"""Host-buffer entry points (wr_encode_host / wr_decode_host, what the drop-in encoding_wrap / decoding_wrap run
on) against the oracle; the work-space slots; plane-ordered upload under the range decoder; dimensions beyond
the launch-grid limits; and NF=8 x 512^3 sharded (BASELINE configs[3]): container against the oracle-coded container
(configs[2], 1024^3, lives in tests/test_golden_large.py: against the reference's own outputs).
Run on the GPU box: python -m pytest tests -m gpu"""
import os
import shutil
import subprocess
import sys
import threading

import numpy as np
import pytest

from util import ROOT, bits_equal, sha
from waverange_amd import synth

pytestmark = pytest.mark.gpu


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


def same_as_oracle(enc, want):
    for k in ("tolabs", "midval", "halfspanval", "wlev", "nlay", "ntot_enc", "len_enc_vec"):
        assert enc[k] == want[k], k
    assert bits_equal(enc["deps_vec"], want["deps_vec"]) and bits_equal(enc["minval_vec"], want["minval_vec"])
    assert np.array_equal(enc["data"], want["data"])


@pytest.mark.parametrize("pinned", [True, False])
@pytest.mark.parametrize("shape,tol,wtflag", [((64, 64, 64), 1e-7, 1), ((37, 21, 13), 1e-6, 1), ((128, 64, 80), 1e-4, 1),
                                              ((64, 64, 8), 1e-4, 0), ((200, 120, 72), 1e-10, 1),
                                              ((400, 300, 272), 1e-6, 1)])  # the last: planes of 2 windows + a partial one
def test_host_entry_points_vs_oracle(ctx, api, oracle, pinned, shape, tol, wtflag):
    nx, ny, nz = shape
    f = synth.field(nx, ny, nz, seed=99)
    want = oracle.encode(f, tol, wtflag=wtflag)
    src = api.pinned_array(f.shape) if pinned else np.empty_like(f)
    src[...] = f
    enc, tm = ctx.encode_host(src, tol, wtflag=wtflag)
    same_as_oracle(enc, want)
    assert bits_equal(src, f), "the field must stay untouched without keep_residual"
    enc["data"] = enc["data"].copy()
    out = api.pinned_array(f.shape) if pinned else np.empty_like(f)
    out[...] = -1.0
    ctx.decode_host(out, enc)
    assert bits_equal(out, oracle.decode(want, f.shape))
    # the reference's side effect on request: the residual in the caller's array (wrappers.cpp:397-398)
    ctx.set_keep_residual(True)
    try:
        enc2, _ = ctx.encode_host(src, tol, wtflag=wtflag)
    finally:
        ctx.set_keep_residual(False)
    same_as_oracle(enc2, want)
    assert bits_equal(src, want["residual"])


def test_host_trivial_field_and_transform(ctx, api, oracle, golden):
    g = golden["G4"]
    f = np.full((4, 5, 6), g["value"])
    enc, _ = ctx.encode_host(f, 1e-6)
    assert (enc["ntot_enc"], enc["nlay"], enc["wlev"]) == (g["ntot_enc"], g["nlay"], g["wlev"])
    out = np.zeros_like(f)
    ctx.decode_host(out, enc)
    assert np.array_equal(out, f)
    for shape in ((64, 64, 64), (13, 9, 7), (96, 64, 64)):
        x = synth.field(*shape, seed=5)
        y = x.copy()
        ctx.transform_host(y, 4)
        want = oracle.cdf97_3d(x, 4)
        assert bits_equal(y, want)
        ctx.transform_host(y, -4)
        assert bits_equal(y, oracle.cdf97_3d(want, -4))


def test_plane_ordered_upload_under_the_decoder(ctx, api, oracle):
    """the decoded symbols go to the plane's device buffer window by window while the decoder is
    still at work on the rest (and on the other planes); the accumulate kernel consumes the planes in plane order.
    The counter proves that path ran; the reconstruction must equal the oracle's (the order of the sums matters,
    wrappers.cpp:513-514).  180 x 190 x 200 symbols are less than one 15 MB window; the full-size tests cover
    planes of 70 windows."""
    api.set_threads(8)
    f = synth.field(180, 190, 200, seed=21)
    for tol in (1e-7, 1e-16):
        want = oracle.encode(f, tol)
        assert want["nlay"] >= 3
        rec = oracle.decode(want, f.shape)
        before = api.stat(api.STAT_EARLY_DECODES)
        out = np.empty_like(f)
        ctx.decode_host(out, want)
        assert api.stat(api.STAT_EARLY_DECODES) == before + 1
        assert bits_equal(out, rec)
        buf = ctx.alloc(f.nbytes)
        ctx.decode(buf, f.shape, want)
        assert api.stat(api.STAT_EARLY_DECODES) == before + 2
        assert bits_equal(buf.download(np.float64, f.size), rec)
        buf.free()
    # grouped coder threads (planes interleaved in one loop): the same path, the same result
    api.set_threads(2)
    try:
        before = api.stat(api.STAT_EARLY_DECODES)
        out = np.empty_like(f)
        ctx.decode_host(out, want)
        assert api.stat(api.STAT_EARLY_DECODES) == before + 1
        assert bits_equal(out, rec)
    finally:
        api.set_threads(8)


@pytest.mark.parametrize("nslots", [1, 3])
def test_concurrent_host_calls_share_the_slots(api, oracle, nslots):
    """Six threads with their own contexts push fields of different shapes through wr_encode_host / wr_decode_host
    at the same time, with one and with three work-space slots on the device: every stream and reconstruction
    must equal the oracle's whatever the interleaving of the upload / kernel / download stages."""
    jobs = [((64, 64, 64), 1e-7, 1), ((96, 64, 64), 1e-4, 2), ((37, 21, 13), 1e-6, 3), ((128, 64, 80), 1e-5, 4),
            ((200, 120, 72), 1e-3, 5), ((64, 128, 64), 1e-9, 6)]
    want = {}
    for shape, tol, seed in jobs:
        f = synth.field(*shape, seed=seed)
        e = oracle.encode(f, tol)
        want[(shape, tol, seed)] = (f, e, oracle.decode(e, f.shape))
    # the slot count can only be lowered while the slots beyond it are empty: run the 1-slot case in a child process
    if nslots == 1:
        code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import pytest; "
                "sys.exit(pytest.main(['-q', '-x', '-m', 'gpu', %r + '::test_concurrent_host_calls_share_the_slots', '-k', '3']))"
                % (ROOT, os.path.join(ROOT, "tests"), os.path.abspath(__file__)))
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, WR_SLOTS="1", WR_TEST_EXPECT_SLOTS="1"),
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        return
    errors = []

    def worker(job):
        try:
            f, e, rec = want[job]
            with api.Context(0) as c:
                for _ in range(4):
                    enc, _ = c.encode_host(f, job[1])
                    assert np.array_equal(enc["data"], e["data"]) and enc["len_enc_vec"] == e["len_enc_vec"]
                    enc["data"] = enc["data"].copy()
                    out = np.empty_like(f)
                    c.decode_host(out, enc)
                    assert bits_equal(out, rec)
        except Exception as exc:  # noqa: BLE001
            errors.append((job, exc))

    ths = [threading.Thread(target=worker, args=(j,)) for j in jobs]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errors, errors
    expect = int(os.environ.get("WR_TEST_EXPECT_SLOTS", "0"))
    if expect:
        assert api.stat(api.STAT_SLOTS_POPULATED) == expect


@pytest.mark.parametrize("shape", [(4, 70000, 2), (2, 3, 66000), (12000, 3, 2), (16, 65600, 16), (6200, 2, 3), (10200, 3, 2), (10201, 2, 2)])
def test_dimensions_beyond_the_launch_grid_limits(ctx, oracle, shape):
    """ny or nz > 65535 (the limit of gridDim.y/z) and x lines longer than the LDS-staged kernel takes: the
    reference has no such limits (it loops), so the drop-in must not have them either.  Lines of 6200 and 10200 samples are
    staged whole in more than 48 KiB of dynamic LDS (the line kernel raises its limit for them), 10200 is the longest line it
    takes and 10201 the first that goes to the streaming pass; 12000 streams at level 0 and has a 6000-sample line below."""
    nx, ny, nz = shape
    f = synth.field(nx, ny, nz, seed=3)
    want = oracle.encode(f, 1e-5)
    enc, _ = ctx.encode_host(f, 1e-5)
    same_as_oracle(enc, want)
    enc["data"] = enc["data"].copy()
    out = np.empty_like(f)
    ctx.decode_host(out, enc)
    assert bits_equal(out, oracle.decode(want, f.shape))


# (BASELINE configs[2], the 1024^3 field at tol 1e-3 and 1e-7: tests/test_golden_large.py holds the product against what
# the reference itself produced at that size -- on per-call coder threads and on the pool / AVX-512 configuration the
# bench times -- instead of running the oracle on the GPU box for a minute.)


@pytest.mark.parametrize("n", [512, 256])
def test_config4_sharded_fields_container_vs_oracle(oracle, tmp_path, n):
    """BASELINE configs[3]: NF = 8 independent 512^3 fp64 fields (seeds 12345..12352) coded by the launchable sharded
    encoder -- python -m torch.distributed.run ... -m waverange_amd.sharded, two ranks here (both on this
    box's one GPU; on an 8-GPU node the same command runs with 8) -- and the .wrh / .wrb pair compared byte for
    byte with the container assembled from the oracle-coded fields (256^3) or with what the COMPILED REFERENCE produced for
    every one of the eight fields (512^3: tests/golden/large.json holds a pin per seed -- no minute of oracle on the GPU box).
    The 512^3 case IS config 4; it is skipped -- visibly, with the free space in the reason -- when the scratch disk cannot
    hold its 8.6 GB input; the 256^3 case always runs."""
    from waverange_amd import sharded
    nf = 8
    free = shutil.disk_usage(tmp_path).free
    if free < 1.5 * nf * n ** 3 * 8:
        pytest.skip("config 4 at %d^3 needs %.1f GB of scratch disk, %.1f GB are free" % (n, 1.5 * nf * n ** 3 * 8 / 1e9, free / 1e9))
    tol = 1e-5
    path = tmp_path / "data.bin"
    fields = []
    with open(path, "wb") as fh:
        for i in range(nf):
            f = synth.field(n, n, n, seed=12345 + i)
            f.tofile(fh)
            fields.append(f)
    specs = [dict(nbytes=8, nx=n, ny=n, nz=n, nh=1, idinv=0, icomp=1, tol_base=tol) for _ in range(nf)]
    encs = [None] * nf
    pins = None
    if n == 512:
        from util import large_golden
        g = large_golden()
        pins = [g["512^3_tol1e-05" + ("" if i == 0 else "_seed%d" % (12345 + i))] for i in range(nf)]
        for i in range(nf):
            assert sha(fields[i]) == pins[i]["input_sha256"]

    def cpu(i):
        e = oracle.encode(fields[i], tol)
        del e["residual"]
        encs[i] = e

    ths = [] if pins else [threading.Thread(target=cpu, args=(i,)) for i in range(nf)]
    for t in ths:
        t.start()
    env = dict(os.environ, WR_QUIET="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29533", "-m", "waverange_amd.sharded", str(path), str(tmp_path / "data.wrb"), str(tmp_path / "data.wrh"),
           "2", "0", str(nf), "2", str(n), str(n), str(n), repr(tol)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=str(tmp_path))
    for t in ths:
        t.join()
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    import hashlib
    if pins:
        # the header text from the reference's scalars (bit patterns), the payload of every field against the reference's hash
        fh = float.fromhex
        encs = [dict(tolabs=fh(p["tolabs"]), midval=fh(p["midval"]), halfspanval=fh(p["halfspanval"]), wlev=p["wlev"], nlay=p["nlay"], ntot_enc=p["ntot_enc"],
                     deps_vec=[fh(v) for v in p["deps_vec"]], minval_vec=[fh(v) for v in p["minval_vec"]], len_enc_vec=p["len_enc_vec"]) for p in pins]
        records = [dict(recl=bytes(8), enc=e, payload=b"") for e in encs]
        sharded.write_container(str(tmp_path / "want.wrh"), str(tmp_path / "want_empty.wrb"), "data.wrb", specs, 2, False, records)
        assert open(tmp_path / "data.wrh").read() == open(tmp_path / "want.wrh").read()
        assert os.path.getsize(tmp_path / "data.wrb") == sum(p["ntot_enc"] for p in pins)
        wrb = np.memmap(tmp_path / "data.wrb", dtype=np.uint8, mode="r")
        off = 0
        for i, p in enumerate(pins):
            assert hashlib.sha256(wrb[off:off + p["ntot_enc"]]).hexdigest() == p["data_sha256"], "coded bytes of field %d differ from the reference's" % i
            off += p["ntot_enc"]
        del wrb
        cmd = cmd[:cmd.index("waverange_amd.sharded") + 1] + [str(tmp_path / "data.wrb"), str(tmp_path / "data.wrh"), str(tmp_path / "datarec.bin"), "2", "0"]
        cmd[cmd.index("29533")] = "29534"
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        got = np.memmap(tmp_path / "datarec.bin", dtype=np.float64, mode="r")
        assert got.size == nf * n ** 3
        for i, p in enumerate(pins):
            assert sha(got[i * n ** 3:(i + 1) * n ** 3]) == p["decoded_sha256"], "reconstruction of field %d differs from the reference's" % i
        return
    records = [dict(recl=bytes(8), enc={k: e[k] for k in ("tolabs", "midval", "halfspanval", "wlev", "nlay", "ntot_enc", "deps_vec",
                                                            "minval_vec", "len_enc_vec")}, payload=e["data"].tobytes()) for e in encs]
    sharded.write_container(str(tmp_path / "want.wrh"), str(tmp_path / "want.wrb"), "data.wrb", specs, 2, False, records)
    assert open(tmp_path / "data.wrh").read() == open(tmp_path / "want.wrh").read()
    assert os.path.getsize(tmp_path / "data.wrb") == sum(e["ntot_enc"] for e in encs)

    def file_sha(p):
        h = hashlib.sha256()
        with open(p, "rb") as fh:
            for chunk in iter(lambda: fh.read(1 << 24), b""):
                h.update(chunk)
        return h.hexdigest()

    assert file_sha(tmp_path / "data.wrb") == file_sha(tmp_path / "want.wrb")

    # and back through the launcher's decoder mode (wrdec's five arguments): every rank writes its fields at their
    # offsets of one output file, which must hold the oracle's reconstructions bit for bit
    recs = [None] * nf

    def cpu_dec(i):
        recs[i] = oracle.decode(encs[i], fields[i].shape)

    ths = [threading.Thread(target=cpu_dec, args=(i,)) for i in range(nf)]
    for t in ths:
        t.start()
    cmd = cmd[:cmd.index("waverange_amd.sharded") + 1] + [str(tmp_path / "data.wrb"), str(tmp_path / "data.wrh"), str(tmp_path / "datarec.bin"), "2", "0"]
    cmd[cmd.index("29533")] = "29534"
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=str(tmp_path))
    for t in ths:
        t.join()
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    got = np.memmap(tmp_path / "datarec.bin", dtype=np.float64, mode="r")
    assert got.size == nf * n ** 3
    for i in range(nf):
        assert bits_equal(got[i * n ** 3:(i + 1) * n ** 3], recs[i]), i


def test_coder_pool_codes_all_fields_in_flight(api, oracle):
    """wr_set_coder_pool: the planes of all concurrent encode / decode calls go to a fixed set of worker threads that
    interleave streams of different fields (and send dominant-symbol planes through the 16-lane AVX-512 loop where
    the CPU has it).  Streams, header scalars and reconstructions must not change."""
    jobs = [((96, 96, 96), 1e-7, 1), ((128, 64, 80), 1e-3, 2), ((180, 190, 200), 1e-7, 3), ((64, 64, 64), 1e-16, 4),
            ((200, 120, 72), 1e-5, 5), ((37, 21, 13), 1e-6, 6)]
    want = {}
    for shape, tol, seed in jobs:
        f = synth.field(*shape, seed=seed)
        e = oracle.encode(f, tol)
        want[(shape, tol, seed)] = (f, e, oracle.decode(e, f.shape))
    api.set_coder_pool(4)
    errors = []

    def worker(job):
        try:
            f, e, rec = want[job]
            with api.Context(0) as c:
                for _ in range(3):
                    enc, _ = c.encode_host(f, job[1])
                    same_as_oracle(enc, e)
                    enc["data"] = enc["data"].copy()
                    out = np.empty_like(f)
                    c.decode_host(out, enc)
                    assert bits_equal(out, rec)
        except Exception as exc:  # noqa: BLE001
            errors.append((job, exc))

    try:
        ths = [threading.Thread(target=worker, args=(j,)) for j in jobs]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
    finally:
        api.set_coder_pool(0)
    assert not errors, errors


def test_decodes_wait_for_admission_without_their_planes(api, oracle):
    """A pooled decode whose kind's queues are long waits at the pool's admission gate BEFORE it prepares its planes (decode_impl:
    a third of the decoders' plane memory used to be held by planes that sat in the queues, and plane memory bounds the fields
    in flight): twelve concurrent decodes of an eight-plane field on a pool of two workers -- the gate is taken
    (WR_STAT_DECODE_GATE_MS moves), every reconstruction is the oracle's, and nothing is left behind."""
    f = synth.field(128, 96, 80, seed=21)
    e = oracle.encode(f, 1e-16)
    rec = oracle.decode(e, f.shape)
    e = {k: v for k, v in e.items() if k != "residual"}
    api.set_coder_pool(2, 4)
    gate0, refused0 = api.stat(api.STAT_DECODE_GATE_MS), api.stat(api.STAT_HANDOVER_ERRORS)
    errors = []

    def worker(k):
        try:
            with api.Context(0) as c:
                for rep in range(2):
                    out = np.empty_like(f)
                    if (k + rep) % 2:
                        c.decode_begin(f.shape, e)
                        c.decode_finish_host(out)
                    else:
                        c.decode_host(out, e)
                    assert bits_equal(out, rec), (k, rep)
        except Exception as exc:  # noqa: BLE001
            errors.append((k, exc))

    try:
        ths = [threading.Thread(target=worker, args=(k,)) for k in range(12)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
    finally:
        api.set_coder_pool(0)
    assert not errors, errors
    assert api.stat(api.STAT_DECODE_GATE_MS) > gate0, "no decode ever waited at the gate: 96 plane jobs on two workers"
    assert api.stat(api.STAT_HANDOVER_ERRORS) == refused0


def test_two_phase_decode(ctx, api, oracle):
    """wr_decode_begin (host range decoding, no field buffer) + wr_decode_finish_host / _device (upload, kernels,
    download): same reconstruction as the one-call decode, with per-call coder threads and with the pool; the
    coded bytes may be dropped after begin; a finish without a begin is an error."""
    f = synth.field(180, 190, 200, seed=21)
    want = oracle.encode(f, 1e-7)
    rec = oracle.decode(want, f.shape)
    for pool in (0, 3):
        api.set_coder_pool(pool)
        try:
            enc = dict(want)
            enc["data"] = want["data"].copy()
            ctx.decode_begin(f.shape, enc)
            enc["data"][:] = 0          # not needed any more
            out = np.full(f.shape, -1.0)
            ctx.decode_finish_host(out)
            assert bits_equal(out, rec)
            ctx.decode_begin(f.shape, want)
            buf = ctx.alloc(f.nbytes)
            ctx.decode_finish(buf)
            assert bits_equal(buf.download(np.float64, f.size), rec)
            buf.free()
        finally:
            api.set_coder_pool(0)
    with pytest.raises(api.WaveRangeError, match="without a wr_decode_begin"):
        ctx.decode_finish_host(np.empty(f.shape))
    # an encode on the context takes the planes a begin parked there: the finish says so instead of decoding garbage
    ctx.decode_begin(f.shape, want)
    enc2, _ = ctx.encode_host(f.copy(), 1e-7)
    same_as_oracle(enc2, want)
    with pytest.raises(api.WaveRangeError, match="without a wr_decode_begin"):
        ctx.decode_finish_host(np.empty(f.shape))
    # trivial field through the two calls
    g = np.full((4, 5, 6), 2.5)
    e, _ = ctx.encode_host(g, 1e-6)
    ctx.decode_begin(g.shape, e)
    out = np.zeros_like(g)
    ctx.decode_finish_host(out)
    assert np.array_equal(out, g)


@pytest.mark.parametrize("env", [{"WR_WINDOW_BLOCKS": "1"}, {"WR_WINDOW_BLOCKS": "2", "WR_NO_DMA": "1"},
                                 {"WR_WINDOW_BLOCKS": "4", "WR_PLANE_CHUNK_MB": "1"}],
                         ids=["one_block_windows", "two_block_windows_hipMemcpyAsync", "planes_in_1MiB_chunks"])
def test_small_windows_on_every_path(env):
    """The planes reach the host coder through 15 MB windows of a pinned ring; with WR_WINDOW_BLOCKS=1 a window is one
    coder block (60000 symbols), so the small fields of the tests in this file and of the parity file cross dozens of
    window boundaries on every path (thread per plane, grouped threads, the pool, two-call decodes, the drop-in
    symbols): run them again in a child process with that setting, and once more with the window copies on
    hipMemcpyAsync and the copy streams (WR_NO_DMA=1: what happens without ROCr's DMA interface), and once with the planes
    in chunks of 1 MiB that drain under the encoder's coder (the storage of large planes, wr_pipeline.cpp: here every plane
    of 2 MiB or more)."""
    here = os.path.dirname(os.path.abspath(__file__))
    sel = ("(codec or trivial or drop_in or local_cutoff or error_paths or concurrent_contexts or grouped_coder or random_shapes "
           "or zero_minimum or host_entry_points or plane_ordered or coder_pool or two_phase or beyond_the_launch "
           "or device_planes or concurrent_host_calls) and not (full_size or large_roundtrip or config4 or small_windows)")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.join(here, "test_gpu_host_api.py"),
                        os.path.join(here, "test_gpu_parity.py"), "-k", sel],
                       env=dict(os.environ, **env), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


def test_device_planes_are_shared_between_contexts(api, oracle):
    """The quantized planes live in device buffers that belong to the device, not to the context: three contexts used
    one after the other hold one set of buffers between them; planes parked by wr_decode_begin stay untouched while
    other contexts borrow and return buffers, and go back to the pool after the finish."""
    f = synth.field(96, 100, 104, seed=33)
    g = synth.field(96, 100, 104, seed=34)
    want_f, want_g = oracle.encode(f, 1e-7), oracle.encode(g, 1e-7)
    pitch = (f.size + 255) // 256 * 256
    base = api.stat(api.STAT_DEVICE_PLANE_BYTES)
    ctxs = [api.Context(0) for _ in range(3)]
    try:
        for c in ctxs:
            enc, _ = c.encode_host(f.copy(), 1e-7)
            same_as_oracle(enc, want_f)
        one_set = api.stat(api.STAT_DEVICE_PLANE_BYTES) - base
        assert one_set <= (want_f["nlay"] + 1) * pitch, one_set         # at most one new set (idle buffers of earlier tests fit too), not three
        ctxs[0].decode_begin(f.shape, want_f)                           # parks nlay planes in context 0
        for c in ctxs[1:]:                                              # the others borrow different buffers meanwhile
            enc, _ = c.encode_host(g.copy(), 1e-7)
            same_as_oracle(enc, want_g)
            out = np.empty(g.shape)
            c.decode_host(out, want_g)
            assert bits_equal(out, oracle.decode(want_g, g.shape))
        out = np.empty(f.shape)
        ctxs[0].decode_finish_host(out)
        assert bits_equal(out, oracle.decode(want_f, f.shape))
        two_sets = api.stat(api.STAT_DEVICE_PLANE_BYTES) - base
        assert two_sets <= 2 * (max(want_f["nlay"], want_g["nlay"]) + 1) * pitch, two_sets
    finally:
        for c in ctxs:
            c.close()


def test_host_api_error_paths(ctx, api):
    """The host entry points return error codes (never crash, never fall back): null field, coded buffer shorter than
    the header says, a header with an impossible transform depth, too small an output capacity, a bad device index;
    the context keeps working afterwards."""
    import ctypes as C
    f = synth.field(48, 40, 24, seed=5)
    enc, _ = ctx.encode_host(f, 1e-6)
    enc["data"] = enc["data"].copy()
    L = api.lib()
    info, tm = api.EncInfo.from_dict(enc), api.Timings()
    out = np.empty_like(f)
    # null host pointers
    assert L.wr_decode_host(ctx.h, None, 48, 40, 24, C.byref(info), enc["data"].ctypes.data, enc["data"].size, C.byref(tm)) != 0
    cut = np.array([1e-6])
    assert L.wr_encode_host(ctx.h, None, 48, 40, 24, 1, 1, 1, 1, cut.ctypes.data_as(C.POINTER(C.c_double)), C.byref(info),
                            enc["data"].ctypes.data, enc["data"].size, C.byref(tm)) != 0
    # the coded buffer is shorter than ntot_enc
    info = api.EncInfo.from_dict(enc)
    rc = L.wr_decode_host(ctx.h, out.ctypes.data, 48, 40, 24, C.byref(info), enc["data"].ctypes.data, enc["data"].size - 1, C.byref(tm))
    assert rc != 0 and b"length of the coded buffer" in L.wr_last_error()
    # impossible transform depth in the header
    bad = dict(enc, wlev=3)
    with pytest.raises(api.WaveRangeError, match="wlev"):
        ctx.decode_host(out, bad)
    # output capacity too small
    small = np.empty(enc["ntot_enc"] // 2, dtype=np.uint8)
    with pytest.raises(api.WaveRangeError, match="encoded array is too large"):
        ctx.encode_host(f, 1e-6, out=small)
    # the slot count: out-of-range values are clamped, a device index beyond the table is an error
    api.set_device_slots(0, 3)
    with pytest.raises(api.WaveRangeError, match="device index"):
        api.set_device_slots(1000, 2)
    # a device allocation the GPU cannot serve: an error, and nothing of it is left behind as the thread's "last error" for the
    # next call's launch check to trip over (round 5: a refused 8.6 GB allocation failed the encode that followed it)
    with pytest.raises(api.WaveRangeError, match="hipMalloc"):
        ctx.alloc(1 << 42)
    # and the context still works
    again, _ = ctx.encode_host(f, 1e-6)
    assert np.array_equal(again["data"], enc["data"])
    ctx.decode_host(out, enc)
    assert np.abs(out - f).max() <= 1.05e-6 * np.abs(f).max()
    # the plane pool keeps the calls' plane memory for the next ones; wr_ctx_trim hands what is idle back to the device
    assert api.stat(api.STAT_DEVICE_PLANE_BYTES) > 0
    ctx.trim()
    assert api.stat(api.STAT_DEVICE_PLANE_BYTES) == 0
    again, _ = ctx.encode_host(f, 1e-6)
    assert np.array_equal(again["data"], enc["data"])


def test_caller_registered_buffers(ctx, api, oracle):
    """a field and an output the caller pinned itself (hipHostRegister through wr_host_register).  ROCr knows such
    memory but the GPU sees it at another address; the library must not hand the host address to its SDMA path.  Big
    enough (>= 1 MiB) for every bulk-copy path, wr_dev_upload / wr_dev_download included."""
    f = synth.field(200, 120, 72, seed=31)
    want = oracle.encode(f, 1e-8)
    src, out = f.copy(), np.full_like(f, -1.0)
    with api.registered(src), api.registered(out):
        enc, _ = ctx.encode_host(src, 1e-8)
        same_as_oracle(enc, want)
        enc["data"] = enc["data"].copy()
        ctx.decode_host(out, enc)
        assert bits_equal(out, oracle.decode(want, f.shape))
        ctx.set_keep_residual(True)   # the residual download into registered memory
        try:
            ctx.encode_host(src, 1e-8)
        finally:
            ctx.set_keep_residual(False)
        assert bits_equal(src, want["residual"])
        src[...] = f
        dbuf = ctx.to_device(src)
        back = np.empty_like(src)
        with api.registered(back):
            api._check(api.lib().wr_dev_download(ctx.h, back.ctypes.data, dbuf.ptr, back.nbytes))
            assert bits_equal(back, f)
        dbuf.free()


def test_pool_stopped_under_running_calls(api, oracle):
    """another thread stops the coder pool while calls are in flight: their planes are coded by the calls' own
    threads instead of waiting for workers that are gone; the bytes stay the same."""
    f = synth.field(160, 96, 64, seed=8)
    want = oracle.encode(f, 1e-7)
    errs = []

    def caller():
        try:
            with api.Context(0) as c:
                out = np.empty_like(f)
                for _ in range(6):
                    enc, _ = c.encode_host(f, 1e-7)
                    same_as_oracle(enc, want)
                    enc["data"] = enc["data"].copy()
                    c.decode_host(out, enc)
                    assert bits_equal(out, oracle.decode(want, f.shape))
        except BaseException as exc:  # noqa: BLE001
            errs.append(exc)

    api.set_coder_pool(4, 4)
    try:
        ths = [threading.Thread(target=caller) for _ in range(3)]
        for t in ths:
            t.start()
        for k in range(12):   # the pool comes and goes under them
            api.set_coder_pool(0 if k % 2 == 0 else 3, 4)
        for t in ths:
            t.join(timeout=300)
            assert not t.is_alive(), "a call is stuck waiting for a pool that was stopped"
    finally:
        api.set_coder_pool(0)
    if errs:
        raise errs[0]


CHUNK_WORKER = r'''
import os, sys, threading
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np
from oracle.loader import Oracle
from waverange_amd import api, synth
from util import bits_equal
api.set_verbosity(0)
o = Oracle()
shape = (128, 160, 192)                      # 3.9 M elements: planes of 4 chunks of 1 MiB
fields = [synth.field(shape[2], shape[1], shape[0], seed=70 + k) for k in range(3)]
want = [o.encode(f, 1e-8) for f in fields]
recs = [o.decode(w, f.shape) for w, f in zip(want, fields)]
errs = []
def caller(k):
    try:
        with api.Context(0) as c:
            out = np.empty_like(fields[k])
            for rep in range(4):
                enc, _ = c.encode_host(fields[k], 1e-8)
                assert enc["len_enc_vec"] == want[k]["len_enc_vec"] and np.array_equal(enc["data"], want[k]["data"]), "coded bytes"
                enc["data"] = enc["data"].copy()
                if rep %% 2:
                    c.decode_begin(fields[k].shape, enc); c.decode_finish_host(out)
                else:
                    c.decode_host(out, enc)
                assert bits_equal(out, recs[k]), "reconstruction"
    except BaseException as exc:
        errs.append(exc)
if os.environ.get("POOL"):
    api.set_coder_pool(4, 4)
else:
    # the verbose mode looks at every plane again after it has been coded (wrappers.cpp:401-409): planes do not drain then,
    # and the diagnostics read them chunk by chunk
    api.set_verbosity(1)
    with api.Context(0) as c:
        enc, _ = c.encode_host(fields[0], 1e-8)
        assert np.array_equal(enc["data"], want[0]["data"]), "verbose mode: coded bytes"
        out = np.empty_like(fields[0]); enc["data"] = enc["data"].copy()
        c.decode_host(out, enc)
        assert bits_equal(out, recs[0]), "verbose mode: reconstruction"
    api.set_verbosity(0)
    # the local-cutoff quantizer scatters into its plane: that plane is one array whatever its size
    cut = np.array([1e-8, 1e-6, 1e-7, 1e-8, 1e-5, 1e-8, 1e-7, 1e-6])
    wl = o.encode(fields[1], None, cutoff=cut, m=(2, 2, 2))
    with api.Context(0) as c:
        enc, _ = c.encode_host(fields[1], None, cutoff=cut, m=(2, 2, 2))
        assert enc["len_enc_vec"] == wl["len_enc_vec"] and np.array_equal(enc["data"], wl["data"]), "local cutoff: coded bytes"
ths = [threading.Thread(target=caller, args=(k,)) for k in range(3)]
for t in ths: t.start()
for t in ths: t.join()
if errs: raise errs[0]
chunk = 1 << 20
print("refused", api.stat(api.STAT_HANDOVER_ERRORS), "waited_ms", api.stat(api.STAT_PLANE_WAIT_MS),
      "plane bytes", api.stat(api.STAT_DEVICE_PLANE_BYTES), "chunks", api.stat(api.STAT_DEVICE_PLANE_BYTES) // chunk)
'''


@pytest.mark.parametrize("limit,pool,alloc_fail", [(None, False, None), ("40", False, None), ("40", True, None), ("34", True, None),
                                                   (None, True, "30:40"), (None, False, "5:60")])
def test_chunked_planes_drain_and_wait(tmp_path, limit, pool, alloc_fail):
    """Large planes live in chunks (the kernels index a table of them, wrk::PlaneRef); an encoder's chunks go back to the pool as
    its coder has fetched the windows they hold, and a call that finds no device memory for a plane waits for chunks to come
    back instead of failing (wr_pipeline.cpp: plane_prepare, plane_buffer_wait; WR_PLANE_LIMIT_MB caps the planes' memory).  Three callers at once, each field with 8 planes of 4 chunks (tol 1e-8): every coded byte and every
    reconstruction equal the oracle's -- with no limit, with a pool of 40 chunks (less than the 3 x 8 x 4 x 2 that three
    encodes and decodes would hold at once without draining and waiting), and with 34 (hardly more than the 32 of one
    field's planes, which a decode holds all at once: the callers take turns).
    alloc_fail: the device allocations number first .. first+count-1 of the planes fail as if the device were full
    (WR_TEST_PLANE_ALLOC_FAIL), so the path of a real exhaustion runs -- hipMalloc fails, the idle buffers are dropped, the
    call hands its quantized planes to their coders and waits without its kernel-stage lock (plane_buffer_wait) -- which the
    software cap never takes; the waits must show in WR_STAT_PLANE_WAIT_MS and no hand-over may be refused."""
    script = tmp_path / "chunks.py"
    script.write_text(CHUNK_WORKER % dict(root=ROOT))
    env = dict(os.environ, WR_PLANE_CHUNK_MB="1", WR_WINDOW_BLOCKS="2")
    if limit:
        env["WR_PLANE_LIMIT_MB"] = limit
    if pool:
        env["POOL"] = "1"
    if alloc_fail:
        env["WR_TEST_PLANE_ALLOC_FAIL"] = alloc_fail
    env["WR_FAULT_LOG"] = "1"
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "hand-over violated" not in r.stderr, r.stderr[-3000:]
    assert int(r.stdout.split("refused")[-1].split()[0]) == 0, r.stdout
    if alloc_fail:
        assert int(r.stdout.split("waited_ms")[-1].split()[0]) > 0, r.stdout
    chunks = int(r.stdout.split("chunks")[-1])
    if limit:
        assert chunks <= int(limit), r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("chunk_mb", ["1", None])
def test_stale_window_request_is_refused(tmp_path, chunk_mb):
    """A host coder that outlives its call must not reach the plane of the next call on the same context (wr_handover.h):
    the window handle of a finished call is replayed against the freshly prepared plane of the next one -- chunked (1 MiB
    chunks) and as one array.  Refused, counted in WR_STAT_HANDOVER_ERRORS, the chunk table, the ring and the window order
    of the new plane untouched.  Before the generation tickets the callback took the live stream, started a copy into its
    ring and marked a window as in flight."""
    script = tmp_path / "stale.py"
    script.write_text("import sys; sys.path.insert(0, %r)\nfrom waverange_amd import api\napi.set_verbosity(0)\n"
                      "with api.Context(0) as c:\n    c.test_stale_window(128 * 160 * 192)\n"
                      "print('refused', api.stat(api.STAT_HANDOVER_ERRORS))\n" % ROOT)
    env = dict(os.environ, WR_WINDOW_BLOCKS="2")
    if chunk_mb:
        env["WR_PLANE_CHUNK_MB"] = chunk_mb
    r = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "refused 1" in r.stdout and "hand-over violated" in r.stderr


@pytest.mark.gpu
def test_bench_takes_the_rccl_barrier_under_a_launcher_with_one_rank(tmp_path):
    """The N > 1 branch of bench.py -- init_process_group("nccl", device_id=...), the all_reduce barrier and the MAX reduction
    of the step time on CUDA tensors -- on real RCCL with the one GPU a test box has: under torch.distributed.run the process
    group is set up for WORLD_SIZE=1 as well.  (The reference's analogue of the multi-GPU run is one process per sub-domain,
    examples/mssg/divided/all_enc_dec.sh:7-11; there is no collective on the data path to test.)"""
    import json
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "WR_BENCH_BACKEND"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "1", "--size", "256", "--steps", "1", "--warmup", "0",
                        "--full", "--no-cpu-baseline", "--secondary-steps", "0"], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 1 and line["config"]["barrier"] == "rccl", line["config"]
    assert line["value"] > 0 and line["parity"] is not None


def test_bench_dump_outputs_are_what_the_timed_path_returned(tmp_path, oracle):
    """bench.py --dump-outputs at a size whose outputs fit whole: runs of different lengths write the same files, and they hold
    the header, the coded bytes and the reconstruction the oracle gives for the bench's field at every tolerance."""
    import json
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "WR_BENCH_BACKEND"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--size", "64", "--jobs", "1", "--no-cpu-baseline", "--secondary-steps", "0",
           "--no-warm-transforms"]
    dumps = []
    for steps, warmup in ((2, 1), (1, 0)):
        d = tmp_path / ("steps%d" % steps)
        r = subprocess.run(cmd + ["--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(d)], env=env, capture_output=True,
                           text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert line["steps"] == steps
        dumps.append({f[:-len(".npy")]: np.load(str(d / f)) for f in os.listdir(str(d))})
    a, b = dumps
    assert sorted(a) == sorted(b) and all(bits_equal(a[k], b[k]) for k in a)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values()) and sum(v.nbytes for v in a.values()) <= 64 * 10 ** 6
    f = synth.field(64, 64, 64, seed=12345)
    for tol in (1e-3, 1e-7):
        p = "tol%g_" % tol
        want = oracle.encode(f, tol)
        assert bits_equal(a[p + "header"], [want[k] for k in ("tolabs", "midval", "halfspanval", "wlev", "nlay", "ntot_enc")])
        assert bits_equal(a[p + "deps_vec"], want["deps_vec"]) and bits_equal(a[p + "minval_vec"], want["minval_vec"])
        assert list(a[p + "len_enc_vec"]) == want["len_enc_vec"]
        assert np.array_equal(a[p + "coded"], want["data"].astype(np.float32)) and list(a[p + "coded_blocks"]) == [0]
        assert bits_equal(a[p + "decoded"], oracle.decode(want, f.shape)) and list(a[p + "decoded_blocks"]) == [0]


def test_plain_bench_run_leaves_the_full_legs_out():
    """bench.py without --full prints the headline line and runs nothing after its timed steps: no accuracy or parity check,
    no warm-clock transforms, secondary pass, single field or CPU baseline (the legs are not switched off one by one here:
    a plain run has none of them)."""
    import json
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "WR_BENCH_BACKEND"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--size", "64", "--jobs", "1", "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["value"] > 0 and line["unit"] == "MB/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["steps"] == 1 and line["ms_per_step"] > 0
    assert not {"accuracy", "parity", "roofline_warm", "resident_fields", "secondary", "single_field", "cpu_baseline"} & set(line)
