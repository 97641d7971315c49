"""Single-precision host fields (wr_encode_host_f32 / wr_decode_host_f32 / wr_decode_finish_host_f32 and the drop-in shaped
wr_encoding_wrap_f32 / wr_decoding_wrap_f32): the coded stream is the one of the field widened to fp64, the reconstruction
is (float) of the fp64 one, bit for bit -- on the fused path (level 0 reads / writes fp32 in the kernels), on the partly
fused and general paths (widened / narrowed by a pass of their own), and with WR_NO_FUSED=1.
Run on the GPU box: python -m pytest tests -m gpu"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import threading

import numpy as np
import pytest

from util import ROOT, bits_equal
from waverange_amd import synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BINDIR = os.path.join(ROOT, "waverange_amd", "bin")

# (shape (nx, ny, nz), tol, wtflag, local cutoff (vector, m) or None)
CASES = {
    "fused_64": ((64, 64, 64), 1e-7, 1, None),                 # all four levels fused, min/max riding along
    "fused_128x64x80": ((128, 64, 80), 1e-4, 1, None),
    "partly_fused": ((200, 120, 72), 1e-10, 1, None),         # three levels fused forward, two inverse
    "general": ((37, 21, 13), 1e-6, 1, None),                 # no level fused
    "wtflag0": ((64, 64, 8), 1e-4, 0, None),
    "windows": ((400, 300, 272), 1e-6, 1, None),              # planes of several host windows
    "local_cutoff": ((64, 48, 40), None, 1, ([1e-3, 1e-5, 1e-4, 1e-6, 1e-5, 1e-3, 1e-6, 1e-4], (2, 2, 2))),
}


def f32_field(shape, seed=99):
    nx, ny, nz = shape
    return synth.field(nx, ny, nz, seed=seed).astype(np.float32)


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


def encode_args(case):
    _, tol, wtflag, local = CASES[case]
    if local:
        return dict(tolrel=None, wtflag=wtflag, cutoff=local[0], m=local[1])
    return dict(tolrel=tol, wtflag=wtflag)


def same_enc(enc, want):
    for k in ("tolabs", "midval", "halfspanval", "wlev", "nlay", "ntot_enc", "len_enc_vec"):
        assert enc[k] == want[k], k
    assert bits_equal(enc["deps_vec"], want["deps_vec"]) and bits_equal(enc["minval_vec"], want["minval_vec"])
    assert np.array_equal(enc["data"], want["data"])


def same_f32(a, b):
    return a.dtype == np.float32 and b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def narrow(x):
    with np.errstate(over="ignore"):
        return x.astype(np.float32)


def roundtrip(api, ctx, f, args, pinned=False):
    """encode_host_f32 + decode_host_f32 + (begin, finish_host_f32); returns (enc, rec, rec2); checks the input is untouched"""
    src = api.pinned_array(f.shape, np.float32) if pinned else np.empty_like(f)
    src[...] = f
    enc, _ = ctx.encode_host_f32(src, args["tolrel"], wtflag=args["wtflag"], cutoff=args.get("cutoff"), m=args.get("m", (1, 1, 1)))
    assert same_f32(src, f), "encode_host_f32 must not write the field"
    enc["data"] = enc["data"].copy()
    out = api.pinned_array(f.shape, np.float32) if pinned else np.empty_like(f)
    out[...] = -1.0
    ctx.decode_host_f32(out, enc)
    rec = out.copy()
    out[...] = 7.0
    ctx.decode_begin(f.shape, enc)
    ctx.decode_finish_host_f32(out)
    return enc, rec, out.copy()


def case_digests(cases=tuple(CASES)):
    """What the fp32 entry points give on each case (SHA-256 of the coded bytes and of the reconstruction's bits): compared
    between this process and a child with WR_NO_FUSED=1"""
    from waverange_amd import api
    api.set_verbosity(0)
    out = {}
    with api.Context(0) as c:
        for case in cases:
            shape = CASES[case][0]
            f = f32_field(shape)
            enc, rec, rec2 = roundtrip(api, c, f, encode_args(case))
            assert same_f32(rec, rec2)
            out[case] = [hashlib.sha256(enc["data"].tobytes()).hexdigest(), enc["len_enc_vec"],
                         hashlib.sha256(rec.view(np.uint32).tobytes()).hexdigest()]
    return out


@pytest.mark.parametrize("pinned", [True, False])
@pytest.mark.parametrize("case", sorted(CASES))
def test_f32_host_entry_points_vs_oracle(api, ctx, oracle, case, pinned):
    f = f32_field(CASES[case][0])
    args = encode_args(case)
    want = oracle.encode(f.astype(np.float64), args["tolrel"], wtflag=args["wtflag"], cutoff=args.get("cutoff"), m=args.get("m", (1, 1, 1)))
    enc, rec, rec2 = roundtrip(api, ctx, f, args, pinned)
    same_enc(enc, want)
    expect = narrow(oracle.decode(want, f.shape))
    assert same_f32(rec, expect), "decode_host_f32 differs from (float) of the fp64 reconstruction"
    assert same_f32(rec2, expect), "decode_begin + decode_finish_host_f32 differs"


def test_f32_without_fused_kernels_gives_the_same(api, ctx):
    here = case_digests()
    code = "import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_f32 as t; print(json.dumps(t.case_digests()))" % (ROOT, HERE)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, WR_NO_FUSED="1", WR_QUIET="1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    there = json.loads(r.stdout.strip().splitlines()[-1])
    assert there == here


def edge_fields():
    rng = np.random.default_rng(5)
    n = (64, 64, 64)
    base = f32_field(n, seed=7)
    out = {}
    out["constant"] = (np.full(base.shape, 1.25, np.float32), 1e-6)
    pos = np.abs(base)
    pz = pos.copy()
    pz.reshape(-1)[rng.choice(pz.size, 50, replace=False)] = -0.0
    pz.reshape(-1)[-3] = 0.0          # the last zero is +0.0
    out["min_zero_last_plus"] = (pz, 1e-5)
    mz = pos.copy()
    mz.reshape(-1)[rng.choice(mz.size, 50, replace=False)] = 0.0
    mz.reshape(-1)[-3] = -0.0         # the last zero is -0.0
    out["min_zero_last_minus"] = (mz, 1e-5)
    sub = (base.astype(np.float64) * 1e-40).astype(np.float32)   # fp32 subnormals (below 1.18e-38)
    assert np.count_nonzero(np.abs(sub) < np.finfo(np.float32).tiny) > sub.size // 2
    out["subnormal"] = (sub, 1e-3)
    big = (base.astype(np.float64) / np.abs(base).max() * float(np.finfo(np.float32).max)).astype(np.float32)
    out["near_flt_max"] = (big, 1e-3)
    out["near_flt_max_overflow"] = (big, 1e-2)   # here the reconstruction exceeds FLT_MAX at two points: inf
    # the general path too: a shape no level of which is fused, with a zero minimum whose last zero is -0.0
    g = np.abs(f32_field((37, 21, 13), seed=3))
    g.reshape(-1)[[5, 100, 2000]] = [0.0, 0.0, -0.0]
    out["general_min_zero_last_minus"] = (g, 1e-6)
    return out


@pytest.mark.parametrize("name", sorted(edge_fields()))
def test_f32_edge_fields(api, ctx, oracle, name):
    f, tol = edge_fields()[name]
    want = oracle.encode(f.astype(np.float64), tol)
    enc, rec, rec2 = roundtrip(api, ctx, f, dict(tolrel=tol, wtflag=1))
    same_enc(enc, want)
    if name == "constant":
        assert enc["nlay"] == 0
    expect = narrow(oracle.decode(want, f.shape))
    assert same_f32(rec, expect) and same_f32(rec2, expect)
    if name == "near_flt_max_overflow":
        assert np.isinf(rec).sum() > 0, "the case is meant to overflow"
    if name == "subnormal":
        assert np.count_nonzero((rec != 0) & (np.abs(rec) < np.finfo(np.float32).tiny)) > 0, "subnormals must survive"


def test_f32_1024_cube_equals_widened_fp64(api, ctx):
    n = 1024
    f = synth.field(n, n, n).astype(np.float32)
    g = f.astype(np.float64)
    tol = 1e-3
    enc32, _ = ctx.encode_host_f32(f, tol)
    enc32["data"] = enc32["data"].copy()
    enc64, _ = ctx.encode_host(g, tol)
    same_enc(enc32, enc64)
    del g
    rec64 = np.empty((n, n, n))
    ctx.decode_host(rec64, enc64)
    want = narrow(rec64)
    del rec64
    rec32 = np.empty_like(f)
    ctx.decode_host_f32(rec32, enc32)
    assert same_f32(rec32, want)


def test_f32_and_fp64_concurrently_on_four_contexts(api):
    shapes = [(64, 64, 64), (200, 120, 72), (37, 21, 13), (128, 64, 80)]
    fields = [f32_field(s, seed=20 + i) for i, s in enumerate(shapes)]

    def one(c, f, use_f32):
        if use_f32:
            enc, _ = c.encode_host_f32(f, 1e-6)
            enc["data"] = enc["data"].copy()
            out = np.empty_like(f)
            c.decode_host_f32(out, enc)
        else:
            g = f.astype(np.float64)
            enc, _ = c.encode_host(g, 1e-6)
            enc["data"] = enc["data"].copy()
            out = np.empty_like(g)
            c.decode_host(out, enc)
        return hashlib.sha256(enc["data"].tobytes()).hexdigest(), hashlib.sha256(out.tobytes()).hexdigest()

    with api.Context(0) as c:
        single = {(i, m): one(c, f, m) for i, f in enumerate(fields) for m in (True, False)}
    api.set_coder_pool(8, 4)
    try:
        results, errors = {}, []

        def worker(i):
            try:
                with api.Context(0) as c:
                    for rep in range(3):
                        for m in ((True, False) if (i + rep) % 2 else (False, True)):
                            results[(i, m, rep)] = one(c, fields[i], m)
            except Exception as e:  # noqa: BLE001 -- reported below
                errors.append(repr(e))
        ts = [threading.Thread(target=worker, args=(i,)) for i in range(4)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
    finally:
        api.set_coder_pool(0)
    assert not errors, errors
    for (i, m, rep), r in results.items():
        assert r == single[(i, m)], (i, m, rep)
    assert len(results) == 4 * 2 * 3


def test_f32_error_paths(api, ctx):
    f = f32_field((64, 64, 64))
    ctx.set_keep_residual(True)
    try:
        with pytest.raises(api.WaveRangeError, match="error -3"):
            ctx.encode_host_f32(f, 1e-6)
    finally:
        ctx.set_keep_residual(False)
    assert same_f32(f, f32_field((64, 64, 64)))
    L = api.lib()
    info, tm = api.EncInfo(), api.Timings()
    cut = (C.c_double * 1)(1e-6)
    buf = np.empty(1 << 20, np.uint8)
    rc = L.wr_encode_host_f32(ctx.h, None, 64, 64, 64, 1, 1, 1, 1, cut, C.byref(info), buf.ctypes.data, buf.size, C.byref(tm))
    assert rc == -1  # WR_ERR_ARG
    with pytest.raises(api.WaveRangeError, match="error -5"):  # WR_ERR_OVERFLOW
        ctx.encode_host_f32(f, 1e-10, out=np.empty(1000, np.uint8))
    enc, _ = ctx.encode_host_f32(f, 1e-6)
    enc["data"] = enc["data"].copy()
    short = dict(enc, data=enc["data"][: enc["ntot_enc"] // 2])
    with pytest.raises(api.WaveRangeError):
        ctx.decode_host_f32(np.empty_like(f), short)
    rc = L.wr_decode_host_f32(ctx.h, None, 64, 64, 64, C.byref(api.EncInfo.from_dict(enc)), enc["data"].ctypes.data, enc["data"].size, None)
    assert rc == -1
    # the context is still good
    out = np.empty_like(f)
    ctx.decode_host_f32(out, enc)


def test_f32_drop_in_wrappers_equal_explicit_context(api, ctx):
    L = api.lib()
    _dp, _u8p, _ulp = C.POINTER(C.c_double), C.POINTER(C.c_ubyte), C.POINTER(C.c_ulong)
    L.wr_encoding_wrap_f32.restype = None
    L.wr_encoding_wrap_f32.argtypes = [C.c_int] * 3 + [C.c_void_p] + [C.c_int] * 4 + [_dp] * 4 + [_u8p, _u8p, _ulp, _dp, _dp, _ulp, C.c_void_p]
    L.wr_decoding_wrap_f32.restype = None
    L.wr_decoding_wrap_f32.argtypes = [C.c_int] * 3 + [C.c_void_p] + [_dp] * 3 + [_u8p, _u8p, _ulp, _dp, _dp, _ulp, C.c_void_p]
    for shape in ((64, 64, 64), (37, 21, 13)):
        nx, ny, nz = shape
        f = f32_field(shape, seed=11)
        want, _ = ctx.encode_host_f32(f, 1e-6)
        _, cap = api.setup_wr(nx, ny, nz)
        data = np.zeros(cap, np.uint8)
        cut = (C.c_double * 1)(1e-6)
        tolabs, midval, half = C.c_double(), C.c_double(), C.c_double()
        wlev, nlay, ntot = C.c_ubyte(), C.c_ubyte(), C.c_ulong()
        deps, mins, lens = (C.c_double * 8)(), (C.c_double * 8)(), (C.c_ulong * 8)()
        src = f.copy()
        L.wr_encoding_wrap_f32(nx, ny, nz, src.ctypes.data, 1, 1, 1, 1, cut, C.byref(tolabs), C.byref(midval), C.byref(half), C.byref(wlev),
                               C.byref(nlay), C.byref(ntot), deps, mins, lens, data.ctypes.data)
        assert same_f32(src, f), "wr_encoding_wrap_f32 must not write the field"
        assert ntot.value == want["ntot_enc"] and nlay.value == want["nlay"] and wlev.value == want["wlev"]
        assert list(lens)[: nlay.value] == want["len_enc_vec"]
        assert bits_equal(np.array(list(deps)[: nlay.value]), want["deps_vec"]) and bits_equal(np.array(list(mins)[: nlay.value]), want["minval_vec"])
        assert np.array_equal(data[: ntot.value], want["data"])
        out = np.empty_like(f)
        L.wr_decoding_wrap_f32(nx, ny, nz, out.ctypes.data, C.byref(tolabs), C.byref(midval), C.byref(half), C.byref(wlev), C.byref(nlay),
                               C.byref(ntot), deps, mins, lens, data.ctypes.data)
        want["data"] = want["data"].copy()
        rec = np.empty_like(f)
        ctx.decode_host_f32(rec, want)
        assert same_f32(out, rec)


def run_cli(d, argv_enc, env):
    subprocess.run([os.path.join(BINDIR, "wrenc")] + argv_enc, cwd=d, check=True, stdout=subprocess.DEVNULL, env=env, timeout=600)
    subprocess.run([os.path.join(BINDIR, "wrdec"), "data.wrb", "data.wrh", "datarec.bin", "2", "0"], cwd=d, check=True,
                   stdout=subprocess.DEVNULL, env=env, timeout=600)
    return {n: open(os.path.join(d, n), "rb").read() for n in ("data.wrh", "data.wrb", "datarec.bin")}


@pytest.mark.parametrize("case", ["argv_two_fp32", "inmeta_new_type0", "inmeta_old_type1_bigendian"])
def test_our_cli_fp32_cases_through_the_f32_entry_points(case):
    """the fp32 records of these cases go through wr_encoding_wrap_f32 / wr_decoding_wrap_f32 (our library has them);
    the files must be the reference's (golden), as on the widening path"""
    import cli_cases
    from test_cli import run_case
    with open(os.path.join(ROOT, "tests", "golden", "cli.json")) as fh:
        g = json.load(fh)[case]
    run_case(case, os.path.join(BINDIR, "wrenc"), os.path.join(BINDIR, "wrdec"), g)
    run_case(case, os.path.join(BINDIR, "wrenc"), os.path.join(BINDIR, "wrdec"), g, WR_CLI_WIDEN_ON_HOST="1")
    assert any(fd["spec"][0] == 4 and fd["icomp"] for fd in cli_cases.CASES[case]["fields"])


def test_our_cli_fp32_256_cube_equals_widening_path(oracle):
    n = 256
    f = synth.field(n, n, n, seed=31).astype(np.float32)
    argv = ["data.bin", "data.wrb", "data.wrh", "2", "0", "1", "1", str(n), str(n), str(n), "1e-5"]
    with tempfile.TemporaryDirectory() as d:
        f.tofile(os.path.join(d, "data.bin"))
        env = dict(os.environ, WR_QUIET="1")
        direct = run_cli(d, argv, env)
        widened = run_cli(d, argv, dict(env, WR_CLI_WIDEN_ON_HOST="1"))
    assert direct == widened
    rec = np.frombuffer(direct["datarec.bin"], np.float32).reshape(f.shape)
    want = oracle.encode(f.astype(np.float64), 1e-5)
    assert direct["data.wrb"] == want["data"].tobytes()
    assert same_f32(rec, narrow(oracle.decode(want, f.shape)))
