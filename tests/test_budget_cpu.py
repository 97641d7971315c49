"""Encode to a byte budget, the parts that need no GPU: the tolerance grid, the size bound of a plane against the host segment
encoder on the planes that break coders, its tightness on real planes, the stand-alone ASan + UBSan harness, and the
plain-Python B(g) the GPU tests are judged by (tests/budget_ref.py)."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import coder_cases as cc
from budget_ref import BudgetRef
from util import ROOT
from oracle.loader import Oracle
from waverange_amd import api, synth

CSRC = os.path.join(ROOT, "waverange_amd", "csrc")
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
SEGS = [16, 1024, 59904]


def test_grid_is_strictly_increasing_with_exact_ends():
    t = [api.budget_tol(g) for g in range(api.BUDGET_GMAX + 1)]
    assert all(b > a for a, b in zip(t, t[1:]))
    assert t[0] == 2.0 ** -60 and t[-1] == 1.0
    assert all(b / a <= 65 / 64 for a, b in zip(t, t[1:]))
    # the formula of the header, in Python's exact arithmetic
    assert all(t[g] == np.ldexp(float(64 + (g & 63)), (g >> 6) - 66) for g in range(api.BUDGET_GMAX + 1))


def test_grid_index_inverts_the_grid_and_clamps():
    for g in range(api.BUDGET_GMAX + 1):
        assert api.budget_index(api.budget_tol(g)) == g
    for g in range(1, api.BUDGET_GMAX + 1):  # just above a point: the next one; just below: the point itself
        t = api.budget_tol(g)
        assert api.budget_index(np.nextafter(t, 0.0)) == g
        assert api.budget_index(np.nextafter(t, 2.0)) == min(g + 1, api.BUDGET_GMAX)
    assert api.budget_index(0.0) == 0 and api.budget_index(2.0 ** -80) == 0 and api.budget_index(-1.0) == 0
    assert api.budget_index(1.0) == api.BUDGET_GMAX and api.budget_index(7.0) == api.BUDGET_GMAX and api.budget_index(np.inf) == api.BUDGET_GMAX
    assert api.budget_tol(-5) == api.budget_tol(0) and api.budget_tol(10 ** 6) == 1.0
    assert api.budget_index(1e-6) == min(g for g in range(api.BUDGET_GMAX + 1) if api.budget_tol(g) >= 1e-6)


def test_the_bound_is_a_bound_on_the_planes_that_break_coders():
    """every plane of tests/coder_cases.py (each distinct plane once), with segments of 16, 1024 and 59904 symbols"""
    seen, bad, kinds, shapes = set(), [], set(), set()
    for c in cc.all_cases():
        p = cc.case_plane(c)
        key = (p.size, p.tobytes())
        if key in seen:
            continue
        seen.add(key)
        kinds.add(c[0])
        for seg in SEGS:
            shapes.add("n<seg" if p.size < seg else "n%seg==0" if p.size % seg == 0 else "n%seg==1" if p.size % seg == 1 else "other")
            bound, blob = api.seg_size_bound_host_ref(p, seg), api.seg_encode_host_ref(p, seg)
            if bound < len(blob):
                bad.append((cc.case_id(c), seg, bound, len(blob)))
    assert not bad, bad[:10]
    # the table holds what this test relies on: one symbol, two symbols, a count of one, all 256, and the three length classes
    assert {"const_0", "alternate", "one_off_first_0", "uniform", "floor256"} <= kinds
    assert {"n<seg", "n%seg==0", "n%seg==1"} <= shapes


@pytest.mark.parametrize("seg", SEGS)
def test_the_bound_on_hand_made_planes(seg):
    rng = np.random.default_rng(seg)
    planes = {
        "one symbol": np.full(3 * seg, 9, np.uint8),
        "two symbols": (np.arange(2 * seg + 1) & 1).astype(np.uint8),
        "all 256 equally": (np.arange(256 * max(1, seg // 256) * 2) % 256).astype(np.uint8),
        "a count of one": np.concatenate([np.zeros(seg - 1, np.uint8), [200]]).astype(np.uint8),
        "n < seg": rng.integers(0, 256, max(1, seg // 3), dtype=np.uint8),
        "n = 4 seg": rng.integers(0, 8, 4 * seg, dtype=np.uint8),
        "n = 2 seg + 1": rng.integers(0, 3, 2 * seg + 1, dtype=np.uint8),
        "one symbol of one": np.zeros(1, np.uint8),
    }
    for name, p in planes.items():
        bound, blob = api.seg_size_bound_host_ref(p, seg), api.seg_encode_host_ref(p, seg)
        assert len(blob) <= bound <= api.seg_bound(p.size, seg), (name, bound, len(blob))


def test_the_bound_refuses_what_the_encoder_refuses():
    for seg in (8, 17, 60000):
        with pytest.raises(api.WaveRangeError):
            api.seg_size_bound_host_ref(np.zeros(64, np.uint8), seg)
    assert api.seg_size_bound_host_ref(np.zeros(0, np.uint8), 16) == 12  # an empty plane: the header


@pytest.mark.parametrize("tol", [1e-3, 1e-7])
def test_the_bound_is_tight_on_real_planes(tol):
    """On the oracle-quantized planes of a 48^3 field the slack (B - ntot_enc) / ntot_enc of the stream is below 1 % -- a condition
    that keeps the bound from being trivially loose.  The plain bound wr_seg_bound fails it by a wide margin (127700 bytes per
    plane whatever is in it); the new one gives 0.63 % at 1e-3 and 0.23 % at 1e-7.  What is left is the coder's worst-case
    rounding loss, 0.0095 bit per symbol or 64 to 72 bytes per segment whatever the segment's entropy: on the one nearly
    constant plane of this field (2269 bytes in two segments) that alone is 5.6 % of the plane's blob, on the others 0.1 - 0.3 %."""
    o = Oracle()
    f = synth.field(48, 48, 48, seed=11)
    n = f.size
    enc = o.encode(f, tol)
    at, blob_sum, bound_sum, plain_sum = 0, 0, 0, 0
    for ln in enc["len_enc_vec"]:
        plane, got = o.range_decode(enc["data"][at:at + ln], n)
        assert got == n
        at += ln
        blob, bound = api.seg_encode_host_ref(plane[:n]), api.seg_size_bound_host_ref(plane[:n])
        print("tol %g: blob %d bound %d plain bound %d" % (tol, len(blob), bound, api.seg_bound(n)))
        assert len(blob) <= bound
        blob_sum += len(blob)
        bound_sum += bound
        plain_sum += api.seg_bound(n)
    assert enc["nlay"] >= 2
    assert bound_sum - blob_sum < 0.01 * blob_sum, (bound_sum, blob_sum)
    assert bound_sum - blob_sum < 0.0075 * blob_sum  # with room to spare
    assert plain_sum - blob_sum > 0.5 * blob_sum  # the existing bound is not this: it fails the condition fifty times over


def test_budget_fuzz_under_asan_ubsan():
    """the bound, its table and the grid as a stand-alone program under ASan + UBSan (tests/native/budget_fuzz.cpp)"""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "budget_fuzz")
        subprocess.check_call(["g++"] + SAN + ["-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "budget_fuzz.cpp"),
                                               "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "budget bound sanitizer run OK" in r.stdout
        assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_python_B_is_the_bound_of_the_oracles_planes():
    """B(g) of tests/budget_ref.py against the oracle's own encode at budget_tol(g): the same planes, hence the same header
    scalars, and B(g) above the segmented stream built from them."""
    o = Oracle()
    f = synth.field(24, 20, 16, seed=5)
    ref = BudgetRef(o, f, seg=1024)
    for g in (api.budget_index(1e-2), api.budget_index(1e-5), api.budget_index(1e-9)):
        enc = o.encode(f, api.budget_tol(g))
        ps = ref.planes(g)
        assert len(ps) == enc["nlay"] == ref.nlay(g)
        assert np.array_equal(np.array([d for _, d, _ in ps]).view(np.uint64), enc["deps_vec"].view(np.uint64))
        assert np.array_equal(np.array([m for _, _, m in ps]).view(np.uint64), enc["minval_vec"].view(np.uint64))
        at, total = 0, 0
        for (q, _, _), ln in zip(ps, enc["len_enc_vec"]):
            plane, got = o.range_decode(enc["data"][at:at + ln], f.size)
            assert got == f.size and np.array_equal(plane[:f.size], q)
            at += ln
            total += len(api.seg_encode_host_ref(q, 1024))
        assert total <= ref.B(g) == sum(api.seg_size_bound_host_ref(q, 1024) for q, _, _ in ps)
    # the intervals: plane l is the last one exactly on last_interval(l)
    for l in range(3):
        a, b = ref.last_interval(l)
        assert ref.nlay(a) == ref.nlay(b) == l + 1 and (a == 0 or ref.nlay(a - 1) == l + 2) and (b == api.BUDGET_GMAX or ref.nlay(b + 1) == l)
    assert BudgetRef(o, np.full((4, 4, 4), 3.5)).B(100) == 0
