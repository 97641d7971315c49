"""Encode to an error bound, the parts that need no GPU: wr_bounded_start against a scan of the grid, the plain-Python E(g) the
GPU tests are judged by (tests/bounded_ref.py) against an actual oracle encode + decode, the reference held against the contract
of the bounded calls for exactly the inputs the GPU tests use (tests/bounded_cases.py), and the stand-alone ASan + UBSan harness
of the start point and the search's host logic."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import bounded_cases as bc
from bounded_ref import BoundedRef, start_scan
from util import ROOT
from oracle.loader import Oracle
from waverange_amd import api, synth

CSRC = os.path.join(ROOT, "waverange_amd", "csrc")
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
GMAX = api.BUDGET_GMAX


@pytest.mark.parametrize("absmax", [1.0, 3.0, 1e-300, 1e300])
def test_bounded_start_equals_a_scan_of_the_grid(absmax):
    a = np.float64(absmax)
    prod = [np.float64(api.budget_tol(g)) * a for g in range(GMAX + 1)]  # one fp64 multiply each, as the library's
    assert all(y >= x for x, y in zip(prod, prod[1:]))

    def scan(m):
        hit = [g for g in range(GMAX + 1) if prod[g] <= m]
        return hit[-1] if hit else -1

    # bounds that hit a grid point exactly, and one ulp to either side of it
    for g in list(range(0, GMAX + 1, 97)) + [1, 63, 64, 65, GMAX - 1, GMAX]:
        for m in (prod[g], np.nextafter(prod[g], 0.0), np.nextafter(prod[g], np.inf)):
            assert api.bounded_start(m, absmax) == scan(m), (g, m)
        assert api.bounded_start(prod[g], absmax) >= g  # (several points share a product only where it is subnormal)
    assert scan(prod[GMAX // 2]) == start_scan(prod[GMAX // 2], absmax)
    # below the grid: -1; above it: clamped
    assert api.bounded_start(np.nextafter(prod[0], 0.0), absmax) == -1
    assert api.bounded_start(prod[0] / 4, absmax) == -1
    if np.isfinite(prod[GMAX] * 2):
        assert api.bounded_start(prod[GMAX] * 2, absmax) == GMAX
    assert api.bounded_start(np.finfo(np.float64).max, absmax) == GMAX


def test_bounded_start_refuses_what_is_not_a_positive_finite_number():
    for bad in (0.0, -0.0, -1.0, np.nan, np.inf, -np.inf):
        assert api.bounded_start(bad, 1.0) == -1, bad
        assert api.bounded_start(1.0, bad) == -1, bad
    assert api.bounded_start(1.0, 1.0) == GMAX and api.bounded_start(2.0 ** -60, 1.0) == 0
    assert api.bounded_start(np.nextafter(2.0 ** -60, 0.0), 1.0) == -1


@pytest.mark.parametrize("kind", bc.KINDS)
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_the_reference_equals_an_oracle_encode_and_decode(kind, f32):
    """E(g) of tests/bounded_ref.py at three grid points of a (16,16,16) field against wro_encode + wro_decode at budget_tol(g)"""
    o = Oracle()
    f = bc.make_field(kind, (16, 16, 16))
    if f32:
        f = f.astype(np.float32)
    ref = BoundedRef(o, f)
    wide = f.astype(np.float64)
    for g in (api.budget_index(1e-3), api.budget_index(1e-7), api.budget_index(3e-12)):
        enc = o.encode(wide, api.budget_tol(g))
        assert enc["nlay"] == ref.nlay(g) == len(ref.planes(g))
        rec = o.decode(enc, f.shape).reshape(f.shape)
        if f32:
            rec = rec.astype(np.float32)
        assert np.array_equal(rec.view(np.uint32 if f32 else np.uint64), ref.recon(g).view(np.uint32 if f32 else np.uint64)), g
        assert ref.E(g) == float(np.abs(wide - rec.astype(np.float64)).max()), g
    assert {ref.nlay(api.budget_index(t)) for t in (1e-3, 1e-7, 3e-12)} >= {2, 4}  # the points differ in their plane count


def all_driver_refs():
    for kind in bc.KINDS:
        for dims, seg in bc.DRIVER_CASES:
            yield kind, dims, bc.ref_of(kind, dims, seg)[1]
    for kind in bc.KINDS:
        yield kind, bc.WT0_CASE[0], bc.ref_of(kind, bc.WT0_CASE[0], bc.WT0_CASE[1], wtflag=0)[1]
    yield "smooth", (64, 64, 64), bc.ref_of("smooth", (64, 64, 64), 0, f32=True)[1]


def test_the_reference_meets_the_contract_on_the_gpu_tests_inputs():
    """every assertion test_gpu_bounded.py makes of the library, made of the reference's own answer first"""
    for kind, dims, ref in all_driver_refs():
        for name, m in bc.bounds_of(ref):
            g = ref.solve(m)
            assert g is not None, (kind, dims, name)
            assert ref.verdict(g, m) is None, (kind, dims, name, ref.verdict(g, m))
            assert ref.E(g) <= m and (g == GMAX or ref.E(g + 1) > m)
            assert ref.nlay(g) >= 1
        e = ref.E(bc.G_EXACT)  # equality counts as holding; the double below it does not hold at G_EXACT
        assert ref.verdict(bc.G_EXACT, e) in (None, "E(%d) = %r holds too: %d is not tight" % (bc.G_EXACT + 1, ref.E(bc.G_EXACT + 1), bc.G_EXACT))
        assert "exceeds" in ref.verdict(bc.G_EXACT, float(np.nextafter(e, 0.0)))
        # a bound above max|f| is met at or near the grid's end
        assert ref.solve(1.5 * ref.absmax) >= GMAX - 64
        # a tol_min too coarse for the bound: the call must fail (WR_ERR_BOUND)
        g_coarse = api.budget_index(1e-2)
        assert ref.E(g_coarse) > 1e-7 * ref.absmax and ref.solve(1e-7 * ref.absmax, g_min=g_coarse) is None


def test_the_gpu_tests_inputs_exercise_the_search():
    """from the reference alone: the chosen bounds make the search walk both ways on the smooth field and far on the noise field"""
    _, ref = bc.ref_of("smooth", (64, 64, 64), 0)
    finer, coarser = [], []
    for name, m in bc.bounds_of(ref):
        s = ref.start(m)
        assert 0 <= s <= GMAX
        if ref.E(s) > m:
            finer.append(name)
        if s < GMAX and ref.E(s + 1) <= m:
            coarser.append(name)
    assert finer, "no bound makes the search walk towards finer"
    assert coarser, "no bound makes the search walk towards coarser"
    _, ref = bc.ref_of("noise", (64, 64, 64), 0)
    far = [name for name, m in bc.bounds_of(ref) if abs(ref.solve(m) - ref.start(m)) >= 8]
    assert far, "the solution lies within 8 grid points of the start for every bound"


def test_a_constant_field_and_the_refusals_of_the_reference():
    ref = BoundedRef(Oracle(), np.full((4, 5, 6), 2.5))
    assert ref.constant and ref.planes(100) == [] and ref.nlay(100) == 0
    assert start_scan(np.nan, 1.0) == -1 and start_scan(1.0, 0.0) == -1 and start_scan(1.0, np.inf) == -1


def test_bounded_fuzz_under_asan_ubsan():
    """tests/native/bounded_fuzz.cpp: wr_bounded_start against a scan and the walk of the search over synthetic E, as a program
    of its own under ASan + UBSan (host code only: csrc/wr_budget.h)"""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "bounded_fuzz")
        subprocess.check_call(["g++"] + SAN + ["-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "bounded_fuzz.cpp"),
                                               "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "bounded search sanitizer run OK" in r.stdout
        assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
