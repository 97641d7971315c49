"""Masked fields in the tolerance searches, the part that needs no GPU: the reference the GPU test is judged by
(tests/masked_quality_cases.py) held against the contract and the guard condition for exactly the inputs
tests/test_gpu_masked_quality.py uses, and the conditions that make that test able to FAIL: a library that let the undefined
samples into the maximum, divided by n instead of nd, or judged the padded field over all n samples has to end somewhere else."""
import math

import numpy as np

import masked_quality_cases as mq
from rms_ref import GMAX, GUARD
from waverange_amd import api


def test_the_pad_is_one_division_of_an_exact_sum():
    for key in mq.all_inputs():
        f, ref = mq.ref_of(*key)
        D = ~ref.und
        assert np.all(np.round(f * 65536.0) == f * 65536.0) and np.abs(f).max() < 256.0 and f.size <= 2 ** 18
        # any order gives the same sum: forwards, backwards, pairwise (numpy) and exactly (fsum)
        v = f[D].astype(np.float64)
        s = math.fsum(v)
        assert s == float(np.sum(v)) == float(np.sum(v[::-1])) == float(np.cumsum(v)[-1])
        pad = s / ref.nd
        assert ref.pad == (float(np.float32(pad)) if f.dtype == np.float32 else pad)
        assert ref.b.flo == float(v.min()) and ref.b.fhi == float(v.max())  # the mean lies in [lo, hi]: f_pad's range is D's
        assert 0 < ref.nd < f.size and ref.nd == f.size - int(ref.und.sum())


def test_the_masks_are_what_the_table_says():
    for call in mq.CALLS:
        _, ref = mq.ref_of(*mq.key_of(call))
        share = ref.und.mean()
        mask = call[8]
        if mask in ("land", "ball"):
            assert 0.25 < share < 0.35, (call[0], share)
        elif mask == "speckle":
            flat = ref.und.reshape(-1)
            assert 0.004 < share < 0.02 and not np.any(flat[1:] & flat[:-1]), (call[0], share)
        else:
            assert int(ref.und.sum()) == 1
        g = mq.field_of(call)
        w = g.astype(np.float64)
        assert np.array_equal(~np.isfinite(w) | (w < call[10]), ref.und), call[0]


def test_the_reference_meets_the_contract_and_the_guard_on_the_gpu_tests_inputs():
    for key in mq.all_inputs():
        _, ref = mq.ref_of(*key)
        for name, norm, target, m in mq.targets_of(*key):
            if norm == api.NORM_MAX:
                g = ref.solve_max(m)
                assert g is not None and ref.verdict_max(g, m) is None, (key, name, g)
                continue
            g, trials = ref.solve(m)
            assert g is not None and trials >= 1, (key, name)
            assert ref.verdict(g, m) is None, (key, name, ref.verdict(g, m))
            assert ref.guarded(g, m), (key, name, g, m, ref.R(g), ref.R(min(g + 1, GMAX)), GUARD)
            assert ref.R(g) <= ref.E(g)
            # nd < n: a library that divided by n would report an R further than the guard from R_D*
            by_n = math.sqrt(ref.S(g) / ref.n)
            assert ref.nd < ref.n and abs(by_n - ref.R(g)) > GUARD * ref.R(g), (key, name, by_n, ref.R(g))
            if name == "psnr 60":
                assert abs(m - ref.range * 1e-3) <= 4 * np.spacing(m)


def test_the_table_can_tell_a_compare_that_ignores_the_mask():
    """at least one case where the undefined samples hold the largest difference, so that letting them in changes max_abs; and
    at least one where the padded field judged over all n samples ends on another grid point"""
    outside, other_g = [], []
    for key in mq.all_inputs():
        _, ref = mq.ref_of(*key)
        for name, norm, target, m in mq.targets_of(*key):
            if norm == api.NORM_MAX:
                g = ref.solve_max(m)
                if ref.E_out(g) > ref.E(g):
                    outside.append((key, name, g, ref.E_out(g), ref.E(g)))
                continue
            g, _ = ref.solve(m)
            if ref.E_out(g) > ref.E(g):
                outside.append((key, name, g, ref.E_out(g), ref.E(g)))
            whole, _ = ref.whole.solve(m)
            if whole != g:
                other_g.append((key, name, g, whole))
    print("undefined samples hold the maximum:", len(outside), outside[:3])
    print("another g over all n:", len(other_g), other_g[:3])
    assert outside and other_g
