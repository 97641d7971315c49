"""The inputs of the masked quality-encode tests (include/waverange_amd.h, "Masked fields in the tolerance searches"), shared by
test_masked_quality_cpu.py and test_gpu_masked_quality.py: the fields, the masks, one reference per field and the targets, made
once and never written to.  The CPU test holds the reference against the contract, the guard condition and the conditions that
make the GPU test able to fail, for exactly these inputs; the GPU test then holds the library against the reference.

Fields.  Every sample is a multiple of 2^-16 with |x| < 2^8, and n <= 2^18: a sum of any of them, in any order, is exact in fp64
(26 + 16 bits), so the pad -- the mean of the defined samples -- is known on the CPU to the bit: the exact sum, ONE IEEE division
by nd, and for an fp32 field one rounding to float.  The samples themselves are exact in fp32 (24 bits).

The reference is bounded_ref.BoundedRef / rms_ref.RmsRef on the padded field f_pad, with E, S* and R* restricted to D, the
defined samples, and R* dividing by nd = |D| (MaskedRef below)."""
import math

import numpy as np

import bounded_cases as bc
from bounded_ref import BoundedRef
from oracle.loader import Oracle
from rms_ref import GMAX, GUARD, RmsRef
from waverange_amd import api

BELOW = -1e30      # the threshold of the cases whose undefined value is UNDEF
UNDEF = -9.99e33   # MSSG's undef
STEP = 2.0 ** -16


def make_field(kind, dims, f32=False):
    """bounded_cases.make_field rounded to multiples of 2^-16"""
    f = bc.make_field(kind, dims)
    q = np.round(f * 65536.0) / 65536.0
    assert np.abs(q).max() < 256.0
    return np.ascontiguousarray(q.astype(np.float32) if f32 else q)


def make_mask(mask, dims):
    """the undefined set, boolean, shaped (nz, ny, nx).  land: about 30 %, coherent -- a half-space, or for "ball" a ball;
    speckle: about 1 %, no two neighbours along x; single: one sample"""
    nx, ny, nz = dims
    n = nx * ny * nz
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    if mask == "land":
        s = 3.0 * x / nx + 2.0 * y / ny + 5.0 * z / nz
        und = s < np.quantile(s, 0.3)
    elif mask == "ball":
        r2 = ((x - 0.45 * nx) / nx) ** 2 + ((y - 0.55 * ny) / ny) ** 2 + ((z - 0.5 * nz) / nz) ** 2
        und = r2 < np.quantile(r2, 0.3)
    elif mask == "speckle":
        und = np.random.default_rng(11 + n).random((nz, ny, nx)) < 0.011
        flat = und.reshape(-1)
        flat[1:] &= ~flat[:-1]
    elif mask == "single":
        und = np.zeros((nz, ny, nx), bool)
        und.reshape(-1)[n // 3] = True
    else:
        raise ValueError(mask)
    return und


class MaskedRef(RmsRef):
    """E_D, S_D*, R_D* of a masked field: RmsRef on f_pad with the differences restricted to D.  E_out(g) is the largest
    |pad - r_g[j]| over the UNDEFINED samples: what a compare that let them in would see."""

    def __init__(self, f, und, seg, wtflag):
        self.und = und
        self.D = ~und.reshape(-1)
        self.nd = int(self.D.sum())
        # the exact sum of the defined samples (integers of at most 42 bits), one division, one rounding for fp32
        total = int(np.round(f.reshape(-1)[self.D].astype(np.float64) * 65536.0).astype(np.int64).sum())
        assert abs(total) < 2 ** 52
        pad = np.float64(total / 65536.0) / np.float64(self.nd)
        self.pad = float(np.float32(pad)) if f.dtype == np.float32 else float(pad)
        f_pad = f.copy()
        f_pad[und] = self.pad
        f_pad.flags.writeable = False
        self.f_pad = f_pad
        super().__init__(BoundedRef(Oracle(), f_pad, seg, wtflag))
        self.whole = RmsRef(self.b)  # the padded field over all n samples: what padding by hand and the plain call would judge
        self._Eout = {}

    def _form(self, g):
        if g not in self._S:
            d = self.f_pad.astype(np.float64).ravel() - self.b.recon(g).astype(np.float64).ravel()
            dd = d[self.D]
            assert np.all(np.isfinite(dd))
            self._S[g] = math.fsum(dd * dd)
            self._E[g] = float(np.abs(dd).max())
            self._Eout[g] = float(np.abs(d[~self.D]).max())

    def E_out(self, g):
        self._form(g)
        return self._Eout[g]

    def R(self, g):
        return math.sqrt(self.S(g) / self.nd)

    # ---- the pointwise norm: the contract of the bounded calls on E_D
    def verdict_max(self, g, m, g_min=0):
        if not g_min <= g <= GMAX:
            return "g = %d outside [%d, %d]" % (g, g_min, GMAX)
        if not self.E(g) <= m:
            return "E_D(%d) = %r exceeds %r" % (g, self.E(g), m)
        if g < GMAX and self.E(g + 1) <= m:
            return "E_D(%d) = %r holds too: %d is not tight" % (g + 1, self.E(g + 1), g)
        return None

    def solve_max(self, m, g_min=0):
        """a g that meets the pointwise contract: the documented walk with E_D in the place of R"""
        self.R = self.E  # (shadows the method for the length of the walk)
        try:
            return self.solve(m, g_min)[0]
        finally:
            del self.__dict__["R"]


# (id, kind, dims, seg, wtflag, f32, format keywords, form, mask, undefined value, below): every driver case of bounded_cases as
# WRS1 from the host -- (39,37,33) and (13,9,7) take the non-fused path, where the trial's copy of the field holds the caller's
# values -- with the masks and the undefined values spread over them; WRS2 and WRS3 once each and fp32 once on (64,64,64); the
# device form once; wtflag = 0 once
CALLS = [
    ("smooth-64x64x64-land-nan", "smooth", (64, 64, 64), 0, 1, False, {}, "host", "land", np.nan, -np.inf),
    ("noise-64x64x64-speckle-undef", "noise", (64, 64, 64), 0, 1, False, {}, "host", "speckle", UNDEF, BELOW),
    ("smooth-16x16x16-single-inf", "smooth", (16, 16, 16), 0, 1, False, {}, "host", "single", np.inf, -np.inf),
    ("noise-16x16x16-ball-nan", "noise", (16, 16, 16), 0, 1, False, {}, "host", "ball", np.nan, -np.inf),
    ("smooth-39x37x33-land-undef", "smooth", (39, 37, 33), 1024, 1, False, {}, "host", "land", UNDEF, BELOW),
    ("noise-39x37x33-speckle-inf-device", "noise", (39, 37, 33), 1024, 1, False, {}, "device", "speckle", np.inf, -np.inf),
    ("smooth-13x9x7-single-nan", "smooth", (13, 9, 7), 1024, 1, False, {}, "host", "single", np.nan, -np.inf),
    ("noise-13x9x7-land-nan", "noise", (13, 9, 7), 1024, 1, False, {}, "host", "land", np.nan, -np.inf),
    ("smooth-64x64x64-land-nan-wrs2", "smooth", (64, 64, 64), 0, 1, False, dict(brick=32), "host", "land", np.nan, -np.inf),
    ("smooth-64x64x64-land-nan-wrs3", "smooth", (64, 64, 64), 0, 1, False, dict(strands=8), "host", "land", np.nan, -np.inf),
    ("smooth-64x64x64-ball-undef-f32", "smooth", (64, 64, 64), 0, 1, True, {}, "host", "ball", UNDEF, BELOW),
    ("smooth-16x16x16-speckle-nan-wt0", "smooth", (16, 16, 16), 0, 0, False, {}, "host", "speckle", np.nan, -np.inf),
]

_REFS, _TARGETS = {}, {}


def key_of(call):
    _, kind, dims, seg, wtflag, f32, _, _, mask, _, _ = call
    return kind, dims, seg, wtflag, f32, mask


def ref_of(kind, dims, seg, wtflag, f32, mask):
    """(the field with its undefined samples still holding defined values, MaskedRef) of a case"""
    key = (kind, dims, seg, wtflag, f32, mask)
    if key not in _REFS:
        f = make_field(kind, dims, f32)
        f.flags.writeable = False
        _REFS[key] = (f, MaskedRef(f, make_mask(mask, dims), seg, wtflag))
    return _REFS[key]


def field_of(call):
    """the caller's field of a case: the undefined value at the undefined samples"""
    f, ref = ref_of(*key_of(call))
    g = f.copy()
    g[ref.und] = call[9]
    return g


def targets_of(kind, dims, seg, wtflag, f32, mask):
    """[(name, norm, target, m)], m the value the error is held against.  Pointwise: the nominal 1e-3 of max|f| (a maximum is
    exact: no guard is needed).  RMS: nominal 1e-3 and 1e-7 of max|f|, moved to the geometric mean of R_D* at the two
    neighbouring grid points the nominal value falls between, so that neither lies within the library's accuracy of the target.
    PSNR: 60 dB, m being the library's own conversion over the range of the defined samples."""
    key = (kind, dims, seg, wtflag, f32, mask)
    if key not in _TARGETS:
        _, ref = ref_of(*key)
        out = [("max 1e-3", api.NORM_MAX, 1e-3 * ref.absmax, 1e-3 * ref.absmax)]
        for name, tol in (("rms 1e-3", 1e-3), ("rms 1e-7", 1e-7)):
            g0, _ = ref.solve(tol * ref.absmax)
            m = math.sqrt(ref.R(g0) * ref.R(g0 + 1)) if g0 < GMAX else tol * ref.absmax
            out.append((name, api.NORM_RMS, m, m))
        out.append(("psnr 60", api.NORM_PSNR, 60.0, api.psnr_rms(60.0, ref.b.flo, ref.b.fhi)))
        _TARGETS[key] = out
    return _TARGETS[key]


def all_inputs():
    seen = set()
    for call in CALLS:
        if key_of(call) not in seen:
            seen.add(key_of(call))
            yield key_of(call)
