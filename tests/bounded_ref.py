"""E(g) of an encode to an error bound (include/waverange_amd.h), in plain Python on top of the CPU oracle: the planes of
BudgetRef at budget_tol(g), the oracle's dequant_accum and inverse transform, and np.abs(f - r).max().  Nothing of the GPU path
is used: the GPU tests take their bounds and their verdicts from here.

For an fp32 field the reconstruction is narrowed to fp32 (the C cast, round to nearest even) and both operands are widened
again before the subtraction.  The same class restates wr_bounded_start as a scan of the grid, and states the contract of the
bounded calls (verdict) so that the CPU test can hold the reference itself against it."""
import numpy as np

from budget_ref import BudgetRef
from waverange_amd import api

GMAX = api.BUDGET_GMAX


def start_scan(max_abs_err, absmax):
    """wr_bounded_start by brute force: the largest g with budget_tol(g) * absmax <= max_abs_err, -1 if there is none or an
    argument is not a positive finite number"""
    m, a = np.float64(max_abs_err), np.float64(absmax)
    if not (m > 0 and a > 0 and np.isfinite(m) and np.isfinite(a)):
        return -1
    best = -1
    for g in range(GMAX + 1):
        if np.float64(api.budget_tol(g)) * a <= m:
            best = g
    return best


class BoundedRef(BudgetRef):
    def __init__(self, oracle, fld, seg=0, wtflag=1):
        self.f32 = fld.dtype == np.float32
        self.f = np.ascontiguousarray(fld)
        self.wtflag = wtflag
        super().__init__(oracle, np.ascontiguousarray(fld, dtype=np.float64), seg, wtflag)
        self.absmax = max(abs(self.flo), abs(self.fhi))
        self._E, self._rec = {}, {}

    def recon(self, g):
        """the reconstruction at budget_tol(g), shaped as the field: float64, or float32 for an fp32 field"""
        if g not in self._rec:
            acc = np.zeros(self.f.size)
            for q, deps, lo in self.planes(g):
                acc = self.o.dequant_accum(acc, q, deps, lo)
            r = acc.reshape(self.shape)
            if self.wtflag:
                r = self.o.cdf97_3d(r, -4)
            self._rec = {g: r.astype(np.float32) if self.f32 else r}  # (one at a time: a (64,64,64) field is 2 MB)
        return self._rec[g]

    def E(self, g):
        if g not in self._E:
            self._E[g] = float(np.abs(self.f.astype(np.float64) - self.recon(g).astype(np.float64)).max())
        return self._E[g]

    def start(self, max_abs_err):
        return start_scan(max_abs_err, self.absmax)

    def verdict(self, g, max_abs_err, g_min=0):
        """None if g meets the contract of the bounded calls for this bound, else what it misses"""
        if not g_min <= g <= GMAX:
            return "g = %d outside [%d, %d]" % (g, g_min, GMAX)
        if not self.E(g) <= max_abs_err:
            return "E(%d) = %r exceeds %r" % (g, self.E(g), max_abs_err)
        if g < GMAX and self.E(g + 1) <= max_abs_err:
            return "E(%d) = %r holds too: %d is not tight" % (g + 1, self.E(g + 1), g)
        return None

    def solve(self, max_abs_err, g_min=0):
        """a g that meets the contract, by a single-step walk from the start point (the reference's own answer: any other g that
        meets the contract is as good); None if E(g_min) exceeds the bound"""
        g = max(self.start(max_abs_err), g_min)
        while self.E(g) > max_abs_err:
            if g == g_min:
                return None
            g -= 1
        while g < GMAX and self.E(g + 1) <= max_abs_err:
            g += 1
        return g
