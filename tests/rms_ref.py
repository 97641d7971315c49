"""S*(g) and R*(g) of an encode to an RMS or PSNR target (include/waverange_amd.h), in plain Python on top of
bounded_ref.BoundedRef.recon(g): d = the fp64 difference array, S* = math.fsum(d * d) -- numpy rounds every product once and fsum
returns the correctly rounded sum of those doubles, so S* is the real sum of the rounded squares to half an ulp -- and
R* = sqrt(S* / n).  Nothing of the GPU path is used: the GPU tests take their targets and their verdicts from here.

verdict states the contract of the quality calls; solve is the reference's own answer, found by the walk the library documents
(csrc/wr_budget.h: bounded_walk, restated here) so that on inputs that pass the guard of test_rms_cpu.py both end on the same
grid point."""
import math

import numpy as np

from bounded_ref import start_scan
from waverange_amd import api

GMAX = api.BUDGET_GMAX
ACCURACY = 2.0 ** -36  # |S - S*| <= ACCURACY * S*: the library's stated accuracy
GUARD = 2.0 ** -30     # a target must stay this far, relatively, from R* at the reference's g and g + 1


class RmsRef:
    def __init__(self, bounded_ref):
        self.b = bounded_ref
        self.n = bounded_ref.f.size
        self.absmax = bounded_ref.absmax
        self.range = bounded_ref.fhi - bounded_ref.flo
        self._S, self._E = {}, {}

    def _form(self, g):
        if g not in self._S:
            d = self.b.f.astype(np.float64).ravel() - self.b.recon(g).astype(np.float64).ravel()
            d = d[np.isfinite(d)]
            self._S[g] = math.fsum(d * d)
            self._E[g] = float(np.abs(d).max()) if d.size else 0.0

    def S(self, g):
        self._form(g)
        return self._S[g]

    def E(self, g):
        self._form(g)
        return self._E[g]

    def R(self, g):
        return math.sqrt(self.S(g) / self.n)

    def nlay(self, g):
        return self.b.nlay(g)

    def recon(self, g):
        return self.b.recon(g)

    def start(self, max_rms):
        return start_scan(max_rms, self.absmax)

    def verdict(self, g, max_rms, g_min=0):
        """None if g meets the contract of the quality calls for this RMS target, else what it misses"""
        if not g_min <= g <= GMAX:
            return "g = %d outside [%d, %d]" % (g, g_min, GMAX)
        if not self.R(g) <= max_rms:
            return "R(%d) = %r exceeds %r" % (g, self.R(g), max_rms)
        if g < GMAX and self.R(g + 1) <= max_rms:
            return "R(%d) = %r holds too: %d is not tight" % (g + 1, self.R(g + 1), g)
        return None

    def guarded(self, g, max_rms):
        """the guard condition at g and g + 1: R* is further from the target than the library's accuracy can bridge"""
        pts = [g] + ([g + 1] if g < GMAX else [])
        return all(abs(self.R(k) - max_rms) > GUARD * max_rms for k in pts)

    def solve(self, max_rms, g_min=0):
        """(g, trials) by the documented walk from the start point; (None, trials) if R(g_min) exceeds the target"""
        asked = set()

        def R(g):
            asked.add(g)
            return self.R(g)

        def points(r):
            d = 48.0 * math.log2(r) if r > 0 else 0.0
            return GMAX if d >= GMAX else int(d) if d > 0 else 0

        at = min(max(self.start(max_rms), g_min), GMAX)
        cur, step = R(at), 0
        while not cur <= max_rms:
            if at == g_min:
                return None, len(asked)
            step = max(points(cur / max_rms), 2 * step, 1)
            at = max(at - step, g_min)
            cur = R(at)
        step = 0
        while at < GMAX:
            step = max(points(max_rms / cur) if cur > 0 else GMAX, 2 * step, 1)
            far = min(at + step, GMAX)
            if R(far) <= max_rms:
                at, cur = far, R(far)
                continue
            good, bad = at, far
            while bad - good > 1:
                mid = good + (bad - good) // 2
                if R(mid) <= max_rms:
                    good = mid
                else:
                    bad = mid
            at = good
            break
        return at, len(asked)
