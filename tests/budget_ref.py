"""B(g) of an encode to a byte budget (include/waverange_amd.h), in plain Python on top of the CPU oracle: the oracle's transform,
wro_quantize_plane through oracle/loader.py, the quantizer loop's scalar steps restated here, and the host size bound
(api.seg_size_bound_host_ref).  Nothing of the GPU path is used: the GPU tests take their budgets and their verdicts from here.

Only the last plane depends on the tolerance, so the full planes are made once and every B(g) costs one quantization."""
import numpy as np

from waverange_amd import api

NLAYMAX = 8
WAV_ACC_COEF = 1.75


class BudgetRef:
    def __init__(self, oracle, fld, seg=0, wtflag=1):
        self.o, self.seg = oracle, seg
        fld = np.ascontiguousarray(fld, dtype=np.float64)
        self.shape = fld.shape
        self.flo, self.fhi = oracle.minmax(fld)
        self.constant = (self.fhi - self.flo) / 2 <= 2 * np.finfo(np.float64).tiny
        self.resid = [(oracle.cdf97_3d(fld, 4) if wtflag else fld.copy()).ravel()]  # resid[l]: what plane l is cut from
        self.range = [oracle.minmax(self.resid[0])]
        self.full = []  # full[l]: (symbols, bound) of plane l cut with its full step
        self._B = {}

    def tolabs(self, g):
        t = api.budget_tol(g) * max(abs(self.flo), abs(self.fhi))
        return t / WAV_ACC_COEF

    def _full_plane(self, l):
        while len(self.full) <= l:
            k = len(self.full)
            lo, hi = self.range[k]
            q, r = self.o.quantize_plane(self.resid[k], (hi - lo) / 255.0, lo)
            self.full.append((q, api.seg_size_bound_host_ref(q, self.seg)))
            self.resid.append(r)
            self.range.append(self.o.minmax(r))
        return self.full[l]

    def planes(self, g):
        """[(symbols, deps, minval)] of the planes the quantizer loop produces at budget_tol(g)"""
        if self.constant:
            return []
        tol, out = self.tolabs(g), []
        for l in range(NLAYMAX):
            lo, hi = self.range[l]
            deps = (hi - lo) / 255.0
            last = deps < tol
            if last:
                deps = tol
            if l >= NLAYMAX - 1:
                last = True
            if last:
                out.append((self.o.quantize_plane(self.resid[l], deps, lo)[0], deps, lo))
                return out
            out.append((self._full_plane(l)[0], deps, lo))

    def nlay(self, g):
        """the number of planes at budget_tol(g), without quantizing the last one"""
        if self.constant:
            return 0
        tol = self.tolabs(g)
        for l in range(NLAYMAX):
            lo, hi = self.range[l]
            if (hi - lo) / 255.0 < tol or l >= NLAYMAX - 1:
                return l + 1
            self._full_plane(l)

    def B(self, g):
        if g not in self._B:
            ps = self.planes(g)
            self._B[g] = sum(self._full_plane(l)[1] for l in range(len(ps) - 1)) + (api.seg_size_bound_host_ref(ps[-1][0], self.seg) if ps else 0)
        return self._B[g]

    def last_interval(self, l, g_min=0):
        """(a, b): the grid points of [g_min, BUDGET_GMAX] at which plane l is the last one (nlay == l + 1); None if there are none"""
        a, b = self._first_with(l + 1, g_min), self._first_with(l, g_min) - 1
        return (a, b) if a <= b else None

    def _first_with(self, most, g_min):
        """the smallest g in [g_min, BUDGET_GMAX] with nlay(g) <= most (nlay does not grow with g); BUDGET_GMAX + 1 if there is none"""
        if self.nlay(api.BUDGET_GMAX) > most:
            return api.BUDGET_GMAX + 1
        lo, hi = g_min - 1, api.BUDGET_GMAX
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if self.nlay(mid) <= most:
                hi = mid
            else:
                lo = mid
        return hi
