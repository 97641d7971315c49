"""The inputs of the bounded-encode tests, shared by the CPU and the GPU file: the fields, the bounds (taken from the reference,
tests/bounded_ref.py) and one BoundedRef per field, made once and never written to.  test_bounded_cpu.py holds the reference
against the contract for exactly these inputs; test_gpu_bounded.py then holds the library against the reference."""
import numpy as np

from bounded_ref import BoundedRef
from oracle.loader import Oracle
from waverange_amd import api, synth

KINDS = ["smooth", "noise"]
# (dims as (nx, ny, nz), seg): the default segment with five segments; n < seg; an odd count on the general transform, where the
# field has to be copied before the forward transform overwrites it; the smallest: fewer elements than one tile of the kernel
DRIVER_CASES = [((64, 64, 64), 0), ((16, 16, 16), 0), ((39, 37, 33), 1024), ((13, 9, 7), 1024)]
WT0_CASE = ((16, 16, 16), 0)  # run once without the transform
G_EXACT = api.budget_index(1e-5)  # the grid point whose E is used as a bound
G_ABOVE = 2509  # a grid point at which E of the smooth (64,64,64) field lies 18 % ABOVE nominal: the search has to go finer


def make_field(kind, dims, seed=3):
    """as tests/test_gpu_budget.py makes them"""
    nx, ny, nz = dims
    if kind == "smooth":
        return synth.field(nx, ny, nz, seed=seed)
    idx = np.arange(nx * ny * nz, dtype=np.uint64)
    r = (synth.splitmix64(seed, idx) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    return np.ascontiguousarray((r - 0.25).reshape(nz, ny, nx))


_REFS = {}


def ref_of(kind, dims, seg=0, wtflag=1, f32=False):
    """(field, BoundedRef) of a case"""
    key = (kind, dims, seg, wtflag, f32)
    if key not in _REFS:
        f = make_field(kind, dims)
        if f32:
            f = f.astype(np.float32)
        f.flags.writeable = False
        _REFS[key] = (f, BoundedRef(Oracle(), f, seg, wtflag))
    return _REFS[key]


def bounds_of(ref):
    """[(name, M)]: E of a grid point (equality must count as holding), the double below it, the nominal bounds at 1e-3 and
    1e-7, the nominal bound of G_ABOVE, and one above max|f|"""
    e = ref.E(G_EXACT)
    return [("E(G)", e), ("below E(G)", float(np.nextafter(e, 0.0))), ("1e-3", 1e-3 * ref.absmax), ("1e-7", 1e-7 * ref.absmax),
            ("nominal of G_ABOVE", api.budget_tol(G_ABOVE) * ref.absmax), ("above max|f|", 1.5 * ref.absmax)]
