"""The inputs of the quality-encode tests, shared by the CPU and the GPU file: the fields of bounded_cases (imported, not edited),
one RmsRef per field and the targets, all taken from the reference (tests/rms_ref.py), made once and never written to.
test_rms_cpu.py holds the reference against the contract and the guard condition for exactly these inputs; test_gpu_quality.py
then holds the library against the reference."""
import math

import bounded_cases as bc
from rms_ref import GMAX, RmsRef
from waverange_amd import api

# (id, kind, dims, seg, wtflag, f32, format keywords, form): every driver case as WRS1 from the host; WRS2 and WRS3 once each on
# (64,64,64); fp32 once; the device-field form once (on the shape whose field has to be copied); wtflag = 0 once on (16,16,16)
CALLS = [("%s-%s-wrs1" % (kind, "x".join(map(str, dims))), kind, dims, seg, 1, False, {}, "host")
         for kind in bc.KINDS for dims, seg in bc.DRIVER_CASES]
CALLS += [("smooth-64x64x64-wrs2", "smooth", (64, 64, 64), 0, 1, False, dict(brick=32), "host"),
          ("smooth-64x64x64-wrs3", "smooth", (64, 64, 64), 0, 1, False, dict(strands=8), "host"),
          ("smooth-64x64x64-f32", "smooth", (64, 64, 64), 0, 1, True, {}, "host"),
          ("noise-39x37x33-device", "noise", (39, 37, 33), 1024, 1, False, {}, "device"),
          ("smooth-16x16x16-wt0", "smooth", bc.WT0_CASE[0], bc.WT0_CASE[1], 0, False, {}, "host")]

_REFS, _TARGETS = {}, {}


def ref_of(kind, dims, seg=0, wtflag=1, f32=False):
    """(field, RmsRef) of a case"""
    key = (kind, dims, seg, wtflag, f32)
    if key not in _REFS:
        f, bref = bc.ref_of(kind, dims, seg, wtflag, f32)
        _REFS[key] = (f, RmsRef(bref))
    return _REFS[key]


def targets_of(kind, dims, seg=0, wtflag=1, f32=False):
    """[(name, norm, target, max_rms)].  The RMS targets at nominal 1e-3 and 1e-7 of max|f| are moved to the geometric mean of
    R* at the two neighbouring grid points the nominal value falls between, so that neither neighbour lies within the
    library's accuracy of the target; a 60 dB PSNR target, max_rms being the library's own conversion; one above max|f|."""
    key = (kind, dims, seg, wtflag, f32)
    if key not in _TARGETS:
        _, ref = ref_of(*key)
        out = []
        for name, tol in (("rms 1e-3", 1e-3), ("rms 1e-7", 1e-7)):
            g0, _ = ref.solve(tol * ref.absmax)
            m = math.sqrt(ref.R(g0) * ref.R(g0 + 1)) if g0 < GMAX else tol * ref.absmax
            out.append((name, api.NORM_RMS, m, m))
        out.append(("psnr 60", api.NORM_PSNR, 60.0, api.psnr_rms(60.0, ref.b.flo, ref.b.fhi)))
        out.append(("above max|f|", api.NORM_RMS, 1.5 * ref.absmax, 1.5 * ref.absmax))
        _TARGETS[key] = out
    return _TARGETS[key]
