"""Cases of tests/test_oracle_vs_ref.py: the CPU oracle and the compiled reference on the same synthetic inputs.

Shared by tools/make_golden_oracle_vs_ref.py (which runs the compiled REFERENCE on them and stores what it returns --
SHA-256 of arrays, doubles as hex bit patterns -- in tests/golden/oracle_vs_ref.json) and by the test, which runs the
oracle on them (and the reference too, where oracle/_ref is built) and compares with that record.  `impl` is an
oracle.loader.Oracle or oracle.loader.Reference: both have cdf97_3d / encode / decode / ind_p2w."""
import hashlib

import numpy as np

from waverange_amd import synth

SHAPES = [(64, 64, 64), (13, 9, 7), (37, 21, 13), (33, 5, 1), (2, 2, 2), (3, 3, 3), (17, 1, 1),
          (9, 1, 40), (1, 1, 1), (1, 4, 1), (100, 3, 2)]
CODEC_TOLS = [1e-2, 1e-3, 1e-5, 1e-7, 1e-10, 1e-16]
CODEC_SHAPES = [(32, 32, 32), (37, 21, 13), (60, 50, 40)]
LOCAL_CUTOFF = [1e-3, 1e-5, 1e-4, 1e-6, 1e-3, 1e-3, 1e-5, 1e-4]
IND_SHAPES = [(64, 64, 64), (13, 9, 7), (5, 1, 33), (2, 2, 2)]


def key(shape, tol=None):
    return "x".join("%d" % v for v in shape) + ("" if tol is None else "_tol%g" % tol)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def _hexes(v):
    return [float(x).hex() for x in v]


def transform(impl, shape):
    """forward transform at 1, 2 and 4 levels and the inverse of each, as SHA-256 of the doubles"""
    nx, ny, nz = shape
    f = synth.field(nx, ny, nz, seed=nx * 131 + ny)
    out = {}
    for lvl in (1, 2, 4):
        a = impl.cdf97_3d(f, lvl)
        out["fwd%d" % lvl], out["inv%d" % lvl] = _sha(a), _sha(impl.cdf97_3d(a, -lvl))
    return out


def codec(impl, shape, tol):
    """every output of encoding_wrap (header bit patterns, plane lengths, coded bytes, residual) and the reconstruction"""
    nx, ny, nz = shape
    f = synth.field(nx, ny, nz, seed=99)
    e = impl.encode(f, tol)
    return dict(tolabs=float(e["tolabs"]).hex(), midval=float(e["midval"]).hex(), halfspanval=float(e["halfspanval"]).hex(),
                wlev=int(e["wlev"]), nlay=int(e["nlay"]), ntot_enc=int(e["ntot_enc"]), len_enc_vec=[int(v) for v in e["len_enc_vec"]],
                deps_vec=_hexes(e["deps_vec"]), minval_vec=_hexes(e["minval_vec"]),
                data_sha256=hashlib.sha256(np.ascontiguousarray(e["data"], dtype=np.uint8).tobytes()).hexdigest(),
                residual_sha256=_sha(e["residual"]), decoded_sha256=_sha(impl.decode(e, f.shape)))


def wtflag0_and_local_cutoff(impl):
    """wtflag = 0 (no transform) and the non-uniform cutoff on 2 x 2 x 2 sub-domains"""
    f = synth.field(32, 16, 8, seed=5)
    e0 = impl.encode(f, 1e-4, wtflag=0)
    el = impl.encode(f, None, cutoff=LOCAL_CUTOFF, m=(2, 2, 2))
    return dict(wtflag0=dict(wlev=int(e0["wlev"]), data_sha256=hashlib.sha256(np.ascontiguousarray(e0["data"]).tobytes()).hexdigest()),
                local_cutoff=dict(len_enc_vec=[int(v) for v in el["len_enc_vec"]], deps_vec=_hexes(el["deps_vec"]),
                                  data_sha256=hashlib.sha256(np.ascontiguousarray(el["data"]).tobytes()).hexdigest()))


def ind_p2w(impl, shape):
    """ind_p2w_3d at 4 levels for 100 seeded points of the shape"""
    n1, n2, n3 = shape
    rs = np.random.RandomState(1)
    pts = [(int(rs.randint(n1)), int(rs.randint(n2)), int(rs.randint(n3))) for _ in range(100)]
    return [list(impl.ind_p2w(4, n1, n2, n3, *p)) for p in pts]
