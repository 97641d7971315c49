"""The fp64 edge-value fields of tests/fused_cases.py belong in the GPU tests only if the reference's behaviour on them is
defined: every field goes through the CPU oracle and, where oracle/_ref is built, through the compiled reference, which
must give the same header scalars, the same bytes and the same reconstruction, all finite.  CPU only."""
import numpy as np
import pytest

import fused_cases as F
from util import bits_equal

HEADER = ("tolabs", "midval", "halfspanval", "wlev", "nlay", "ntot_enc", "len_enc_vec")


@pytest.fixture(scope="module")
def live_reference():
    from oracle.loader import Reference, have_ref
    return Reference() if have_ref() else None


def test_the_fields_that_must_be_there_are():
    assert "below" in F.EDGE_FIELDS and "scaled_1e300" in F.EDGE_FIELDS and {"above", "x10"} & set(F.EDGE_FIELDS)
    assert set(F.SUBNORMAL_FIELDS) <= set(F.EDGE_FIELDS)
    assert len(F.EDGE_SHAPES) == 4


@pytest.mark.parametrize("name", F.EDGE_FIELDS)
@pytest.mark.parametrize("shape", sorted(F.EDGE_SHAPES), ids=F.ident)
def test_edge_field_is_defined_in_the_reference(oracle, live_reference, shape, name, capfd):
    f = F.edge_field(shape, name)
    F.check_edge_input(f, name)
    want = oracle.encode(f, F.EDGE_TOL)
    rec = oracle.decode(want, f.shape)
    assert all(np.isfinite(want[k]) for k in ("tolabs", "midval", "halfspanval"))
    assert np.isfinite(want["deps_vec"]).all() and np.isfinite(want["minval_vec"]).all() and np.isfinite(rec).all()
    if name == "below":
        # trivial by the reference's rule (halfspanval <= 2 DBL_MIN): nothing is coded, the decode is the constant midval
        assert (want["nlay"], want["ntot_enc"]) == (0, 0)
        assert 0 < want["halfspanval"] <= 2 * F.TINY and 0 < abs(want["midval"]) < F.TINY
        assert bits_equal(rec, np.full(f.shape, want["midval"]))
    else:
        assert want["nlay"] >= 1 and want["ntot_enc"] > 0 and want["halfspanval"] > 2 * F.TINY
    if name in F.SUBNORMAL_FIELDS and name != "below":
        assert want["nlay"] == 8, "a field of subnormals runs out of planes before it meets the tolerance"
    if live_reference is not None:
        ref = live_reference.encode(f, F.EDGE_TOL)
        for k in HEADER:
            assert ref[k] == want[k], k
        assert bits_equal(ref["deps_vec"], want["deps_vec"]) and bits_equal(ref["minval_vec"], want["minval_vec"])
        assert np.array_equal(ref["data"], want["data"])
        assert bits_equal(ref["residual"], want["residual"])
        assert bits_equal(live_reference.decode(ref, f.shape), rec)
