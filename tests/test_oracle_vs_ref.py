"""The CPU oracle against the reference itself: against the reference's outputs stored in tests/golden/oracle_vs_ref.json
(tools/make_golden_oracle_vs_ref.py, from oracle/_ref built by oracle/Makefile) and, where oracle/_ref is built, against
the reference run on the same inputs.  CPU only."""
import json
import os

import pytest

import oracle_vs_ref_cases as C
from util import GOLDEN


@pytest.fixture(scope="module")
def stored():
    with open(os.path.join(GOLDEN, "oracle_vs_ref.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def live_reference():
    from oracle.loader import Reference, have_ref
    return Reference() if have_ref() else None


def check(case, want, oracle, reference, *args):
    """the oracle's outputs equal the reference's stored ones -- and the reference, where it is built, still gives them"""
    if reference is not None:
        assert case(reference, *args) == want, "tests/golden/oracle_vs_ref.json is not what the reference gives (tools/make_golden_oracle_vs_ref.py)"
    assert case(oracle, *args) == want


@pytest.mark.parametrize("shape", C.SHAPES)
def test_transform_matches_reference(oracle, live_reference, stored, shape):
    check(C.transform, stored["transform"][C.key(shape)], oracle, live_reference, shape)


@pytest.mark.parametrize("tol", C.CODEC_TOLS)
@pytest.mark.parametrize("shape", C.CODEC_SHAPES)
def test_codec_matches_reference(oracle, live_reference, stored, shape, tol, capfd):
    check(C.codec, stored["codec"][C.key(shape, tol)], oracle, live_reference, shape, tol)


def test_wtflag0_and_local_cutoff_match_reference(oracle, live_reference, stored, capfd):
    want = stored["wtflag0_and_local_cutoff"]
    assert want["wtflag0"]["wlev"] == 0
    check(C.wtflag0_and_local_cutoff, want, oracle, live_reference)


def test_ind_p2w_matches_reference(oracle, live_reference, stored):
    for shape in C.IND_SHAPES:
        check(C.ind_p2w, stored["ind_p2w"][C.key(shape)], oracle, live_reference, shape)
