#!/usr/bin/env python3
"""Write tests/golden/oracle_vs_ref.json: the compiled REFERENCE's outputs (oracle/_ref, strict-IEEE build) on the cases of
tests/oracle_vs_ref_cases.py -- hashes and bit patterns only -- so that tests/test_oracle_vs_ref.py pins the CPU oracle to
the reference where the reference is not built.

    make -C oracle ref && python tools/make_golden_oracle_vs_ref.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_vs_ref_cases as C  # noqa: E402
from oracle.loader import Reference  # noqa: E402


def main():
    ref = Reference()
    G = {"_about": "outputs of the compiled reference (strict IEEE build) on tests/oracle_vs_ref_cases.py; see tools/make_golden_oracle_vs_ref.py",
         "transform": {C.key(s): C.transform(ref, s) for s in C.SHAPES},
         "codec": {C.key(s, t): C.codec(ref, s, t) for s in C.CODEC_SHAPES for t in C.CODEC_TOLS},
         "wtflag0_and_local_cutoff": C.wtflag0_and_local_cutoff(ref),
         "ind_p2w": {C.key(s): C.ind_p2w(ref, s) for s in C.IND_SHAPES}}
    with open(os.path.join(ROOT, "tests", "golden", "oracle_vs_ref.json"), "w") as fh:
        json.dump(G, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
