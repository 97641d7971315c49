#!/usr/bin/env python3
"""One segmented decode call on a small field, to be run under a kernel trace: the device work of a driver, call by call.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/seg_driver_trace.py multi|batch

The field is tests/test_gpu_seg_drivers.py's: 64^3, tolerance 1e-6, coded as WRS1 (seg 1008) and as WRS2 (brick 16).  `multi`:
one wr_decode_host_seg_roi_multi call of the region set W on the WRS2 stream; `batch`: one wr_decode_host_seg_batch call of the
two streams.  The two encodes in front of the call are in the trace as well; they are the same in every run."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

from roi_multi_cases import regions_at
from waverange_amd import api, synth


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "multi"
    api.set_verbosity(0)
    shape = (64, 64, 64)
    f = synth.field(64, 64, 64, seed=41)
    with api.Context(0) as ctx:
        encs = []
        for kw in (dict(), dict(brick=16)):
            enc, _ = ctx.encode_host_seg(f, 1e-6, 1, 1008, **kw)
            enc["data"] = enc["data"].copy()
            encs.append(enc)
        if what == "multi":
            out = ctx.decode_host_seg_rois(shape, 0, regions_at("W", 0), encs[1])
            print("multi ok", [o.shape for o in out])
        else:
            outs = [np.empty(shape), np.empty(shape)]
            ctx.decode_host_seg_batch(outs, encs)
            print("batch ok", np.array_equal(outs[0], outs[1]))


if __name__ == "__main__":
    main()
