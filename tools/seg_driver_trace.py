#!/usr/bin/env python3
"""One segmented call on a small field, to be run under a kernel trace: the device work of a driver, call by call.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/seg_driver_trace.py MODE

The field is tests/test_gpu_seg_drivers.py's: 64^3, tolerance 1e-6, seg 1008.  The decode modes code it as WRS1 and as WRS2
(brick 16) first; those two encodes are in the trace as well, the same in every run.
    multi          one wr_decode_host_seg_roi_multi call of the region set W on the WRS2 stream
    batch          one wr_decode_host_seg_batch call of the two streams
    encode         one WRS2 (brick 16) and one WRS3 (8 strands) encode, nothing else
    encode_batch   one wr_encode_host_seg_batch call of two fields as WRS2, nothing else
    transcode      the reference's stream of the field (one wr_encode_host), then reference -> WRS3 and WRS2 -> reference
The masked modes code the field with a disc of undefined samples as one masked WRS1 record first (mask cut at seg 1008 too):
    masked_whole   one wr_decode_host_seg_masked call
    masked_region  one wr_decode_host_seg_roi_masked call of a centred 32^3 box at level 0
    masked_batch   one wr_decode_host_seg_roi_batch_masked call of two such records and that box"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

from roi_multi_cases import regions_at
from waverange_amd import api, synth

TOL, SEG = 1e-6, 1008


def own(enc):
    enc["data"] = enc["data"].copy()
    return enc


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "multi"
    api.set_verbosity(0)
    shape = (64, 64, 64)
    f = synth.field(64, 64, 64, seed=41)
    with api.Context(0) as ctx:
        if what == "encode":
            a, _ = ctx.encode_host_seg(f, TOL, 1, SEG, brick=16)
            b, _ = ctx.encode_host_seg(f, TOL, 1, SEG, strands=8)
            print("encode ok", a["ntot_enc"], b["ntot_enc"])
            return
        if what == "encode_batch":
            encs, _ = ctx.encode_host_seg_batch([f, synth.field(64, 64, 64, seed=7)], TOL, 1, SEG, brick=16)
            print("encode_batch ok", [e["ntot_enc"] for e in encs])
            return
        if what == "transcode":
            ref = own(ctx.encode_host(f, TOL)[0])
            wrs3, _ = ctx.transcode(ref, ref["data"], "wrs3:seg=1008:strands=8", shape=shape)
            wrs2, info2 = api.transcode_host_ref(shape, ref, ref["data"], "wrs2:seg=1008:brick=16")  # (on the host: no kernel)
            back, _ = ctx.transcode(info2, wrs2, "ref", shape=shape)
            print("transcode ok", wrs3.size, back.tobytes() == ref["data"].tobytes())
            return
        if what.startswith("masked_"):
            z, y, x = np.meshgrid(np.arange(64), np.arange(64), np.arange(64), indexing="ij")
            f[(x - 30) ** 2 + (y - 34) ** 2 < 300] = -9.99e33
            rec = own(ctx.encode_host_seg_masked(f, TOL, -1e30, seg=SEG)[0])
            box = ((16, 48), (16, 48), (16, 48))
            if what == "masked_whole":
                res, _ = ctx.decode_host_seg_masked(np.empty(shape), rec)
            elif what == "masked_region":
                res, _ = ctx.decode_host_seg_roi_masked(np.empty(api.roi_shape(box)), shape, 0, box, rec)
            else:
                masks = []
                ctx.decode_host_seg_rois_batch_masked(shape, 0, [box], [rec, rec], masks=masks)
                res = masks[1]
            print(what, "ok", res["undefined"], res["mask_len"])
            return
        encs = [own(ctx.encode_host_seg(f, TOL, 1, SEG, **kw)[0]) for kw in (dict(), dict(brick=16))]
        if what == "multi":
            out = ctx.decode_host_seg_rois(shape, 0, regions_at("W", 0), encs[1])
            print("multi ok", [o.shape for o in out])
        else:
            outs = [np.empty(shape), np.empty(shape)]
            ctx.decode_host_seg_batch(outs, encs)
            print("batch ok", np.array_equal(outs[0], outs[1]))


if __name__ == "__main__":
    main()
