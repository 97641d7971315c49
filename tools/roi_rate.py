#!/usr/bin/env python3
"""One field alone, pinned to pinned: the region decode of a segmented stream against the full decode of it.

  decode_host_seg       the whole field (the yardstick)
  decode_host_seg_roi   level 0, all planes: centred cubes of 32, 64, 128 and 256 samples and one z-plane

Both on the same stream and the same pinned buffers, interleaved in one process, --reps repetitions after a warm-up round,
medians of the wall time around each call; per region also the call's own stage times (wr_timings: the copies of the needed
streams, the decoder launches, the window dequantiser, the inverse on the window with the crop, the download), the window,
the segments launched and the payload bytes uploaded (wr_stat).  Every region is checked equal to the crop of the full
decode bit for bit once per stream.

    python tools/roi_rate.py [--sizes 512,1024] [--tols 1e-3,1e-7] [--reps 5] [--seg 0]

Prints one JSON object."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, *a, **k):
    t0 = time.perf_counter()
    r = fn(*a, **k)
    return time.perf_counter() - t0, r


def med(v, digits=4):
    return round(float(np.median(v)), digits)


def regions(n):
    out = {}
    for e in (32, 64, 128, 256):
        if e < n:
            out["cube%d" % e] = ((n // 2 - e // 2, n // 2 + e // 2),) * 3
    z = 500 * n // 1024
    out["zplane"] = ((z, z + 1), (0, n), (0, n))
    return out


def run(api, n, tols, reps, seg):
    shape = (n, n, n)
    fld, rec = api.pinned_array(shape), api.pinned_array(shape)
    rois = regions(n)
    outs = {k: api.pinned_array(api.roi_shape(r)) for k, r in rois.items()}
    out = {}
    with api.Context(0) as ctx:
        buf = ctx.alloc(fld.nbytes)
        ctx.synth_field(buf, n, n, n, 2024)
        fld.reshape(-1)[:] = buf.download(np.float64, fld.size)
        buf.free()
        coded = api.pinned_array((ctx._seg_cap(shape, seg),), np.uint8)
        for tol in tols:
            enc, _ = ctx.encode_host_seg(fld, tol, 1, seg, out=coded)
            ctx.decode_host_seg(rec, enc)
            same = {}
            for k, r in rois.items():
                outs[k][:] = 0
                ctx.decode_host_seg_roi(outs[k], shape, 0, r, enc)
                want = np.ascontiguousarray(rec[tuple(slice(lo, hi) for lo, hi in r)])
                same[k] = bool(np.array_equal(outs[k].view(np.uint64), want.view(np.uint64)))
            nseg_all = ((fld.size + (seg or api.SEG_DEFAULT) - 1) // (seg or api.SEG_DEFAULT)) * int(enc["nlay"])
            t_full, tm_full = [], []
            t = {k: [] for k in rois}
            tm = {k: [] for k in rois}
            stat = {}
            for rep in range(reps + 1):  # the first round warms up (allocations, code objects, clocks)
                dt, m = timed(ctx.decode_host_seg, rec, enc)
                if rep:
                    t_full.append(dt); tm_full.append(m)
                for k, r in rois.items():
                    s0, b0 = api.stat(api.STAT_ROI_SEGMENTS), api.stat(api.STAT_ROI_BYTES_UP)
                    dt, m = timed(ctx.decode_host_seg_roi, outs[k], shape, 0, r, enc)
                    stat[k] = (api.stat(api.STAT_ROI_SEGMENTS) - s0, api.stat(api.STAT_ROI_BYTES_UP) - b0)
                    if rep:
                        t[k].append(dt); tm[k].append(m)

            def stages(ms):
                return {"up_ms": med([m["h2d_ms"] for m in ms], 2), "decoder_kernels_ms": med([1e3 * m["rangecoder"] for m in ms], 2),
                        "dequant_ms": med([m["quant_ms"] for m in ms], 2), "inverse_ms": med([m["transform_ms"] for m in ms], 2),
                        "down_ms": med([m["d2h_ms"] for m in ms], 2)}

            row = {"nlay": int(enc["nlay"]), "coded_bytes": int(enc["ntot_enc"]), "segments_all_planes": int(nseg_all),
                   "full": dict(seconds=med(t_full), **stages(tm_full))}
            for k, r in rois.items():
                win = api.roi_window(shape, 0, r)
                row[k] = dict(seconds=med(t[k]), speedup_vs_full=round(med(t_full) / med(t[k]), 2), region=[list(v) for v in r],
                              window=[list(v) for v in win], fused_inverse=bool(api.fused_plan(tuple(b - a for a, b in win), True)["used"]),
                              equals_crop_of_full_decode=same[k], segments_launched=int(stat[k][0]), payload_bytes_up=int(stat[k][1]),
                              **stages(tm[k]))
            out["%g" % tol] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,1024")
    ap.add_argument("--tols", default="1e-3,1e-7")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seg", type=int, default=0)
    a = ap.parse_args()
    from waverange_amd import api
    api.set_verbosity(0)
    res = {"seg": a.seg or api.SEG_DEFAULT, "reps": a.reps}
    for n in (int(v) for v in a.sizes.split(",")):
        res["%d^3" % n] = run(api, n, [float(v) for v in a.tols.split(",")], a.reps, a.seg)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
