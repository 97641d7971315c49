#!/usr/bin/env python3
"""One field alone, pinned to pinned: the low-resolution decode of a segmented stream against the full decode of it.

  decode_host_seg                     the whole field (the yardstick)
  decode_host_seg_lowres, level 1..4  the box of that level, from all planes (and, with --planes, from the first ones only)

Both on the same stream and the same pinned buffers, interleaved in one process, --reps repetitions after a warm-up round,
medians of the wall time around each call; per level also the call's own stage times (wr_timings: the copies of the needed
streams, the decoder launches, the box dequantiser, the inverse on the box with the scaling, the download), the segments
launched and the payload bytes uploaded (wr_stat).  Level 0 of the low-resolution call is checked equal to the full decode
bit for bit once per stream.

    python tools/lowres_rate.py [--sizes 512,1024] [--tols 1e-3,1e-7] [--reps 5] [--seg 0] [--planes 0]

Prints one JSON object."""
import argparse
import hashlib
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


def digest(a, chunk=1 << 28):
    h = hashlib.blake2b()
    b = a.reshape(-1).view(np.uint8)
    for o in range(0, b.size, chunk):
        h.update(b[o:o + chunk])
    return h.hexdigest()


def run(api, n, tols, reps, seg, planes):
    shape = (n, n, n)
    fld, rec = api.pinned_array(shape), api.pinned_array(shape)
    levels = (1, 2, 3, 4)
    boxes = {r: api.pinned_array(api.lowres_shape(shape, r)) for r in levels}
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
            full_digest = digest(rec)
            rec[:] = 0
            ctx.decode_host_seg_lowres(rec, shape, 0, enc)
            level0_same = digest(rec) == full_digest
            nseg_all = sum((fld.size + s - 1) // s for s in [seg or api.SEG_DEFAULT] * int(enc["nlay"]))
            t_full, tm_full = [], []
            t = {r: [] for r in levels}
            tm = {r: [] for r in levels}
            stat = {}
            for k in range(reps + 1):  # the first round warms up (allocations, code objects, clocks)
                dt, m = timed(ctx.decode_host_seg, rec, enc)
                if k:
                    t_full.append(dt); tm_full.append(m)
                for r in levels:
                    s0, b0 = api.stat(api.STAT_LOWRES_SEGMENTS), api.stat(api.STAT_LOWRES_BYTES_UP)
                    dt, m = timed(ctx.decode_host_seg_lowres, boxes[r], shape, r, enc, planes)
                    stat[r] = (api.stat(api.STAT_LOWRES_SEGMENTS) - s0, api.stat(api.STAT_LOWRES_BYTES_UP) - b0)
                    if k:
                        t[r].append(dt); tm[r].append(m)

            def stages(ms):
                return {"up_ms": med([m["h2d_ms"] for m in ms], 2), "decoder_kernels_ms": med([1e3 * m["rangecoder"] for m in ms], 2),
                        "dequant_ms": med([m["quant_ms"] for m in ms], 2), "inverse_ms": med([m["transform_ms"] for m in ms], 2),
                        "down_ms": med([m["d2h_ms"] for m in ms], 2)}

            row = {"nlay": int(enc["nlay"]), "planes_used": planes or int(enc["nlay"]), "coded_bytes": int(enc["ntot_enc"]),
                   "segments_all_planes": int(nseg_all), "level0_equals_full_decode": level0_same,
                   "full": dict(seconds=med(t_full), **stages(tm_full))}
            for r in levels:
                row["level%d" % r] = dict(seconds=med(t[r]), speedup_vs_full=round(med(t_full) / med(t[r]), 2), box=list(boxes[r].shape),
                                          segments_launched=int(stat[r][0]), payload_bytes_up=int(stat[r][1]), **stages(tm[r]))
            out["%g" % tol] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,1024")
    ap.add_argument("--tols", default="1e-3,1e-7")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seg", type=int, default=0)
    ap.add_argument("--planes", type=int, default=0, help="max_planes of the low-resolution calls (0: all)")
    a = ap.parse_args()
    from waverange_amd import api
    api.set_verbosity(0)
    res = {"seg": a.seg or api.SEG_DEFAULT, "reps": a.reps}
    for n in (int(v) for v in a.sizes.split(",")):
        res["%d^3" % n] = run(api, n, [float(v) for v in a.tols.split(",")], a.reps, a.seg, a.planes)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
