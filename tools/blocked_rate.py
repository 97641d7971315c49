#!/usr/bin/env python3
"""One field alone, pinned to pinned: the blocked symbol order ("WRS2") against the row-major segmented stream ("WRS1").

  encode_host_seg / decode_host_seg   both formats interleaved, the same field and the same pinned buffers
  decode_host_seg_lowres              levels 1..4 on both streams
  decode_host_seg_roi                 level 0, the centred cubes of 32 and 128 samples on both streams
  plane_reorder                       the reorder kernel alone on one plane of n bytes, both directions, next to
                                      wr_dev_copy_kernel of the same n bytes (device to device) in the same run

All in one process, --reps repetitions after a warm-up round, medians of the wall time around each call; per partial decode
also the segments launched and the payload bytes uploaded (wr_stat).  Coded bytes of both streams are given against the
reference format's (encode_host) for the same field.  Every result on the blocked stream is checked equal, bit for bit, to
the same request on the WRS1 stream once per stream.

    python tools/blocked_rate.py [--sizes 512,1024] [--tols 1e-3,1e-7] [--reps 5] [--seg 0] [--brick 0]

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


def same_bits(a, b):
    return bool(np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)))


def reorder_alone(api, ctx, n, brick, reps):
    """Milliseconds per plane of n^3 bytes: the reorder kernel forward and inverse, and the copy kernel on the same bytes."""
    nb = n ** 3
    src, dst = ctx.alloc(nb), ctx.alloc(nb)
    L = api.lib()
    t = {"reorder_forward_ms": [], "reorder_inverse_ms": [], "copy_kernel_ms": []}
    try:
        api._check(L.wr_dev_copy_kernel(ctx.h, src.ptr, dst.ptr, nb, 2048))  # (touches both buffers once)
        ctx.sync()
        for rep in range(reps + 1):
            for key, inverse in (("reorder_forward_ms", 0), ("reorder_inverse_ms", 1)):
                t0 = time.perf_counter()
                api._check(L.wr_dev_plane_reorder(ctx.h, dst.ptr, src.ptr, n, n, n, 4, brick, inverse))  # (returns when the kernel is done)
                if rep:
                    t[key].append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            api._check(L.wr_dev_copy_kernel(ctx.h, dst.ptr, src.ptr, nb, 2048))
            ctx.sync()
            if rep:
                t["copy_kernel_ms"].append(1e3 * (time.perf_counter() - t0))
    finally:
        src.free()
        dst.free()
    out = {k: med(v, 3) for k, v in t.items()}
    out["plane_bytes"] = nb
    out["forward_over_copy"] = round(out["reorder_forward_ms"] / out["copy_kernel_ms"], 2)
    out["inverse_over_copy"] = round(out["reorder_inverse_ms"] / out["copy_kernel_ms"], 2)
    return out


def run(api, n, tols, reps, seg, brick):
    shape = (n, n, n)
    fld, rec1, rec2 = api.pinned_array(shape), api.pinned_array(shape), api.pinned_array(shape)
    cubes = {"cube%d" % e: ((n // 2 - e // 2, n // 2 + e // 2),) * 3 for e in (32, 128)}
    out = {}
    with api.Context(0) as ctx:
        buf = ctx.alloc(fld.nbytes)
        ctx.synth_field(buf, n, n, n, 2024)
        fld.reshape(-1)[:] = buf.download(np.float64, fld.size)
        buf.free()
        out["reorder_kernel"] = reorder_alone(api, ctx, n, brick, reps)
        coded = [api.pinned_array((ctx._seg_cap(shape, seg, brick),), np.uint8) for _ in range(2)]
        for tol in tols:
            ref, _ = ctx.encode_host(fld, tol)
            ref_bytes = int(ref["ntot_enc"])
            del ref
            kw = (dict(), dict(brick=brick))  # WRS1, WRS2
            enc = [None, None]
            t_enc, t_dec = ([], []), ([], [])
            for rep in range(reps + 1):  # the first round warms up (allocations, code objects, clocks)
                for k in (0, 1):
                    dt, (e, _) = timed(ctx.encode_host_seg, fld, tol, 1, seg, out=coded[k], **kw[k])
                    enc[k] = e
                    if rep:
                        t_enc[k].append(dt)
                    dt, _ = timed(ctx.decode_host_seg, rec2 if k else rec1, e)
                    if rep:
                        t_dec[k].append(dt)
            row = {"nlay": int(enc[0]["nlay"]), "reference_format_bytes": ref_bytes, "full_decode_same_bits": same_bits(rec1, rec2)}
            for k, name in enumerate(("wrs1", "blocked")):
                row[name] = {"coded_bytes": int(enc[k]["ntot_enc"]), "over_reference_format": round(int(enc[k]["ntot_enc"]) / ref_bytes, 4),
                             "encode_s": med(t_enc[k]), "decode_s": med(t_dec[k]), "round_trip_s": round(med(t_enc[k]) + med(t_dec[k]), 4)}
            row["blocked_round_trip_over_wrs1"] = round(row["blocked"]["round_trip_s"] / row["wrs1"]["round_trip_s"], 4)
            # partial decodes: the same request on both streams, interleaved
            requests = [("lowres%d" % r, ("lowres", r)) for r in range(1, 5)] + [(k, ("roi", v)) for k, v in cubes.items()]
            for name, (kind, arg) in requests:
                if kind == "lowres":
                    outs = [api.pinned_array(api.lowres_shape(shape, arg)) for _ in range(2)]
                    call = lambda k: ctx.decode_host_seg_lowres(outs[k], shape, arg, enc[k])  # noqa: E731
                    stats = (api.STAT_LOWRES_SEGMENTS, api.STAT_LOWRES_BYTES_UP)
                else:
                    outs = [api.pinned_array(api.roi_shape(arg)) for _ in range(2)]
                    call = lambda k: ctx.decode_host_seg_roi(outs[k], shape, 0, arg, enc[k])  # noqa: E731
                    stats = (api.STAT_ROI_SEGMENTS, api.STAT_ROI_BYTES_UP)
                t, st = ([], []), [None, None]
                for rep in range(reps + 1):
                    for k in (0, 1):
                        s0 = [api.stat(s) for s in stats]
                        dt, _ = timed(call, k)
                        st[k] = [api.stat(s) - a for s, a in zip(stats, s0)]
                        if rep:
                            t[k].append(dt)
                row[name] = {"same_bits": same_bits(outs[0], outs[1]),
                             "wrs1": {"seconds": med(t[0]), "segments_launched": int(st[0][0]), "payload_bytes_up": int(st[0][1])},
                             "blocked": {"seconds": med(t[1]), "segments_launched": int(st[1][0]), "payload_bytes_up": int(st[1][1])},
                             "blocked_over_wrs1": round(med(t[1]) / med(t[0]), 3)}
            out["%g" % tol] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,1024")
    ap.add_argument("--tols", default="1e-3,1e-7")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seg", type=int, default=0)
    ap.add_argument("--brick", type=int, default=0)
    a = ap.parse_args()
    from waverange_amd import api
    api.set_verbosity(0)
    res = {"seg": a.seg or api.SEG_DEFAULT, "brick": a.brick or api.BRICK_DEFAULT, "reps": a.reps}
    for n in (int(v) for v in a.sizes.split(",")):
        res["%d^3" % n] = run(api, n, [float(v) for v in a.tols.split(",")], a.reps, a.seg, a.brick)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
