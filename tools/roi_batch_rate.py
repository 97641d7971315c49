#!/usr/bin/env python3
"""The same regions of N coded fields: one batch call against a loop of N many-region calls.

  wr_decode_host_seg_roi_multi  x N   one call per field (the yardstick of the batch row of the same run)
  wr_decode_host_seg_roi_batch        the N fields in one call: at most two coder launches

Fields: N coded fields of n^3 (the same synthetic field coded once per format and tolerance and handed in N times: the coder's
time is one segment's chain whatever the symbols are, and every field still has its own planes, blobs and windows on the
device).  Formats WRS1, WRS2 (brick 32), WRS3 (K = 8).  Regions: one centred probe of 32^3, eight probes, the centre z-plane,
the whole box of level 2.  Both ways on pinned buffers in one process, interleaved inside every repetition; --reps repetitions
after a warm-up round in which every region of every field of the batch call is compared bit for bit with the loop's.  Medians
of the wall time around the call (the loop: around all N calls) and of the calls' own stage times (wr_timings, summed over
the loop's calls), with the payload bytes uploaded and the coder launches (wr_stat).  A configuration whose batch does not fit
api.seg_roi_batch_device_bytes into the device's free memory as ONE call is recorded as skipped.

    python tools/roi_batch_rate.py [--sizes 256,512] [--ns 1,8,64] [--tols 1e-3,1e-7] [--formats wrs1,wrs2,wrs3]
                                   [--regions probe,probes8,zplane,level2] [--reps 5] [--out FILE]

Prints one JSON object (and writes it to FILE)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMATS = {"wrs1": dict(), "wrs2": dict(brick=32), "wrs3": dict(strands=8)}


def med(v, digits=4):
    return round(float(np.median(v)), digits)


def regions(n, which, edge=32):
    """(level, rois) in the coordinates of the box of that level"""
    c = (n - edge) // 2
    if which == "probe":
        return 0, [((c, c + edge),) * 3]
    if which == "probes8":
        q = n // 4
        return 0, [tuple((a + (q - edge) // 2, a + (q - edge) // 2 + edge) for a in (z, y, x)) for z in (q, 2 * q) for y in (q, 2 * q) for x in (q, 2 * q)]
    if which == "zplane":
        return 0, [((n // 2, n // 2 + 1), (0, n), (0, n))]
    if which == "level2":
        return 2, [((0, n // 4),) * 3]
    raise ValueError(which)


def counters(api):
    return np.array([api.stat(api.STAT_ROI_SEGMENTS), api.stat(api.STAT_ROI_BYTES_UP), api.stat(api.STAT_ROI_CODER_LAUNCHES)], dtype=np.int64)


def stages(ms):
    """the stage times of one repetition in ms, summed over its calls"""
    return dict(up_ms=sum(m["h2d_ms"] for m in ms), coder_ms=sum(1e3 * m["rangecoder"] for m in ms),
                window_stage_ms=sum(m["quant_ms"] + m["transform_ms"] for m in ms), down_ms=sum(m["d2h_ms"] for m in ms))


def row(walls, tms, stat):
    out = dict(seconds=med(walls), payload_bytes_up=int(stat[1]), coder_launches=int(stat[2]), segments_launched=int(stat[0]))
    for k in ("up_ms", "coder_ms", "window_stage_ms", "down_ms"):
        out[k] = med([t[k] for t in tms], 2)
    return out


def run(api, n, ns, tols, formats, which, reps):
    shape = (n, n, n)
    fld = api.pinned_array(shape)
    out = {}
    with api.Context(0) as ctx:
        buf = ctx.alloc(fld.nbytes)
        ctx.synth_field(buf, n, n, n, 2024)
        fld.reshape(-1)[:] = buf.download(np.float64, fld.size)
        buf.free()
        multi = api.lib().wr_decode_host_seg_roi_multi
        for tol in tols:
            for fmt in formats:
                kw = FORMATS[fmt]
                coded = api.pinned_array((ctx._seg_cap(shape, 0, kw.get("brick"), kw.get("strands")),), np.uint8)
                enc, _ = ctx.encode_host_seg(fld, tol, 1, 0, out=coded, **kw)
                nlay = int(enc["nlay"])
                for name in which:
                    level, rois = regions(n, name)
                    T = int(api.roi_multi_offsets(shape, level, rois)[-1])
                    for N in ns:
                        key = "%d^3 tol=%g %s %s N=%d" % (n, tol, fmt, name, N)
                        need = api.seg_roi_batch_device_bytes(N, n ** 3, nlay, 0, kw.get("brick", 0), kw.get("strands", 0), T)
                        free = ctx.device_free_bytes()
                        if not need or need > free:
                            out[key] = dict(skipped="the batch needs %d bytes by the sizing function (0: over the job limit), %d are free" % (need, free))
                            continue
                        one_out, all_out = api.pinned_array((N * T,)), api.pinned_array((N * T,))
                        t = {"loop": [], "batch": []}
                        tm = {"loop": [], "batch": []}
                        stat, same = {}, True
                        for rep in range(reps + 1):  # the first round warms up and checks the values
                            c0 = counters(api)
                            ms, dt = [], 0.0
                            for f in range(N):
                                t0 = time.perf_counter()
                                ms.append(ctx._decode_seg_rois(multi, one_out[f * T:].ctypes.data, shape, level, rois, enc, 0))
                                dt += time.perf_counter() - t0
                            stat["loop"] = counters(api) - c0
                            if rep:
                                t["loop"].append(dt); tm["loop"].append(stages(ms))
                            c0 = counters(api)
                            m = {}
                            t0 = time.perf_counter()
                            ctx.decode_host_seg_rois_batch(shape, level, rois, [enc] * N, 0, timings=m, out=all_out)
                            dt = time.perf_counter() - t0
                            stat["batch"] = counters(api) - c0
                            if rep:
                                t["batch"].append(dt); tm["batch"].append(stages([m]))
                            else:
                                same = bool(np.array_equal(one_out.view(np.uint64), all_out.view(np.uint64)))
                        rec = dict(nlay=nlay, fields=N, out_elems_per_field=T, sized_bytes=need, loop=row(t["loop"], tm["loop"], stat["loop"]),
                                   batch=row(t["batch"], tm["batch"], stat["batch"]), every_field_equals_the_loop=same)
                        b, l = rec["batch"], rec["loop"]
                        rec["batch"]["speedup_vs_loop_wall"] = round(l["seconds"] / b["seconds"], 2) if b["seconds"] else None
                        rec["batch"]["speedup_vs_loop_coder"] = round(l["coder_ms"] / b["coder_ms"], 2) if b["coder_ms"] else None
                        rec["batch"]["window_stage_share_of_wall"] = round(b["window_stage_ms"] / (1e3 * b["seconds"]), 3) if b["seconds"] else None
                        out[key] = rec
                        print(key, "loop %.3f s, batch %.3f s" % (l["seconds"], b["seconds"]), file=sys.stderr, flush=True)
                        del one_out, all_out
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--ns", default="1,8,64")
    ap.add_argument("--tols", default="1e-3,1e-7")
    ap.add_argument("--formats", default="wrs1,wrs2,wrs3")
    ap.add_argument("--regions", default="probe,probes8,zplane,level2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from waverange_amd import api
    api.set_verbosity(0)
    res = {"reps": a.reps, "seg": api.SEG_DEFAULT, "rows": {}}
    for n in (int(v) for v in a.sizes.split(",")):
        res["rows"].update(run(api, n, [int(v) for v in a.ns.split(",")], [float(v) for v in a.tols.split(",")], a.formats.split(","), a.regions.split(","), a.reps))
        if a.out:  # (kept up to date size by size: a long run leaves what it has measured)
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
