#!/usr/bin/env python3
"""Masked region decode across a batch of fields: the one call against the loop it replaces, in one process.

  a  decode_host_seg_rois_batch_masked(records, regions)            the new call
  b  decode_host_seg_roi_masked(record, region) for every record and region: the loop, the yardstick
  c  decode_host_seg_rois_batch(field parts, regions)               the plain batch call on the same records: a - c is what
                                                                    the masks cost

Within a repetition the order is a, b, b, a behind an untimed call, a call's time the mean of its two (DESIGN 10.14 says why:
the first call behind a pause pays for it); c is timed once per repetition behind them.  --reps repetitions after a warm-up
round; medians.  Recorded per row: the wall times, tm["rangecoder"] of a against the sum over the loop of rangecoder and
mask_coder_ms, the restore launch (fill_ms of a, HIP events) against the sum of the loop's, and the deltas of
WR_STAT_ROI_CODER_LAUNCHES, WR_STAT_MASK_ROI_SEGMENTS and WR_STAT_MASK_ROI_BYTES_UP for a and for b.  There is no gate.

Rows: --rows 8x256,64x256,8x512 (fields x edge), --regions probe (one centred 32^3 box), probes8 (eight 32^3 boxes on the
diagonal), level2 (the whole box of level 2), --formats wrs1,wrs3.  The fields are the synthetic field, fp64, with a disc of about
30 % of the x-y plane undefined through every z, tolerance 1e-3.  One record is encoded per (edge, format) and stands for every
field of the batch: a decode does not care that its records are equal.

    python tools/masked_roi_batch_rate.py [--rows 8x256] [--regions probe,probes8,level2] [--formats wrs1,wrs3] [--reps 5]
                                          [--out profiles/masked_roi_batch/masked_roi_batch_rate.json]

Prints one JSON object (and rewrites --out after every row)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

UNDEF = -9.99e33
BELOW = -1e30
FORMATS = {"wrs1": dict(brick=0, strands=0), "wrs3": dict(brick=0, strands=8)}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def med(v, digits=6):
    return round(float(np.median(v)), digits)


def disc(n, fraction):
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return (x - 0.45 * n) ** 2 + (y - 0.55 * n) ** 2 < fraction * n * n / np.pi


def regions_of(name, n):
    c = n // 2
    if name == "probe":
        return 0, [((c - 16, c + 16),) * 3]
    if name == "probes8":
        step = (n - 32) // 7
        return 0, [((k * step, k * step + 32),) * 3 for k in range(8)]
    if name == "level2":
        b = (n + 3) // 4
        return 2, [((0, b), (0, b), (0, b))]
    raise SystemExit("unknown region set " + name)


def row(api, ctx, rec, nfields, n, level, rois, reps):
    shape = (n, n, n)
    recs = [rec] * nfields
    parts = [dict(rec, data=rec["data"][:rec["ntot_enc"]])] * nfields
    T = int(api.roi_multi_offsets(shape, level, rois)[-1])
    out = api.pinned_array((nfields * T,), np.float64)
    singles = [np.empty(api.roi_shape(r)) for r in rois]
    stats = (api.STAT_ROI_CODER_LAUNCHES, api.STAT_MASK_ROI_SEGMENTS, api.STAT_MASK_ROI_BYTES_UP)
    got = {}

    def a():
        masks, tm = [], {}
        ctx.decode_host_seg_rois_batch_masked(shape, level, rois, recs, UNDEF, out=out, masks=masks, timings=tm)
        got["a"] = dict(rangecoder_ms=1e3 * tm["rangecoder"], fill_ms=masks[0]["fill_ms"], undefined=sum(m["undefined"] for m in masks))

    def b():
        coder = mask_coder = fill = 0.0
        und = 0
        for r in recs:
            for o, roi in zip(singles, rois):
                res, tm = ctx.decode_host_seg_roi_masked(o, shape, level, roi, r, UNDEF)
                coder += 1e3 * tm["rangecoder"]; mask_coder += res["mask_coder_ms"]; fill += res["fill_ms"]; und += res["undefined"]
        got["b"] = dict(rangecoder_ms=coder, mask_coder_ms=mask_coder, fill_ms=fill, undefined=und)

    def c():
        ctx.decode_host_seg_rois_batch(shape, level, rois, parts, out=out)

    def delta(fn):
        s0 = [api.stat(s) for s in stats]
        fn()
        return dict(zip(("coder_launches", "mask_segments", "mask_bytes_up"), [api.stat(s) - v for s, v in zip(stats, s0)]))

    counters = dict(a=delta(a), b=delta(b))
    assert got["a"]["undefined"] == got["b"]["undefined"]
    ta, tb, tc, ea, eb = [], [], [], [], []
    for rep in range(reps + 1):
        c()  # (untimed)
        a1 = timed(a); b1 = timed(b); b2 = timed(b); a2 = timed(a)
        c1 = timed(c)
        if rep:
            ta.append(0.5 * (a1 + a2)); tb.append(0.5 * (b1 + b2)); tc.append(c1)
            ea.append(dict(got["a"])); eb.append(dict(got["b"]))
    return dict(nfields=nfields, edge=n, level=level, nroi=len(rois), out_elems_per_field=T, undefined_in_regions=int(got["a"]["undefined"]),
                batch_s=med(ta, 5), loop_s=med(tb, 5), plain_batch_s=med(tc, 5), loop_over_batch=round(med(tb) / med(ta), 2),
                masks_cost_s=round(med(ta) - med(tc), 5),
                batch_rangecoder_ms=med([e["rangecoder_ms"] for e in ea], 3),
                loop_rangecoder_ms=med([e["rangecoder_ms"] for e in eb], 3), loop_mask_coder_ms=med([e["mask_coder_ms"] for e in eb], 3),
                batch_restore_ms=med([e["fill_ms"] for e in ea], 4), loop_restore_ms_sum=med([e["fill_ms"] for e in eb], 4),
                counters=counters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="8x256,64x256,8x512")
    ap.add_argument("--regions", default="probe,probes8,level2")
    ap.add_argument("--formats", default="wrs1,wrs3")
    ap.add_argument("--tol", type=float, default=1e-3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from waverange_amd import api
    api.set_verbosity(0)
    res = {"argv": sys.argv[1:], "tol": a.tol, "reps": a.reps, "order": "untimed c; a, b, b, a; c", "rows": {}}

    def emit():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                json.dump(res, fh, indent=1)
                fh.write("\n")

    rows = [tuple(int(v) for v in r.split("x")) for r in a.rows.split(",") if r]
    with api.Context(0) as ctx:
        for n in sorted({e for _, e in rows}):
            buf = ctx.alloc(8 * n ** 3)
            ctx.synth_field(buf, n, n, n, 2024)
            f = buf.download(np.float64, n ** 3).reshape(n, n, n)
            buf.free()
            f[:, disc(n, 0.30)] = UNDEF
            for fmt in [v for v in a.formats.split(",") if v]:
                rec, _ = ctx.encode_host_seg_masked(f, a.tol, BELOW, **FORMATS[fmt])
                rec["data"] = rec["data"].copy()
                for nfields, edge in rows:
                    if edge != n:
                        continue
                    for name in [v for v in a.regions.split(",") if v]:
                        level, rois = regions_of(name, n)
                        key = "%d x %d^3 %s %s" % (nfields, n, fmt, name)
                        res["rows"][key] = dict(row(api, ctx, rec, nfields, n, level, rois, a.reps), nlay=int(rec["nlay"]),
                                                undefined_share=round(rec["mask"]["undefined"] / f.size, 4))
                        emit()
                        print(key, "done", file=sys.stderr, flush=True)
            del f
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
