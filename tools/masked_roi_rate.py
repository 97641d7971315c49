#!/usr/bin/env python3
"""Masked region and low-resolution decode: what the box restore costs against the flat restore, what a masked partial decode
costs against the plain one, and how much of the mask it touches, in one process with the rows interleaved.

  mask_restore_box(whole box, level 0)  vs  mask_restore     the same work on the same device array and mask, in the same
                                                              repetition: the stage calls' wall time
  decode_host_seg_roi_masked(record)    vs  decode_host_seg_roi / _lowres(field part), for a centred 32^3 probe, the z-plane
                                                              through the centre and the whole box at level 2
  decode_host_seg_masked(record)        vs  decode_host_seg(field part): the full decode's own ratio in the same run, which is
                                                              the yardstick for the partial ones
  WR_STAT_MASK_ROI_SEGMENTS / _BYTES_UP                       per region, against the mask's segment count and plane bytes

Fields are the synthetic field at --sizes cubed, fp64; the undefined samples are a disc in the x-y plane through every z (about
1 % and about 30 % of the samples) holding a value far below the threshold, as in tools/masked_rate.py.  --reps repetitions after
a warm-up round; medians.  The two calls of a pair run in the order a, b, b, a inside a repetition behind an untimed call, and a
call's time is the mean of its two.  mask_coder_ms and fill_ms are the library's HIP-event times.  There is no gate.

    python tools/masked_roi_rate.py [--sizes 512,1024] [--tol 1e-5] [--reps 5] [--out profiles/masked_roi/masked_roi_rate.json]

Prints one JSON object (and rewrites --out after every row)."""
import argparse
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

UNDEF = -9.99e33
BELOW = -1e30
FRACTIONS = (("1%", 0.01), ("30%", 0.30))


def timed(fn, *a, **k):
    t0 = time.perf_counter()
    r = fn(*a, **k)
    return time.perf_counter() - t0, r


def med(v, digits=6):
    return round(float(np.median(v)), digits)


def disc(n, fraction):
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return (x - 0.45 * n) ** 2 + (y - 0.55 * n) ** 2 < fraction * n * n / np.pi


def pair(a, b):
    """the times of a and b run in the order a, b, b, a: the mean of each call's two"""
    ta, _ = timed(a)
    tb, _ = timed(b)
    tb = 0.5 * (tb + timed(b)[0])
    ta = 0.5 * (ta + timed(a)[0])
    return ta, tb


def row(api, ctx, f, land, tol, reps):
    n3 = f.size
    n = f.shape[0]
    shape = f.shape
    rec, _ = ctx.encode_host_seg_masked(f, tol, BELOW)
    rec["data"] = rec["data"].copy()
    nt = rec["ntot_enc"]
    field_part = dict(rec, data=rec["data"][:nt])
    at = nt + 32
    mask_seg, mask_nseg = struct.unpack("<II", bytes(rec["data"][at + 4:at + 12]))
    mask_plane_bytes = int(rec["mask"]["mask_len"]) - 32 - 12 - 4 * mask_nseg
    c = n // 2
    regions = {"probe 32^3": (0, ((c - 16, c + 16),) * 3), "z-plane": (0, ((c, c + 1), (0, n), (0, n))), "level 2": (2, None)}
    # ---- the kernel: the box restore on the whole box at level 0 against the flat restore
    und = np.zeros(shape, bool)
    und[:, land] = True
    bits = np.packbits(und.reshape(-1), bitorder="little")
    del und
    d_f = ctx.to_device(f)
    d_bits = ctx.to_device(np.concatenate([bits, np.zeros(256, np.uint8)]))
    t_box, t_flat = [], []
    try:
        for rep in range(reps + 1):
            ctx.mask_restore(d_f, n3, d_bits, UNDEF)  # (untimed)
            tb, tf = pair(lambda: ctx.mask_restore_box(d_f, shape, 0, None, d_bits, UNDEF), lambda: ctx.mask_restore(d_f, n3, d_bits, UNDEF))
            if rep:
                t_box.append(tb); t_flat.append(tf)
    finally:
        d_f.free()
        d_bits.free()
    o = dict(samples=n3, undefined=int(rec["mask"]["undefined"]), undefined_share=round(rec["mask"]["undefined"] / n3, 5), field_bytes=int(nt),
             mask_len=int(rec["mask"]["mask_len"]), mask_segments=int(mask_nseg), mask_seg=int(mask_seg),
             restore_box_call_s=med(t_box), restore_call_s=med(t_flat), restore_box_over_restore=round(med(t_box) / med(t_flat), 3))
    # ---- the full decode's own ratio: the yardstick
    out = np.empty(shape)
    t_m, t_p = [], []
    for rep in range(reps + 1):
        ctx.decode_host_seg(out, field_part)  # (untimed)
        tm, tp = pair(lambda: ctx.decode_host_seg_masked(out, rec, UNDEF), lambda: ctx.decode_host_seg(out, field_part))
        if rep:
            t_m.append(tm); t_p.append(tp)
    o["full"] = dict(masked_s=med(t_m, 5), plain_s=med(t_p, 5), masked_over_plain=round(med(t_m) / med(t_p), 3))
    del out
    # ---- the partial decodes
    o["regions"] = {}
    for name, (level, roi) in regions.items():
        oshape = api.roi_shape(roi) if roi is not None else api.lowres_shape(shape, level)
        out = np.empty(oshape)
        plain = (lambda: ctx.decode_host_seg_roi(out, shape, level, roi, field_part)) if roi is not None else (lambda: ctx.decode_host_seg_lowres(out, shape, level, field_part))
        got = {}

        def masked():
            got["res"], got["tm"] = ctx.decode_host_seg_roi_masked(out, shape, level, roi, rec, UNDEF)

        t_m, t_p, coder, fill, field_coder = [], [], [], [], []
        s0 = api.stat(api.STAT_MASK_ROI_SEGMENTS), api.stat(api.STAT_MASK_ROI_BYTES_UP)
        masked()
        segs, up = api.stat(api.STAT_MASK_ROI_SEGMENTS) - s0[0], api.stat(api.STAT_MASK_ROI_BYTES_UP) - s0[1]
        assert segs == len(api.mask_roi_segments(shape, level, roi, mask_seg))
        for rep in range(reps + 1):
            plain()  # (untimed)
            tm, tp = pair(masked, plain)
            if rep:
                t_m.append(tm); t_p.append(tp)
                coder.append(got["res"]["mask_coder_ms"]); fill.append(got["res"]["fill_ms"]); field_coder.append(1e3 * got["tm"]["rangecoder"])
        o["regions"][name] = dict(level=level, out_elems=int(np.prod(oshape)), undefined_in_box=int(got["res"]["undefined"]), masked_s=med(t_m, 5),
                                  plain_s=med(t_p, 5), masked_over_plain=round(med(t_m) / med(t_p), 3),
                                  above_the_full_decodes_ratio=bool(med(t_m) / med(t_p) > o["full"]["masked_over_plain"]),
                                  event_ms=dict(mask_coder=med(coder, 4), restore=med(fill, 4), field_plane_coders=med(field_coder, 4)),
                                  coder_under_field_coders=bool(med(coder) <= med(field_coder)),
                                  mask_segments_up=int(segs), mask_segments_share=round(segs / mask_nseg, 5), mask_bytes_up=int(up),
                                  mask_bytes_share=round(up / max(mask_plane_bytes, 1), 5))
    return o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,1024")
    ap.add_argument("--tol", type=float, default=1e-5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from waverange_amd import api
    api.set_verbosity(0)
    res = {"argv": sys.argv[1:], "tol": a.tol, "reps": a.reps, "rows": {}}

    def emit():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                json.dump(res, fh, indent=1)
                fh.write("\n")

    with api.Context(0) as ctx:
        for n in [int(v) for v in a.sizes.split(",") if v]:
            buf = ctx.alloc(8 * n ** 3)
            ctx.synth_field(buf, n, n, n, 2024)
            base = buf.download(np.float64, n ** 3).reshape(n, n, n)
            buf.free()
            f = api.pinned_array((n, n, n), np.float64)
            for name, fraction in FRACTIONS:
                land = disc(n, fraction)
                f[...] = base
                f[:, land] = UNDEF
                key = "%d^3 float64 %s undefined" % (n, name)
                res["rows"][key] = row(api, ctx, f, land, a.tol, a.reps)
                emit()
                print(key, "done", file=sys.stderr, flush=True)
            del base, f
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
