#!/usr/bin/env python3
"""Masked batch encode and decode: what one call for N masked fields costs against the loop of the single masked call, and
against the plain batch call on the pre-padded fields, in one process with the rows interleaved.

  a  encode_host_seg_batch_masked(fields)            / decode_host_seg_batch_masked(records)
  b  the loop of encode_host_seg_masked(field)       / decode_host_seg_masked(record) over the same fields
  c  encode_host_seg_batch[_strands](padded fields)  / decode_host_seg_batch_mixed(field parts): the plain batch call

Per repetition: an untimed call, then a, b, b, a (a call's time is the mean of its two), then c.  --reps repetitions after a
warm-up round that also compares the bytes; medians.  Wall time is time.perf_counter around the call(s); coder time is
wr_timings.rangecoder (the plane launches) plus, on an encode, the mask launch's HIP-event time (a: once, it runs on its own
stream under the plane launches, so the sum is an upper bound; b: per field).  On a decode the masks ride in the plain launch.
Fields: the synthetic field at different seeds, fp64, about 30 % of the samples undefined (a disc in the x-y plane through
every z, shifted per field).  Formats: WRS1 and WRS3 (K = 8).
Also: the batched split against the loop of the single split on the same device arrays, per sample.  There is no gate.

    python tools/masked_batch_rate.py [--cases 8x128,64x128,8x256,64x256,8x512] [--tol 1e-3] [--reps 5] [--out profiles/masked_batch/rate.json]

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


def timed(fn, *a, **k):
    t0 = time.perf_counter()
    r = fn(*a, **k)
    return time.perf_counter() - t0, r


def med(v, digits=6):
    return round(float(np.median(v)), digits)


def disc(n, fraction, shift):
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    r2 = fraction * n * n / np.pi
    return (x - (0.40 + 0.02 * (shift % 8)) * n) ** 2 + (y - 0.55 * n) ** 2 < r2


def split_rows(ctx, fields, reps):
    """mask_split_batch against the loop of mask_split on the same device arrays"""
    n = fields[0].size
    bufs = [ctx.to_device(f) for f in fields]
    bits = [ctx.alloc((n + 7) // 8 + 256) for _ in fields]
    tb, tl = [], []
    try:
        for rep in range(reps + 1):
            dt_b, got = timed(ctx.mask_split_batch, bufs, n, bits, BELOW)
            t0 = time.perf_counter()
            want = [ctx.mask_split(b, n, m, BELOW) for b, m in zip(bufs, bits)]
            dt_l = time.perf_counter() - t0
            if not rep:
                assert [g[0] for g in got] == [w[0] for w in want]
                assert [np.float64(g[1]).view(np.uint64) for g in got] == [np.float64(w[1]).view(np.uint64) for w in want]
                continue
            tb.append(dt_b)
            tl.append(dt_l)
    finally:
        for b in bufs + bits:
            b.free()
    total = n * len(fields)
    return dict(batch_call_s=med(tb), loop_s=med(tl), batch_ns_per_sample=round(1e9 * med(tb, 9) / total, 5), loop_ns_per_sample=round(1e9 * med(tl, 9) / total, 5),
                batch_read_GBps=round(8 * total / med(tb, 9) / 1e9, 1), loop_read_GBps=round(8 * total / med(tl, 9) / 1e9, 1))


def coder_s(tm, masks, once):
    ms = [m["mask_coder_ms"] for m in masks if m["mask_len"]]
    return tm["rangecoder"] + 1e-3 * ((ms[0] if ms else 0.0) if once else sum(ms))


def row(ctx, fields, tol, fmt, reps):
    nf, shape = len(fields), fields[0].shape
    kw = FORMATS[fmt]

    def enc_a():
        recs, tm = ctx.encode_host_seg_batch_masked(fields, tol, BELOW, **kw)
        for r in recs:
            r["data"] = r["data"].copy()
        return recs, coder_s(tm, [r["mask"] for r in recs], True)

    def enc_b():
        recs, c = [], 0.0
        for f in fields:
            r, tm = ctx.encode_host_seg_masked(f, tol, BELOW, **kw)
            r["data"] = r["data"].copy()
            recs.append(r)
            c += coder_s(tm, [r["mask"]], False)
        return recs, c

    recs, _ = enc_a()
    padded = [np.where(f < BELOW, r["mask"]["pad"], f) for f, r in zip(fields, recs)]

    def enc_c():
        if kw["strands"]:
            _, tm = ctx.encode_host_seg_batch_strands(padded, tol, strands=kw["strands"])
        else:
            _, tm = ctx.encode_host_seg_batch(padded, tol)
        return None, tm["rangecoder"]

    outs = [np.empty(shape) for _ in fields]
    parts = [dict(r, data=r["data"][:r["ntot_enc"]]) for r in recs]

    def dec_a():
        _, tm = ctx.decode_host_seg_batch_masked(outs, recs, UNDEF)
        return None, tm["rangecoder"]

    def dec_b():
        c = 0.0
        for o, r in zip(outs, recs):
            m, tm = ctx.decode_host_seg_masked(o, r, UNDEF)
            c += tm["rangecoder"] + 1e-3 * m["mask_coder_ms"]
        return None, c

    def dec_c():
        tm = ctx.decode_host_seg_batch_mixed(outs, parts)
        return None, tm["rangecoder"]

    # the warm-up round: the batch's records are the loop's, byte for byte
    want, _ = enc_b()
    for g, w in zip(recs, want):
        if not (np.array_equal(g["data"], w["data"]) and g["len_enc_vec"] == w["len_enc_vec"]):
            raise SystemExit("masked_batch_rate: a record of the batch differs from the single call's")
    o = dict(fields=nf, samples=int(fields[0].size), format=fmt, nlay=[r["nlay"] for r in recs], field_bytes=int(sum(r["ntot_enc"] for r in recs)),
             mask_bytes=int(sum(r["mask"]["mask_len"] for r in recs)), same_bytes=True)
    for what, (fa, fb, fc) in (("encode", (enc_a, enc_b, enc_c)), ("decode", (dec_a, dec_b, dec_c))):
        wall = {k: [] for k in "abc"}
        coder = {k: [] for k in "abc"}
        for rep in range(reps + 1):
            fc()  # (untimed: the first call after the other direction's belongs to neither)
            ta1, (_, ca1) = timed(fa)
            tb1, (_, cb1) = timed(fb)
            tb2, (_, cb2) = timed(fb)
            ta2, (_, ca2) = timed(fa)
            tc, (_, cc) = timed(fc)
            if not rep:
                continue
            wall["a"].append(0.5 * (ta1 + ta2)); wall["b"].append(0.5 * (tb1 + tb2)); wall["c"].append(tc)
            coder["a"].append(0.5 * (ca1 + ca2)); coder["b"].append(0.5 * (cb1 + cb2)); coder["c"].append(cc)
        o[what] = dict(wall_s={k: med(v, 5) for k, v in wall.items()}, coder_s={k: med(v, 6) for k, v in coder.items()},
                       loop_over_batch_wall=round(med(wall["b"]) / med(wall["a"]), 3), loop_over_batch_coder=round(med(coder["b"], 9) / med(coder["a"], 9), 3),
                       batch_over_plain_wall=round(med(wall["a"]) / med(wall["c"]), 3), batch_over_plain_coder=round(med(coder["a"], 9) / med(coder["c"], 9), 3))
    return o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="8x128,64x128,8x256,64x256,8x512")
    ap.add_argument("--tol", type=float, default=1e-3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from waverange_amd import api
    api.set_verbosity(0)
    res = {"argv": sys.argv[1:], "tol": a.tol, "reps": a.reps, "undefined_share": 0.30, "rows": {}, "split": {}}

    def emit():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                json.dump(res, fh, indent=1)
                fh.write("\n")

    with api.Context(0) as ctx:
        for case in [c for c in a.cases.split(",") if c]:
            nf, n = (int(v) for v in case.split("x"))
            fields = []
            buf = ctx.alloc(8 * n ** 3)
            for f in range(nf):
                ctx.synth_field(buf, n, n, n, 2024 + f)
                x = api.pinned_array((n, n, n), np.float64)
                x.reshape(-1)[:] = buf.download(np.float64, n ** 3)
                x[:, disc(n, 0.30, f)] = UNDEF
                fields.append(x)
            buf.free()
            res["split"]["%d x %d^3" % (nf, n)] = split_rows(ctx, fields, a.reps)
            emit()
            for fmt in FORMATS:
                key = "%d x %d^3 %s" % (nf, n, fmt)
                res["rows"][key] = row(ctx, fields, a.tol, fmt, a.reps)
                emit()
                print(key, "done", file=sys.stderr, flush=True)
            del fields
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
