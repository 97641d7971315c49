#!/usr/bin/env python3
"""Masked fields in the tolerance searches: what the masked compare costs against the plain one, and what the masked quality and
budget calls cost against the plain calls on the pre-padded field, in one process with the rows interleaved.

  err_stats_masked(a, b, bits)  vs  err_stats(a, b)   the stage calls' wall time (one launch pair and one synchronise each) on the
                                                      same two device arrays in the same repetition; by traffic the masked
                                                      compare reads 16 + 1/8 bytes per sample (fp64) against 16, and neither
                                                      array where a turn's 128 bits are all set
  encode_host_seg_quality_masked(f)                   vs encode_host_seg_quality(padded), an RMS target of --rms times max|f|;
                                                      padded = f with its undefined samples replaced by the returned pad (g and the
                                                      bytes of the field part are compared in the warm-up round)
  encode_host_seg_budget_masked(f, B)                 vs encode_host_seg_budget(padded, B - mask_len), B = the field's bytes / --ratio

Fields are the synthetic field at --sizes cubed (fp64) and --f32-sizes (fp32); the second array of the compare is the synthetic
field of another seed.  The undefined samples are a disc in the x-y plane through every z: 0, about 1 % and about 30 % of the
samples, holding a value far below the threshold.  The whole calls run at --call-sizes / --call-f32-sizes.  --reps repetitions
after a warm-up round; medians.  The two calls of a pair run in the order a, b, b, a inside a repetition, behind an untimed call,
and a call's time is the mean of its two (tools/masked_rate.py says why).  There is no gate.

    python tools/masked_quality_rate.py [--sizes 512,1024] [--f32-sizes 512,1024] [--call-sizes 512,1024] [--call-f32-sizes 512]
                                        [--rms 1e-3] [--ratio 8] [--reps 5] [--out profiles/masked_quality/masked_quality_rate.json]

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
FRACTIONS = (("0%", 0.0), ("1%", 0.01), ("30%", 0.30))


def timed(fn, *a, **k):
    t0 = time.perf_counter()
    r = fn(*a, **k)
    return time.perf_counter() - t0, r


def med(v, digits=6):
    return round(float(np.median(v)), digits)


def disc(n, fraction):
    """(n, n) boolean: a disc of about `fraction` of the x-y plane"""
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    r2 = fraction * n * n / np.pi
    return (x - 0.45 * n) ** 2 + (y - 0.55 * n) ** 2 < r2


def device_field(ctx, n, seed, dtype):
    """the synthetic field of n^3 samples on the device, and (fp32: only then) its host copy"""
    buf = ctx.alloc(8 * n ** 3)
    ctx.synth_field(buf, n, n, n, seed)
    if np.dtype(dtype) == np.float64:
        return buf
    host = buf.download(np.float64, n ** 3).astype(np.float32)
    buf.free()
    return ctx.to_device(host)


def compare_rows(ctx, n, dtype, reps, res, emit):
    count = n ** 3
    item = np.dtype(dtype).itemsize
    d_a, d_b = device_field(ctx, n, 2024, dtype), device_field(ctx, n, 2025, dtype)
    d_bits = ctx.alloc((count + 7) // 8 + 256)
    try:
        for name, fraction in FRACTIONS:
            land = disc(n, fraction) if fraction else np.zeros((n, n), bool)
            row_bits = np.packbits(land.reshape(-1), bitorder="little")  # (n * n is a multiple of 8 at these sizes)
            d_bits.upload(np.tile(row_bits, n))
            t = {"masked": [], "plain": []}
            got = None
            for rep in range(reps + 1):
                dt_p, plain = timed(ctx.err_stats, d_a, d_b, count, dtype=dtype)
                dt_m, got = timed(ctx.err_stats_masked, d_a, d_b, count, d_bits, dtype=dtype)
                dt_m = 0.5 * (dt_m + timed(ctx.err_stats_masked, d_a, d_b, count, d_bits, dtype=dtype)[0])
                dt_p = 0.5 * (dt_p + timed(ctx.err_stats, d_a, d_b, count, dtype=dtype)[0])
                if not rep:
                    assert got["defined"] == count - int(land.sum()) * n, (got, int(land.sum()) * n)
                    assert fraction or (got["sumsq"] == plain["sumsq"] and got["max_abs"] == plain["max_abs"]), (got, plain)
                    continue
                t["masked"].append(dt_m); t["plain"].append(dt_p)
            key = "compare %d^3 %s %s undefined" % (n, np.dtype(dtype).name, name)
            m, p = med(t["masked"]), med(t["plain"])
            read = got["defined"] * 2 * item + (count + 7) // 8
            res["rows"][key] = dict(samples=count, dtype=np.dtype(dtype).name, defined=got["defined"], err_stats_masked_call_s=m, err_stats_call_s=p,
                                    masked_over_plain=round(m / p, 3), plain_read_GBps=round(count * 2 * item / p / 1e9, 1),
                                    masked_read_GBps_of_defined_samples_and_mask=round(read / m / 1e9, 1))
            emit()
            print(key, "done", file=sys.stderr, flush=True)
    finally:
        d_a.free(); d_b.free(); d_bits.free()


def pair(t, name_a, call_a, name_b, call_b, untimed, rep):
    """a, b, b, a behind an untimed call; the results of the first a and b"""
    untimed()
    dt_a, ra = timed(call_a)
    dt_b, rb = timed(call_b)
    dt_b = 0.5 * (dt_b + timed(call_b)[0])
    dt_a = 0.5 * (dt_a + timed(call_a)[0])
    if rep:
        t.setdefault(name_a, []).append(dt_a)
        t.setdefault(name_b, []).append(dt_b)
    return ra, rb


def call_rows(api, ctx, n, dtype, a, res, emit):
    f32 = np.dtype(dtype) == np.float32
    q_m = ctx.encode_host_seg_quality_masked_f32 if f32 else ctx.encode_host_seg_quality_masked
    q_p = ctx.encode_host_seg_quality_f32 if f32 else ctx.encode_host_seg_quality
    b_m = ctx.encode_host_seg_budget_masked_f32 if f32 else ctx.encode_host_seg_budget_masked
    b_p = ctx.encode_host_seg_budget_f32 if f32 else ctx.encode_host_seg_budget
    buf = ctx.alloc(8 * n ** 3)
    ctx.synth_field(buf, n, n, n, 2024)
    base = buf.download(np.float64, n ** 3).astype(dtype).reshape(n, n, n)
    buf.free()
    absmax = float(np.abs(base).max())
    target = a.rms * absmax
    budget = int(base.nbytes / a.ratio)
    f, padded = api.pinned_array((n, n, n), dtype), api.pinned_array((n, n, n), dtype)
    for name, fraction in FRACTIONS:
        land = disc(n, fraction) if fraction else np.zeros((n, n), bool)
        f[...] = base
        padded[...] = base
        if fraction:
            f[:, land] = dtype(UNDEF)
        t, info = {}, {}
        for rep in range(a.reps + 1):
            if not rep:  # the pad, and with it the padded field
                i, _, _ = q_m(f, api.NORM_RMS, target, BELOW)
                mask = dict(i["mask"])
                if fraction:
                    padded[:, land] = dtype(mask["pad"])
            (mi, md, mr), (pi, pd, pr) = pair(t, "quality_masked", lambda: q_m(f, api.NORM_RMS, target, BELOW), "quality_plain",
                                              lambda: q_p(padded, api.NORM_RMS, target), lambda: q_p(padded, api.NORM_RMS, target), rep)
            if not rep:
                # (with a sample undefined the two calls judge different things -- R over D against R over all n -- and may choose
                # different grid points; without one they are the same call)
                same = mr["g"] == pr["g"] and np.array_equal(md[:mi["ntot_enc"]], pd)
                assert fraction or same
                info = dict(samples=n ** 3, dtype=np.dtype(dtype).name, undefined=int(mask["undefined"]), mask_len=int(mask["mask_len"]),
                            rms_target=target, quality_masked=dict(g=mr["g"], rms=mr["rms"], max_abs=mr["max_abs"], trials=mr["trials"], field_bytes=int(mi["ntot_enc"])),
                            quality_plain_on_padded=dict(g=pr["g"], rms=pr["rms"], max_abs=pr["max_abs"], trials=pr["trials"], field_bytes=int(pi["ntot_enc"])))
            ml = int(mask["mask_len"])
            (mi, md, mr), (pi, pd, pr) = pair(t, "budget_masked", lambda: b_m(f, budget, BELOW), "budget_plain", lambda: b_p(padded, budget - ml),
                                              lambda: b_p(padded, budget - ml), rep)
            if not rep:
                if not (mr["g"] == pr["g"] and mr["bound"] == pr["bound"] and np.array_equal(md[:mi["ntot_enc"]], pd)):
                    raise SystemExit("masked_quality_rate: the masked budget call differs from the plain call at max_bytes - mask_len")
                info["budget"] = dict(max_bytes=budget, g=mr["g"], bound=int(mr["bound"]), field_bytes=int(mi["ntot_enc"]), probe_passes=mr["probe_passes"],
                                      record_bytes=int(mi["ntot_enc"]) + ml)
        o = dict(info)
        for k, v in t.items():
            o[k + "_s"] = med(v, 5)
        o["quality_masked_over_plain"] = round(o["quality_masked_s"] / o["quality_plain_s"], 3)
        o["budget_masked_over_plain"] = round(o["budget_masked_s"] / o["budget_plain_s"], 3)
        key = "calls %d^3 %s %s undefined" % (n, np.dtype(dtype).name, name)
        res["rows"][key] = o
        emit()
        print(key, "done", file=sys.stderr, flush=True)


def sizes(text):
    return [int(v) for v in text.split(",") if v]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,1024")
    ap.add_argument("--f32-sizes", default="512,1024")
    ap.add_argument("--call-sizes", default="512,1024")
    ap.add_argument("--call-f32-sizes", default="512")
    ap.add_argument("--rms", type=float, default=1e-3)
    ap.add_argument("--ratio", type=float, default=8.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from waverange_amd import api
    api.set_verbosity(0)
    res = {"argv": sys.argv[1:], "rms": a.rms, "ratio": a.ratio, "reps": a.reps, "rows": {}}

    def emit():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                json.dump(res, fh, indent=1)
                fh.write("\n")

    with api.Context(0) as ctx:
        for n, dtype in [(n, np.float64) for n in sizes(a.sizes)] + [(n, np.float32) for n in sizes(a.f32_sizes)]:
            compare_rows(ctx, n, dtype, a.reps, res, emit)
        for n, dtype in [(n, np.float64) for n in sizes(a.call_sizes)] + [(n, np.float32) for n in sizes(a.call_f32_sizes)]:
            call_rows(api, ctx, n, dtype, a, res, emit)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
