#!/usr/bin/env python3
"""Masked fields: what the split, fill and restore kernels cost against the bytes they move, what a masked encode / decode
costs against the plain call on the pre-padded field, and what the mask weighs, in one process with the rows interleaved.

  mask_split(f)  vs  minmax(f)                  both are one read of the field: the stage calls' wall time (one launch pair and
                                                one synchronise each) on the same device array, in the same repetition
  mask_fill, mask_restore                       wall time of the stage calls, against ceil(n / 8) mask bytes read and
                                                undefined * sizeof(sample) bytes stored
  encode_host_seg_masked(f)                     vs encode_host_seg(padded), padded = f with its undefined samples replaced by
                                                the pad the masked call returned (the bytes are compared in the warm-up round)
  decode_host_seg_masked(record)                vs decode_host_seg(field part)
  mask_len                                      vs the field part, and vs the reference's scheme for the same mask: the plain
                                                encode of the {lo, 0} mask field without the transform at the MSSG mask tolerance
  wrenc_mssg [--mask=bits]                      (--tool-size N, 0 = skip) on a single-precision regular-output set of N^3 with
                                                about 30 % undefined points, WR_STREAM_FORMAT=wrs1: wall time and payload size

Fields are the synthetic field at --sizes cubed, fp64, and fp32 at --f32-sizes; the undefined samples are a disc in the x-y
plane through every z (0, about 1 % and about 30 % of the samples) holding a value far below the threshold.  --reps repetitions
after a warm-up round; medians.  The two calls of a whole-call pair run in the order a, b, b, a inside a repetition and a call's
time is the mean of its two; an untimed plain call goes in front of each pair, because the first decode after an encode (and
the first encode after a decode) was measured slower even where both calls of the pair run the same code.  mask_coder_ms, split_ms, fill_ms are the library's HIP-event times; `coder_under_transform` says
whether the mask's coder kernels (on their own stream) took less than the field's transform and quantizer stages,
`coder_under_field_coders` whether they took less than those plus the field's own plane coders, which follow on the context's
stream.  There is no gate.

    python tools/masked_rate.py [--sizes 512,1024] [--f32-sizes 512] [--tol 1e-5] [--reps 5] [--tool-size 256] [--out profiles/masked/masked_rate.json]

Prints one JSON object (and rewrites --out after every row)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

UNDEF = -9.99e33
BELOW = -1e30
FRACTIONS = (("0%", 0.0), ("1%", 0.01), ("30%", 0.30))
MSSG_MASK_TOLREL = 0.126


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


def row(api, ctx, f, padded, out, land, dtype, tol, reps):
    n = f.size
    f32 = np.dtype(dtype) == np.float32
    enc_m = ctx.encode_host_seg_masked_f32 if f32 else ctx.encode_host_seg_masked
    dec_m = ctx.decode_host_seg_masked_f32 if f32 else ctx.decode_host_seg_masked
    enc_p = ctx.encode_host_seg_f32 if f32 else ctx.encode_host_seg
    dec_p = ctx.decode_host_seg_f32 if f32 else ctx.decode_host_seg
    item = np.dtype(dtype).itemsize
    d_f = ctx.to_device(f)
    d_bits = ctx.alloc((n + 7) // 8 + 256)
    t = {k: [] for k in ("split", "minmax", "fill", "restore", "enc_masked", "enc_plain", "dec_masked", "dec_plain", "split_ms", "fill_ms", "coder_ms",
                         "under_ms", "restore_ms", "dec_coder_ms", "field_coder_ms")}
    info = {}
    try:
        for rep in range(reps + 1):  # the first round warms up and checks the bytes
            dt_split, (undefined, pad) = timed(ctx.mask_split, d_f, n, d_bits, BELOW, dtype=dtype)
            dt_mm, _ = timed(ctx.minmax, d_f, n) if not f32 else (float("nan"), None)
            dt_fill, _ = timed(ctx.mask_fill, d_f, n, d_bits, UNDEF, dtype=dtype)  # (the value that is there: the array stays as it is)
            dt_rest, count = timed(ctx.mask_restore, d_f, n, d_bits, UNDEF, dtype=dtype)
            if rep:  # (the first encode after a decode is slower whichever call it is: it belongs to neither call of the pair)
                enc_p(padded, tol)
            dt_em, (rec, tm_m) = timed(enc_m, f, tol, BELOW)
            rec["data"] = rec["data"].copy()
            mask = rec["mask"]
            if not rep:
                if undefined:
                    padded.reshape(f.shape)[:, land] = dtype(mask["pad"])
                assert count == undefined == mask["undefined"] and (pad == mask["pad"] or (pad != pad and not n - undefined))
            dt_ep, (plain, tm_p) = timed(enc_p, padded, tol)
            # (each pair once more in the other order, the two times of a call averaged: whatever the first call of a pair pays
            # for coming first, both pay once)
            dt_ep = 0.5 * (dt_ep + timed(enc_p, padded, tol)[0])
            dt_em = 0.5 * (dt_em + timed(enc_m, f, tol, BELOW)[0])
            nt = rec["ntot_enc"]
            field_part = dict(rec, data=rec["data"][:nt])
            dec_p(out, field_part)  # (likewise the first decode after an encode)
            dt_dm, (got, _) = timed(dec_m, out, rec, UNDEF)
            dt_dp, _ = timed(dec_p, out, field_part)
            dt_dp = 0.5 * (dt_dp + timed(dec_p, out, field_part)[0])
            dt_dm = 0.5 * (dt_dm + timed(dec_m, out, rec, UNDEF)[0])
            if not rep:
                if not (np.array_equal(rec["data"][:nt], plain["data"]) and rec["len_enc_vec"] == plain["len_enc_vec"]):
                    raise SystemExit("masked_rate: the field part of the masked record differs from the plain call's stream")
                ref_scheme = None
                if undefined:
                    lo = float(f.min())
                    m = np.zeros(f.shape)
                    m[:, land] = lo
                    ref_enc, _ = ctx.encode_host_seg(m, MSSG_MASK_TOLREL, 0)
                    ref_scheme = int(ref_enc["ntot_enc"])
                    del m
                info = dict(samples=n, dtype=np.dtype(dtype).name, undefined=int(undefined), undefined_share=round(undefined / n, 5), pad=mask["pad"],
                            field_bytes=int(nt), mask_len=int(mask["mask_len"]), mask_over_field=round(mask["mask_len"] / max(nt, 1), 6),
                            reference_scheme_mask_bytes=ref_scheme, same_bytes=True)
                continue
            t["split"].append(dt_split); t["minmax"].append(dt_mm); t["fill"].append(dt_fill); t["restore"].append(dt_rest)
            t["enc_masked"].append(dt_em); t["enc_plain"].append(dt_ep); t["dec_masked"].append(dt_dm); t["dec_plain"].append(dt_dp)
            t["split_ms"].append(mask["split_ms"]); t["fill_ms"].append(mask["fill_ms"]); t["coder_ms"].append(mask["mask_coder_ms"])
            t["under_ms"].append(tm_m["transform_ms"] + tm_m["quant_ms"])
            t["field_coder_ms"].append(1e3 * tm_m["rangecoder"])
            t["restore_ms"].append(got["fill_ms"]); t["dec_coder_ms"].append(got["mask_coder_ms"])
    finally:
        d_f.free()
        d_bits.free()
    o = dict(info)
    o["split_call_s"], o["minmax_call_s"] = med(t["split"]), (None if f32 else med(t["minmax"]))
    o["split_over_minmax"] = None if f32 else round(o["split_call_s"] / o["minmax_call_s"], 3)
    o["split_read_GBps"] = round(n * item / o["split_call_s"] / 1e9, 1)
    moved = (n + 7) // 8 + info["undefined"] * item
    for k in ("fill", "restore"):
        o[k + "_call_s"] = med(t[k])
        o[k + "_bytes"] = moved
        o[k + "_GBps"] = round(moved / o[k + "_call_s"] / 1e9, 2)
    for k in ("enc_masked", "enc_plain", "dec_masked", "dec_plain"):
        o[k + "_s"] = med(t[k], 5)
    o["encode_masked_over_plain"] = round(o["enc_masked_s"] / o["enc_plain_s"], 3)
    o["decode_masked_over_plain"] = round(o["dec_masked_s"] / o["dec_plain_s"], 3)
    o["event_ms"] = dict(split=med(t["split_ms"], 4), fill=med(t["fill_ms"], 4), mask_coder=med(t["coder_ms"], 4),
                         transform_plus_quantizer=med(t["under_ms"], 4), field_plane_coders=med(t["field_coder_ms"], 4), restore=med(t["restore_ms"], 4), decode_mask_coder=med(t["dec_coder_ms"], 4))
    # the mask's coder starts when the split has been read back; the field's plane coders follow the transform and quantizer on
    # the context's stream, one plane after the other
    o["coder_under_transform"] = bool(o["event_ms"]["mask_coder"] <= o["event_ms"]["transform_plus_quantizer"])
    o["coder_under_field_coders"] = bool(o["event_ms"]["mask_coder"] <= o["event_ms"]["transform_plus_quantizer"] + o["event_ms"]["field_plane_coders"])
    return o


def tool_rows(n, tol, reps):
    """wrenc_mssg with and without --mask=bits on a regular-output set of n^3 single-precision samples, about 30 % undefined"""
    from waverange_amd import synth
    enc = os.path.join(ROOT, "waverange_amd", "bin", "wrenc_mssg")
    f = (synth.field(n, n, n, seed=500) * 3.0 + 280.0).astype(np.float32)
    f[:, disc(n, 0.30)] = np.float32(UNDEF)
    out = {}
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "t.ctl"), "w") as fh:
            fh.write("DSET ^t.grd\nTITLE synthetic MSSG regular output\nUNDEF -9.99E33\nXDEF %d LINEAR 0.0 1.0\nYDEF %d LINEAR 0.0 1.0\n"
                     "ZDEF %d LEVELS 1 2 3\nTDEF 1 LINEAR 00Z01JAN2000 1hr\nVARS 1\nt %d 99 temperature\nENDVARS\n" % (n, n, n, n))
        f.tofile(os.path.join(d, "t.grd"))
        del f
        env = dict(os.environ, WR_QUIET="1", WR_STREAM_FORMAT="wrs1")
        times = {"plain": [], "bits": []}
        sizes = {}
        for rep in range(reps + 1):
            for name, opts in (("plain", []), ("bits", ["--mask=bits"])):
                dt, _ = timed(subprocess.run, [enc] + opts + ["t", ".enc", "0", "1", "0", str(tol), "0"], cwd=d, env=env, check=True,
                              stdout=subprocess.DEVNULL, timeout=600)
                sizes[name] = os.path.getsize(os.path.join(d, "t_f.enc"))
                if rep:
                    times[name].append(dt)
        out = dict(samples=n ** 3, wall_s={k: med(v, 4) for k, v in times.items()}, payload_bytes=sizes,
                   bits_over_plain_wall=round(med(times["bits"]) / med(times["plain"]), 3),
                   bits_over_plain_bytes=round(sizes["bits"] / sizes["plain"], 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,1024")
    ap.add_argument("--f32-sizes", default="512")
    ap.add_argument("--tol", type=float, default=1e-5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tool-size", type=int, default=256)
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

    cases = [(int(v), np.float64) for v in a.sizes.split(",") if v] + [(int(v), np.float32) for v in a.f32_sizes.split(",") if v]
    with api.Context(0) as ctx:
        for n, dtype in cases:
            base = np.empty((n, n, n), dtype)
            buf = ctx.alloc(8 * base.size)
            ctx.synth_field(buf, n, n, n, 2024)
            base.reshape(-1)[:] = buf.download(np.float64, base.size)
            buf.free()
            # the encoders' inputs are pinned; the decoders' output is pageable for both decodes alike
            f, padded, out = api.pinned_array((n, n, n), dtype), api.pinned_array((n, n, n), dtype), np.empty((n, n, n), dtype)
            for name, fraction in FRACTIONS:
                land = disc(n, fraction) if fraction else np.zeros((n, n), bool)
                f[...] = base
                padded[...] = base
                if fraction:
                    f[:, land] = dtype(UNDEF)
                key = "%d^3 %s %s undefined" % (n, np.dtype(dtype).name, name)
                res["rows"][key] = row(api, ctx, f, padded, out, land, dtype, a.tol, a.reps)
                emit()
                print(key, "done", file=sys.stderr, flush=True)
            del base, f, padded, out
    if a.tool_size:
        res["wrenc_mssg"] = tool_rows(a.tool_size, a.tol, a.reps)
        emit()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
