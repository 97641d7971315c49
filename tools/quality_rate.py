#!/usr/bin/env python3
"""Encode to an RMS target against the plain segmented encode at the tolerance it returns, and the new compare kernel against
the pointwise call's, in the same run.

  encode_host_seg_quality(f, NORM_RMS, M)       the search in the L2 norm (trials on the device), every plane coded once
  encode_host_seg(f, budget_tol(g))             the existing call at the tolerance the search chose: the yardstick
  encode_host_seg_bounded(f, M)                 the pointwise call on the same field: its trials run k_linf_cnt on arrays of
                                                the same size and alignment, the yardstick of k_err_stats

Per size and nominal tolerance the target is M = tol * max|f|.  The three calls are interleaved inside each repetition; --reps
repetitions after a warm-up round in which the quality call's bytes are compared with the plain call's and its RMS error with
seg_error_stats_host of the stream (the run ends with an error where they differ); medians.  Recorded per row: wall time of
the quality and the plain call and their ratio, the start point and the grid point chosen, the RMS error reached and its ratio
to the target, the PSNR, the trials, the planes coded (WR_STAT_QUALITY_CODER_RUNS), the time of one trial's three stages as
HIP-event milliseconds summed over the call's trials and divided by their number, the same for the pointwise call, and
compare_ratio = the quality call's compare stage (k_err_stats) over the pointwise call's (k_linf_cnt).  There is no gate.

    python tools/quality_rate.py [--sizes 512,1024] [--tols 1e-3,1e-7] [--reps 5] [--seg 0] [--out profiles/quality/quality_rate.json]

Prints one JSON object (and rewrites --out after every row)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("requant_ms", "inverse_ms", "compare_ms")


def timed(fn, *a, **k):
    t0 = time.perf_counter()
    r = fn(*a, **k)
    return time.perf_counter() - t0, r


def med(v, digits=5):
    return round(float(np.median(v)), digits)


def row(api, ctx, f, absmax, tol, reps, seg):
    target = tol * absmax
    t = {"quality": [], "plain": [], "bounded": []}
    t.update({"q_" + k: [] for k in STAGES})
    t.update({"b_" + k: [] for k in STAGES})
    info = {}
    for rep in range(reps + 1):  # the first round warms up and checks the bytes
        before = api.stat(api.STAT_QUALITY_CODER_RUNS)
        dt_q, (enc, data, res) = timed(ctx.encode_host_seg_quality, f, api.NORM_RMS, target, seg=seg)
        runs = api.stat(api.STAT_QUALITY_CODER_RUNS) - before
        q_stage = ctx.bounded_trial_ms()
        dt_p, (plain, _) = timed(ctx.encode_host_seg, f, res["tolrel"], 1, seg)
        dt_b, (_, _, bres) = timed(ctx.encode_host_seg_bounded, f, target, seg=seg)
        b_stage = ctx.bounded_trial_ms()
        if not rep:
            if not (np.array_equal(data, plain["data"]) and enc["len_enc_vec"] == plain["len_enc_vec"] and runs == enc["nlay"]):
                raise SystemExit("quality_rate: the quality call's stream differs from the plain call's at tol %g" % res["tolrel"])
            st = ctx.seg_error_stats_host(f, enc)
            if st["rms"] != res["rms"] or st["max_abs"] != res["max_abs"] or not st["rms"] <= target:
                raise SystemExit("quality_rate: the stream measures %r, the call said %r for the target %r" % (st, res, target))
            info = dict(target=target, nominal_tol=tol, start=api.bounded_start(target, absmax), g=res["g"], tolrel=res["tolrel"], rms=res["rms"],
                        rms_over_target=round(res["rms"] / target, 6), max_abs=res["max_abs"], psnr=round(res["psnr"], 4), trials=res["trials"],
                        nlay=int(enc["nlay"]), ntot_enc=int(enc["ntot_enc"]), coder_runs=int(runs), same_bytes=True,
                        bounded_g=bres["g"], bounded_trials=bres["trials"])
            continue
        t["quality"].append(dt_q); t["plain"].append(dt_p); t["bounded"].append(dt_b)
        for k, v in zip(STAGES, q_stage):
            t["q_" + k].append(v / max(res["trials"], 1))
        for k, v in zip(STAGES, b_stage):
            t["b_" + k].append(v / max(bres["trials"], 1))
    out = dict(info)
    out["quality_s"], out["plain_s"], out["bounded_s"] = med(t["quality"]), med(t["plain"]), med(t["bounded"])
    out["per_trial"] = {k: med(t["q_" + k], 4) for k in STAGES}
    out["bounded_per_trial"] = {k: med(t["b_" + k], 4) for k in STAGES}
    out["quality_over_plain"] = round(out["quality_s"] / out["plain_s"], 3)
    out["compare_ratio"] = round(out["per_trial"]["compare_ms"] / out["bounded_per_trial"]["compare_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,1024")
    ap.add_argument("--tols", default="1e-3,1e-7")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seg", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from waverange_amd import api
    api.set_verbosity(0)
    res = {"argv": sys.argv[1:], "seg": a.seg or api.SEG_DEFAULT, "reps": a.reps, "rows": {}}

    def emit():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                json.dump(res, fh, indent=1)
                fh.write("\n")

    with api.Context(0) as ctx:
        for n in [int(v) for v in a.sizes.split(",")]:
            f = api.pinned_array((n, n, n))
            buf = ctx.alloc(f.nbytes)
            ctx.synth_field(buf, n, n, n, 2024)
            f.reshape(-1)[:] = buf.download(np.float64, f.size)
            buf.free()
            absmax = float(max(abs(f.min()), abs(f.max())))
            for tol in [float(v) for v in a.tols.split(",")]:
                key = "%d^3 tol %g" % (n, tol)
                res["rows"][key] = row(api, ctx, f, absmax, tol, a.reps, a.seg)
                emit()
                print(key, "done", file=sys.stderr, flush=True)
            del f
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
