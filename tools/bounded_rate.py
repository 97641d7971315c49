#!/usr/bin/env python3
"""Encode to a pointwise error bound against the plain segmented encode at the tolerance it returns, in the same run.

  encode_host_seg_bounded(f, M)                  the search (trials on the device), every plane coded once
  encode_host_seg(f, budget_tol(g))              the existing call at the tolerance the search chose: the yardstick

Per size and nominal tolerance the bound is M = tol * max|f|.  The two calls are interleaved inside each repetition; --reps
repetitions after a warm-up round in which the bounded call's bytes are compared with the plain call's and its error with
seg_error_host of the stream (the run ends with an error where they differ); medians.  Recorded per row: wall time of both and
their ratio, the grid point, the error reached and its ratio to the bound, the trials, the planes coded (the counter
WR_STAT_BOUNDED_CODER_RUNS), and the time of one trial's three stages -- the coefficient sum (requant_accum), the inverse
transform, the compare -- as HIP-event milliseconds summed over the call's trials and divided by their number.  There is no gate.

    python tools/bounded_rate.py [--sizes 512,1024] [--tols 1e-3,1e-7] [--reps 5] [--seg 0] [--out profiles/bounded/bounded_rate.json]

Prints one JSON object (and rewrites --out after every row)."""
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


def med(v, digits=5):
    return round(float(np.median(v)), digits)


def row(api, ctx, f, absmax, tol, reps, seg):
    bound = tol * absmax
    t = {"bounded": [], "plain": [], "requant_ms": [], "inverse_ms": [], "compare_ms": []}
    info = {}
    for rep in range(reps + 1):  # the first round warms up and checks the bytes
        before = api.stat(api.STAT_BOUNDED_CODER_RUNS)
        dt_b, (enc, data, res) = timed(ctx.encode_host_seg_bounded, f, bound, seg=seg)
        runs = api.stat(api.STAT_BOUNDED_CODER_RUNS) - before
        stage = ctx.bounded_trial_ms()
        dt_p, (plain, _) = timed(ctx.encode_host_seg, f, res["tolrel"], 1, seg)
        if not rep:
            if not (np.array_equal(data, plain["data"]) and enc["len_enc_vec"] == plain["len_enc_vec"] and runs == enc["nlay"]):
                raise SystemExit("bounded_rate: the bounded call's stream differs from the plain call's at tol %g" % res["tolrel"])
            measured = ctx.seg_error_host(f, enc)
            if measured != res["err"] or not measured <= bound:
                raise SystemExit("bounded_rate: the error of the stream is %r, the call said %r for the bound %r" % (measured, res["err"], bound))
            info = dict(bound=bound, nominal_tol=tol, start=api.bounded_start(bound, absmax), g=res["g"], tolrel=res["tolrel"], err=res["err"],
                        err_over_bound=round(res["err"] / bound, 6), trials=res["trials"], nlay=int(enc["nlay"]), ntot_enc=int(enc["ntot_enc"]),
                        coder_runs=int(runs), same_bytes=True)
            continue
        t["bounded"].append(dt_b); t["plain"].append(dt_p)
        for k, v in zip(("requant_ms", "inverse_ms", "compare_ms"), stage):
            t[k].append(v / max(res["trials"], 1))
    out = dict(info)
    out["bounded_s"], out["plain_s"] = med(t["bounded"]), med(t["plain"])
    out["per_trial"] = {k: med(t[k], 4) for k in ("requant_ms", "inverse_ms", "compare_ms")}
    out["bounded_over_plain"] = round(out["bounded_s"] / out["plain_s"], 3)
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
