#!/usr/bin/env python3
"""Encode to a byte budget against the plain segmented encode at the tolerance it returns, in the same run.

  encode_host_seg_budget(f, budget)              the search, every plane coded once
  encode_host_seg(f, budget_tol(g))              the existing call at the tolerance the search chose: the yardstick

Per size and tolerance regime the budget is what a plain encode at that tolerance takes (its ntot_enc plus 1 %), so the search
ends near that tolerance.  The two calls are interleaved inside each repetition; --reps repetitions after a warm-up round in
which the budget call's bytes are compared with the plain call's (the run ends with an error where they differ); medians.
Recorded per row: wall time and coder-kernel time of both, their ratio, probe_passes, the planes coded (the counter
WR_STAT_BUDGET_CODER_RUNS), the slack (B(g) - ntot_enc) / ntot_enc, and the time of one size-probe launch on the field's
array with 1, 4 and 8 candidate steps (wr_dev_quant_size_probe: whether the loads or the histograms bind it).  There is no gate.

    python tools/budget_rate.py [--sizes 512,1024] [--tols 1e-3,1e-7] [--reps 5] [--seg 0] [--out profiles/budget/budget_rate.json]

Prints one JSON object (and rewrites --out after every row)."""
import argparse
import ctypes as C
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


def probe_times(api, ctx, f, seg, reps):
    """milliseconds of one probe launch (upload excluded, the call's synchronisation included) for 1, 4 and 8 candidates"""
    lo, hi = float(f.min()), float(f.max())
    buf = ctx.to_device(f)
    out = {}
    try:
        for k in (1, 4, api.BUDGET_PROBE_MAX):
            deps = np.array([(hi - lo) / 255.0 * (1.0 + 0.37 * j) for j in range(k)])
            got = (C.c_size_t * k)()
            call = lambda: api._check(api.lib().wr_dev_quant_size_probe(ctx.h, buf.ptr, f.size, lo, k, deps.ctypes.data_as(api._dp), seg, got))
            call()
            out["candidates_%d_ms" % k] = med([1e3 * timed(call)[0] for _ in range(reps)], 4)
    finally:
        buf.free()
    return out


def row(api, ctx, f, tol, reps, seg):
    plain0, _ = ctx.encode_host_seg(f, tol, 1, seg)
    budget = int(plain0["ntot_enc"] * 1.01) + 1
    t = {who: {"encode_s": [], "coder_s": []} for who in ("budget", "plain")}
    info = {}
    for rep in range(reps + 1):  # the first round warms up and checks the bytes
        before = api.stat(api.STAT_BUDGET_CODER_RUNS)
        dt_b, (enc, data, res) = timed(ctx.encode_host_seg_budget, f, budget, 2.0 ** -60, 1, seg)
        runs = api.stat(api.STAT_BUDGET_CODER_RUNS) - before
        dt_p, (plain, tm_p) = timed(ctx.encode_host_seg, f, res["tolrel"], 1, seg)
        if not rep:
            if not (np.array_equal(data, plain["data"]) and enc["len_enc_vec"] == plain["len_enc_vec"] and runs == enc["nlay"]):
                raise SystemExit("budget_rate: the budget call's stream differs from the plain call's at tol %g" % res["tolrel"])
            info = dict(budget=budget, asked_tol=tol, g=res["g"], tolrel=res["tolrel"], nlay=int(enc["nlay"]), ntot_enc=int(enc["ntot_enc"]),
                        bound=int(res["bound"]), slack=round((res["bound"] - enc["ntot_enc"]) / enc["ntot_enc"], 6),
                        probe_passes=res["probe_passes"], coder_runs=int(runs), same_bytes=True)
            continue
        t["budget"]["encode_s"].append(dt_b); t["budget"]["coder_s"].append(res["timings"]["rangecoder"])
        t["plain"]["encode_s"].append(dt_p); t["plain"]["coder_s"].append(tm_p["rangecoder"])
    out = dict(info)
    for who in t:
        out[who] = {k: med(v) for k, v in t[who].items()}
    out["budget_over_plain"] = round(out["budget"]["encode_s"] / out["plain"]["encode_s"], 3)
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
    res = {"argv": sys.argv[1:], "seg": a.seg or api.SEG_DEFAULT, "reps": a.reps, "rows": {}, "probe": {}}

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
            res["probe"]["%d^3" % n] = probe_times(api, ctx, f, a.seg, a.reps)
            emit()
            for tol in [float(v) for v in a.tols.split(",")]:
                key = "%d^3 tol %g" % (n, tol)
                res["rows"][key] = row(api, ctx, f, tol, a.reps, a.seg)
                emit()
                print(key, "done", file=sys.stderr, flush=True)
            del f
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
