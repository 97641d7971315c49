#!/usr/bin/env python3
"""Q probes of one snapshot: one multi-region decode against Q single-region decodes against the full decode.

  decode_host_seg             the whole field
  decode_host_seg_roi  x Q    level 0, all planes, one probe of 32^3 per call (the yardstick of the multi row of the same run)
  wr_decode_host_seg_roi_multi   the same Q probes in one call

Probes sit on a seeded choice of the cells of a 4 x 4 x 4 grid over the field, Q = 1, 8 and 64.  All on the same WRS1 stream and
pinned buffers, interleaved in one process, --reps repetitions after a warm-up round in which every region of the multi call is
checked bit-equal to the single call's; medians of the wall time around each call (for the single calls: around all Q), and of
the calls' own stage times (wr_timings; summed over the Q single calls), with the segments launched, the payload bytes uploaded
and the coder launches (wr_stat).

    python tools/roi_multi_rate.py [--sizes 512,1024] [--tols 1e-3,1e-7] [--reps 5] [--seg 0] [--probe 32] [--out FILE]

Prints one JSON object (and writes it to FILE)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QS = (1, 8, 64)


def med(v, digits=4):
    return round(float(np.median(v)), digits)


def probes(n, q, edge, seed=2026):
    """q probes of edge^3, each centred in its own cell of a 4 x 4 x 4 grid; which cells: a seeded permutation"""
    cell = n // 4
    cells = np.random.default_rng(seed).permutation(64)[:q]
    out = []
    for c in cells:
        lo = [(int(c) >> (2 * k) & 3) * cell + (cell - edge) // 2 for k in range(3)]
        out.append(tuple((a, a + edge) for a in lo))
    return out


def counters(api):
    return np.array([api.stat(api.STAT_ROI_SEGMENTS), api.stat(api.STAT_ROI_BYTES_UP), api.stat(api.STAT_ROI_CODER_LAUNCHES)], dtype=np.int64)


STAGES = (("up_ms", "h2d_ms", 1.0), ("decoder_kernels_ms", "rangecoder", 1e3), ("dequant_ms", "quant_ms", 1.0), ("inverse_ms", "transform_ms", 1.0),
          ("down_ms", "d2h_ms", 1.0))


def stage_sum(ms):
    """the stage times of one repetition: summed over its calls"""
    return {k: sum(f * m[src] for m in ms) for k, src, f in STAGES}


def stage_medians(reps):
    out = {k: med([r[k] for r in reps], 2) for k, _, _ in STAGES}
    out["window_stage_ms"] = med([r["dequant_ms"] + r["inverse_ms"] for r in reps], 2)
    return out


def run(api, n, tols, reps, seg, edge):
    shape = (n, n, n)
    fld, rec = api.pinned_array(shape), api.pinned_array(shape)
    sets = {q: probes(n, q, edge) for q in QS}
    one = api.pinned_array((edge,) * 3)
    multi = {q: api.pinned_array((q * edge ** 3,)) for q in QS}
    fn = api.lib().wr_decode_host_seg_roi_multi
    out = {}
    with api.Context(0) as ctx:
        buf = ctx.alloc(fld.nbytes)
        ctx.synth_field(buf, n, n, n, 2024)
        fld.reshape(-1)[:] = buf.download(np.float64, fld.size)
        buf.free()
        coded = api.pinned_array((ctx._seg_cap(shape, seg),), np.uint8)
        for tol in tols:
            enc, _ = ctx.encode_host_seg(fld, tol, 1, seg, out=coded)
            t_full, tm_full = [], []
            t = {(q, how): [] for q in QS for how in ("multi", "single")}
            tm = {k: [] for k in t}
            stat, same = {}, {}
            for rep in range(reps + 1):  # the first round warms up (allocations, code objects, clocks) and checks the values
                t0 = time.perf_counter()
                m = ctx.decode_host_seg(rec, enc)
                if rep:
                    t_full.append(time.perf_counter() - t0); tm_full.append(stage_sum([m]))
                for q in QS:
                    rois = sets[q]
                    c0 = counters(api)
                    t0 = time.perf_counter()
                    m = ctx._decode_seg_rois(fn, multi[q].ctypes.data, shape, 0, rois, enc, 0)
                    dt = time.perf_counter() - t0
                    stat[q, "multi"] = counters(api) - c0
                    if rep:
                        t[q, "multi"].append(dt); tm[q, "multi"].append(stage_sum([m]))
                    ms, ok, dt = [], True, 0.0
                    c0 = counters(api)
                    for i, r in enumerate(rois):
                        t0 = time.perf_counter()
                        ms.append(ctx.decode_host_seg_roi(one, shape, 0, r, enc))
                        dt += time.perf_counter() - t0
                        if not rep:
                            ok = ok and np.array_equal(one.reshape(-1).view(np.uint64), multi[q][i * edge ** 3:(i + 1) * edge ** 3].view(np.uint64))
                    stat[q, "single"] = counters(api) - c0
                    if rep:
                        t[q, "single"].append(dt); tm[q, "single"].append(stage_sum(ms))
                    else:
                        same[q] = bool(ok)
            row = {"nlay": int(enc["nlay"]), "coded_bytes": int(enc["ntot_enc"]), "full": dict(seconds=med(t_full), **stage_medians(tm_full))}
            for q in QS:
                for how in ("single", "multi"):
                    k = (q, how)
                    rec_ = dict(seconds=med(t[k]), segments_launched=int(stat[k][0]), payload_bytes_up=int(stat[k][1]), coder_launches=int(stat[k][2]),
                                speedup_vs_full=round(med(t_full) / med(t[k]), 2), **stage_medians(tm[k]))
                    if how == "multi":
                        rec_["speedup_vs_single_calls"] = round(med(t[q, "single"]) / med(t[k]), 2)
                        rec_["every_region_equals_the_single_call"] = same[q]
                    row["Q%d_%s" % (q, how)] = rec_
            out["%g" % tol] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,1024")
    ap.add_argument("--tols", default="1e-3,1e-7")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seg", type=int, default=0)
    ap.add_argument("--probe", type=int, default=32)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from waverange_amd import api
    api.set_verbosity(0)
    res = {"seg": a.seg or api.SEG_DEFAULT, "reps": a.reps, "probe": a.probe, "Q": list(QS)}
    for n in (int(v) for v in a.sizes.split(",")):
        res["%d^3" % n] = run(api, n, [float(v) for v in a.tols.split(",")], a.reps, a.seg, a.probe)
    text = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
