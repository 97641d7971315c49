#!/usr/bin/env python3
"""One field alone, pinned to pinned: stranded segments ("WRS3") at K = 1 .. 32 against WRS1 and WRS2 in the same run.

  encode_host_seg / decode_host_seg   every variant in turn inside each repetition, the same field and pinned buffers
  decode_host_seg_roi                 level 0, the centred cube of 32 samples
  decode_host_seg_lowres              level 2

All in one process, --reps repetitions after a warm-up round, medians.  Per variant: coded bytes against WRS1's, the coder
kernels' time of the encode and of the decode (wr_timings.rangecoder: all planes, compaction included) and per plane, the
wall time of the round trip, of the region and of the level-2 decode with their coder-kernel times.  Every reconstruction,
region and box is checked equal, bit for bit, to the WRS1 stream's in the warm-up round, and the run ends with an error and
no result where one differs.  The yardstick for a WRS3 row is
the WRS1 / WRS2 row of the same run.

    python tools/strands_rate.py [--sizes 512,1024] [--tols 1e-3,1e-7] [--reps 5] [--seg 0] [--strands 1,2,4,8,16,32]

Prints one JSON object."""
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


def med(v, digits=4):
    return round(float(np.median(v)), digits)


def same_bits(a, b):
    return bool(np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)))


def run(api, n, tols, reps, seg, strands):
    shape = (n, n, n)
    fld, rec, rec_ref = api.pinned_array(shape), api.pinned_array(shape), api.pinned_array(shape)
    cube = ((n // 2 - 16, n // 2 + 16),) * 3
    variants = [("wrs1", dict()), ("wrs2", dict(brick=0))] + [("wrs3_k%d" % k, dict(strands=k)) for k in strands]
    variants.append(("wrs3_k%d_blocked" % api.STRANDS_DEFAULT, dict(brick=api.BRICK_DEFAULT, strands=0)))
    out = {}
    with api.Context(0) as ctx:
        buf = ctx.alloc(fld.nbytes)
        ctx.synth_field(buf, n, n, n, 2024)
        fld.reshape(-1)[:] = buf.download(np.float64, fld.size)
        buf.free()
        coded = api.pinned_array((ctx._seg_cap(shape, seg, 0, max(strands)),), np.uint8)  # one buffer, every variant in turn
        roi_out, roi_ref = api.pinned_array(api.roi_shape(cube)), api.pinned_array(api.roi_shape(cube))
        low_out, low_ref = api.pinned_array(api.lowres_shape(shape, 2)), api.pinned_array(api.lowres_shape(shape, 2))
        for tol in tols:
            t = {name: {k: [] for k in ("encode_s", "decode_s", "enc_coder_s", "dec_coder_s", "roi32_s", "roi32_coder_s", "lowres2_s", "lowres2_coder_s")}
                 for name, _ in variants}
            row = {name: {} for name, _ in variants}
            for rep in range(reps + 1):  # the first round warms up (allocations, code objects, clocks) and checks the bits
                for name, kw in variants:
                    dt_e, (enc, tm_e) = timed(ctx.encode_host_seg, fld, tol, 1, seg, out=coded, **kw)
                    dt_d, tm_d = timed(ctx.decode_host_seg, rec, enc)
                    dt_r, tm_r = timed(ctx.decode_host_seg_roi, roi_out, shape, 0, cube, enc)
                    dt_l, tm_l = timed(ctx.decode_host_seg_lowres, low_out, shape, 2, enc)
                    if not rep:
                        if name == "wrs1":
                            rec_ref[:], roi_ref[:], low_ref[:] = rec, roi_out, low_out
                        same = {"reconstruction": same_bits(rec, rec_ref), "region": same_bits(roi_out, roi_ref), "level 2": same_bits(low_out, low_ref)}
                        if not all(same.values()):  # no timings from a run that computed something else
                            raise SystemExit("strands_rate: %d^3 tol %g %s differs from WRS1's: %s" % (n, tol, name, ", ".join(k for k, v in same.items() if not v)))
                        row[name].update(coded_bytes=int(enc["ntot_enc"]), nlay=int(enc["nlay"]), same_bits=True)
                        continue
                    for key, v in (("encode_s", dt_e), ("decode_s", dt_d), ("enc_coder_s", tm_e["rangecoder"]), ("dec_coder_s", tm_d["rangecoder"]),
                                   ("roi32_s", dt_r), ("roi32_coder_s", tm_r["rangecoder"]), ("lowres2_s", dt_l), ("lowres2_coder_s", tm_l["rangecoder"])):
                        t[name][key].append(v)
            base = row["wrs1"]["coded_bytes"]
            for name, _ in variants:
                r = row[name]
                r.update({k: med(v) for k, v in t[name].items()})
                r["bytes_over_wrs1"] = round(r["coded_bytes"] / base, 4)
                r["round_trip_s"] = round(r["encode_s"] + r["decode_s"], 4)
                r["dec_coder_ms_per_plane"] = round(1e3 * r["dec_coder_s"] / max(r["nlay"], 1), 2)
                r["enc_coder_ms_per_plane"] = round(1e3 * r["enc_coder_s"] / max(r["nlay"], 1), 2)
                r["roi32_over_full_decode"] = round(r["roi32_s"] / r["decode_s"], 3)
            out["%g" % tol] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,1024")
    ap.add_argument("--tols", default="1e-3,1e-7")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seg", type=int, default=0)
    ap.add_argument("--strands", default="1,2,4,8,16,32")
    a = ap.parse_args()
    from waverange_amd import api
    api.set_verbosity(0)
    strands = [int(v) for v in a.strands.split(",")]
    res = {"seg": a.seg or api.SEG_DEFAULT, "brick_of_wrs2": api.BRICK_DEFAULT, "reps": a.reps, "strands": strands}
    for n in (int(v) for v in a.sizes.split(",")):
        res["%d^3" % n] = run(api, n, [float(v) for v in a.tols.split(",")], a.reps, a.seg, strands)
        print("%d^3 done" % n, file=sys.stderr, flush=True)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
