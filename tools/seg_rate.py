#!/usr/bin/env python3
"""One field alone, host buffer to host buffer: the reference-format pair against the segmented pair.

  encode_host + decode_host          the reference's stream: one host coder thread per plane (what bench.py's single_field times)
  encode_host_seg + decode_host_seg  segmented plane streams ("WRS1"), coded and decoded by the GPU

Both on the same pinned buffers, interleaved in one process, --reps repetitions after a warm-up, medians of the wall time
around each call; plus the coded bytes of both formats and the segmented calls' own coder time (wr_timings.rangecoder: the
coder kernels and the compaction).  The reconstructions are checked equal bit for bit.

    python tools/seg_rate.py [--sizes 512,1024] [--tols 1e-3,1e-7] [--reps 5] [--seg 0] [--seg-only]

--seg-only skips the reference-format pair (for a kernel trace of the segmented path).  Prints one JSON object."""
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


def med(v):
    return round(float(np.median(v)), 4)


def run(api, n, tols, reps, seg, seg_only):
    shape = (n, n, n)
    fld = api.pinned_array(shape)
    rec, rec_seg = api.pinned_array(shape), api.pinned_array(shape)
    out = {}
    with api.Context(0) as ctx:
        buf = ctx.alloc(fld.nbytes)
        ctx.synth_field(buf, n, n, n, 2024)
        fld.reshape(-1)[:] = buf.download(np.float64, fld.size)
        buf.free()
        coded = api.pinned_array((ctx._seg_cap(shape, seg),), np.uint8)
        for tol in tols:
            t = {k: [] for k in ("enc", "dec", "enc_seg", "dec_seg", "coder_enc", "coder_dec")}
            ref_bytes = seg_bytes = nlay = 0
            same = True
            for r in range(reps + 1):  # the first round warms up (allocations, code objects, clocks)
                if not seg_only:
                    te, (e, _) = timed(ctx.encode_host, fld, tol, out=coded)
                    e["data"] = e["data"].copy()
                    td, _ = timed(ctx.decode_host, rec, e)
                    ref_bytes = int(e["ntot_enc"])
                ts, (s, tm_e) = timed(ctx.encode_host_seg, fld, tol, 1, seg, out=coded)
                tu, tm_d = timed(ctx.decode_host_seg, rec_seg, s)
                seg_bytes, nlay = int(s["ntot_enc"]), int(s["nlay"])
                if r:
                    if not seg_only:
                        t["enc"].append(te); t["dec"].append(td)
                    t["enc_seg"].append(ts); t["dec_seg"].append(tu)
                    t["coder_enc"].append(tm_e["rangecoder"]); t["coder_dec"].append(tm_d["rangecoder"])
                elif not seg_only:
                    same = bool(np.array_equal(rec.reshape(-1).view(np.uint64), rec_seg.reshape(-1).view(np.uint64)))
            row = {"nlay": nlay, "seg_bytes": seg_bytes, "enc_seg_s": med(t["enc_seg"]), "dec_seg_s": med(t["dec_seg"]),
                   "coder_kernels_enc_s": med(t["coder_enc"]), "coder_kernels_dec_s": med(t["coder_dec"]),
                   "seg_round_trip_GBps": round(2 * fld.nbytes / (med(t["enc_seg"]) + med(t["dec_seg"])) / 1e9, 3)}
            if not seg_only:
                row.update({"ref_bytes": ref_bytes, "bytes_ratio": round(seg_bytes / ref_bytes, 5), "enc_s": med(t["enc"]), "dec_s": med(t["dec"]),
                            "ref_round_trip_GBps": round(2 * fld.nbytes / (med(t["enc"]) + med(t["dec"])) / 1e9, 3),
                            "speedup_round_trip": round((med(t["enc"]) + med(t["dec"])) / (med(t["enc_seg"]) + med(t["dec_seg"])), 2),
                            "reconstructions_bit_identical": same})
            out["%g" % tol] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,1024")
    ap.add_argument("--tols", default="1e-3,1e-7")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seg", type=int, default=0)
    ap.add_argument("--seg-only", action="store_true")
    a = ap.parse_args()
    from waverange_amd import api
    api.set_verbosity(0)
    res = {"seg": a.seg or api.SEG_DEFAULT, "reps": a.reps}
    for n in (int(v) for v in a.sizes.split(",")):
        res["%d^3" % n] = run(api, n, [float(v) for v in a.tols.split(",")], a.reps, a.seg, a.seg_only)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
