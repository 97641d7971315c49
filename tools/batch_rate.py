#!/usr/bin/env python3
"""N small same-shaped fields, pinned to pinned: ONE batch call against a loop of N single-field calls, in the same run.

  encode_host_seg_batch / decode_host_seg_batch   plane l of all N fields in one coder launch
  encode_host_seg / decode_host_seg               the same fields one after the other: the yardstick of the row above

All in one process.  Per (size, tolerance, N, format) the two are interleaved inside each repetition; --reps repetitions after
a warm-up round, medians.  In the warm-up round every field's coded bytes and reconstruction from the batch are compared with
the single call's, and the run ends with an error and no result where one differs.  Recorded per row: wall time of encode
and decode, the coder kernels' time (wr_timings.rangecoder) and per plane index (plane_coder_s; for the loop of singles the
sum over the fields), and GB/s of field data.  WRS1 always; WRS2 at brick 32 once (--wrs2-at).  There is no gate.

    python tools/batch_rate.py [--sizes 64,128,256] [--counts 1,8,64] [--tols 1e-3,1e-7] [--reps 5] [--seg 0]
                               [--wrs2-at 128,8,1e-3] [--out profiles/batch/batch_rate.json]

--strands K measures the batch calls for WRS3 instead.  Per (size, tolerance, N), in the same process and inside each repetition:

  wrs3_batch     encode_host_seg_batch_strands, then decode_host_seg_batch_mixed on its streams (one coder launch)
  wrs1_batch     encode_host_seg_batch and decode_host_seg_batch: the yardstick of the new encode, and of the line below
  wrs1_mixed     decode_host_seg_batch_mixed on those same WRS1 streams (one launch where the line above makes one per plane index)
  wrs3_singles   a loop of N encode_host_seg(strands=K) / decode_host_seg calls: the yardstick of the batching

The warm-up round compares every field's bytes and reconstruction with the single call's.  The yardsticks are rows of the same
run, never figures printed elsewhere.

Prints one JSON object (and rewrites --out after every row, so that a run that is cut short leaves what it measured)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DISTINCT = 8  # fields made per size; a batch of more cycles through them (inputs are only read)


def timed(fn, *a, **k):
    t0 = time.perf_counter()
    r = fn(*a, **k)
    return time.perf_counter() - t0, r


def med(v, digits=5):
    return round(float(np.median(v)), digits)


def same_bits(a, b):
    return bool(np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)))


def row(api, ctx, fields, recs, tol, count, reps, seg, brick):
    fs = [fields[i % len(fields)] for i in range(count)]
    outs = recs[:count]
    field_gb = count * fs[0].nbytes / 1e9
    keys = ("encode_s", "decode_s", "enc_coder_s", "dec_coder_s")
    t = {who: {k: [] for k in keys} for who in ("batch", "singles")}
    planes = {who: {"enc": [], "dec": []} for who in ("batch", "singles")}
    coded = None
    info = {}
    for rep in range(reps + 1):  # the first round warms up (allocations, code objects, clocks) and checks the bits
        # ---- the loop of singles
        dt_e = dt_d = ce = cd = 0.0
        pe, pd = np.zeros(api.NLAYMAX), np.zeros(api.NLAYMAX)
        singles = []
        for i, f in enumerate(fs):
            dt, (enc, tm) = timed(ctx.encode_host_seg, f, tol, 1, seg, out=None if coded is None else coded[i], brick=brick)
            dt_e += dt; ce += tm["rangecoder"]; pe += np.array(tm["plane_coder_s"])
            if not rep:
                enc["data"] = enc["data"].copy()
            singles.append(enc)
            dt, tm = timed(ctx.decode_host_seg, outs[i], enc)
            dt_d += dt; cd += tm["rangecoder"]; pd += np.array(tm["plane_coder_s"])
        if not rep:
            want = [o.copy() for o in outs[:min(count, len(fields))]]
            for o in outs:
                o[:] = 0
        else:
            for k, v in zip(keys, (dt_e, dt_d, ce, cd)):
                t["singles"][k].append(v)
            planes["singles"]["enc"].append(pe); planes["singles"]["dec"].append(pd)
        # ---- the batch
        dt_e, (encs, tm_e) = timed(ctx.encode_host_seg_batch, fs, tol, 1, seg, brick, outs=coded)
        dt_d, tm_d = timed(ctx.decode_host_seg_batch, outs, encs)
        if not rep:
            for i in range(count):
                ok = (encs[i]["len_enc_vec"] == singles[i]["len_enc_vec"] and np.array_equal(encs[i]["data"], singles[i]["data"])
                      and same_bits(outs[i], want[i % len(want)]))
                if not ok:  # no timings from a run that computed something else
                    raise SystemExit("batch_rate: field %d of %d (%s, tol %g, brick %s) differs from the single call's" % (i, count, fs[0].shape, tol, brick))
            info = dict(fields=count, field_gb=round(field_gb, 4), nlay=[int(e["nlay"]) for e in encs[:len(fields)]],
                        coded_bytes=int(sum(e["ntot_enc"] for e in encs)), same_bits=True,
                        device_bytes_formula=api.seg_batch_device_bytes(count, fs[0].size, max(e["nlay"] for e in encs), seg, brick or 0))
            # from here on both sides write into the same pinned buffers, sized by what the warm-up round produced
            coded = [api.pinned_array((max(int(e["ntot_enc"]), 16),), np.uint8) for e in encs]
            continue
        for k, v in zip(keys, (dt_e, dt_d, tm_e["rangecoder"], tm_d["rangecoder"])):
            t["batch"][k].append(v)
        planes["batch"]["enc"].append(np.array(tm_e["plane_coder_s"])); planes["batch"]["dec"].append(np.array(tm_d["plane_coder_s"]))
    out = dict(info)
    for who in ("batch", "singles"):
        r = {k: med(v) for k, v in t[who].items()}
        r["encode_gb_s"] = round(field_gb / r["encode_s"], 3)
        r["decode_gb_s"] = round(field_gb / r["decode_s"], 3)
        r["enc_plane_coder_ms"] = [round(1e3 * float(v), 3) for v in np.median(np.array(planes[who]["enc"]), axis=0)]
        r["dec_plane_coder_ms"] = [round(1e3 * float(v), 3) for v in np.median(np.array(planes[who]["dec"]), axis=0)]
        out[who] = r
    out["singles_over_batch"] = {k: round(out["singles"][k] / out["batch"][k], 2) if out["batch"][k] else None for k in keys}
    return out


def strand_row(api, ctx, fields, recs, tol, count, reps, seg, K):
    fs = [fields[i % len(fields)] for i in range(count)]
    outs = recs[:count]
    field_gb = count * fs[0].nbytes / 1e9
    whos = ("wrs3_batch", "wrs1_batch", "wrs1_mixed", "wrs3_singles")
    t = {who: {"encode_s": [], "decode_s": [], "enc_coder_s": [], "dec_coder_s": []} for who in whos}
    coded3 = coded1 = None
    info = {}
    for rep in range(reps + 1):  # the first round warms up and checks the bits
        # ---- the loop of single WRS3 calls
        dt_e = dt_d = ce = cd = 0.0
        singles = []
        for i, f in enumerate(fs):
            dt, (enc, tm) = timed(ctx.encode_host_seg, f, tol, 1, seg, out=None if coded3 is None else coded3[i], strands=K)
            dt_e += dt; ce += tm["rangecoder"]
            if not rep:
                enc["data"] = enc["data"].copy()
            singles.append(enc)
            dt, tm = timed(ctx.decode_host_seg, outs[i], enc)
            dt_d += dt; cd += tm["rangecoder"]
        if not rep:
            want = [o.copy() for o in outs[:min(count, len(fields))]]
        else:
            for k, v in zip(("encode_s", "decode_s", "enc_coder_s", "dec_coder_s"), (dt_e, dt_d, ce, cd)):
                t["wrs3_singles"][k].append(v)

        def check(encs, ref, what):
            for i in range(count):
                if ref is not None and not (encs[i]["len_enc_vec"] == ref[i]["len_enc_vec"] and np.array_equal(encs[i]["data"], ref[i]["data"])):
                    raise SystemExit("batch_rate: %s: field %d of %d (%s, tol %g) has other bytes than the single call's" % (what, i, count, fs[0].shape, tol))
                if not same_bits(outs[i], want[i % len(want)]):
                    raise SystemExit("batch_rate: %s: field %d of %d (%s, tol %g) is reconstructed differently" % (what, i, count, fs[0].shape, tol))

        def wipe():
            if not rep:
                for o in outs:
                    o[:] = 0

        # ---- the strand batch and the mixed decode of its streams
        wipe()
        dt_e, (encs3, tm_e) = timed(ctx.encode_host_seg_batch_strands, fs, tol, 1, seg, 0, K, outs=coded3)
        dt_d, tm_d = timed(ctx.decode_host_seg_batch_mixed, outs, encs3)
        if not rep:
            check(encs3, singles, "wrs3_batch")
        else:
            for k, v in zip(("encode_s", "decode_s", "enc_coder_s", "dec_coder_s"), (dt_e, dt_d, tm_e["rangecoder"], tm_d["rangecoder"])):
                t["wrs3_batch"][k].append(v)
        # ---- the WRS1 batch calls, and the mixed decode on the same WRS1 streams
        wipe()
        dt_e, (encs1, tm_e) = timed(ctx.encode_host_seg_batch, fs, tol, 1, seg, None, outs=coded1)
        dt_d, tm_d = timed(ctx.decode_host_seg_batch, outs, encs1)
        if not rep:
            check(encs1, None, "wrs1_batch")  # (the same quantized planes, so the same reconstruction)
        else:
            for k, v in zip(("encode_s", "decode_s", "enc_coder_s", "dec_coder_s"), (dt_e, dt_d, tm_e["rangecoder"], tm_d["rangecoder"])):
                t["wrs1_batch"][k].append(v)
        wipe()
        dt_d, tm_d = timed(ctx.decode_host_seg_batch_mixed, outs, encs1)
        if not rep:
            check(encs1, None, "wrs1_mixed")
            nlay = max(int(e["nlay"]) for e in encs3)
            info = dict(fields=count, field_gb=round(field_gb, 4), strands=K, nlay=[int(e["nlay"]) for e in encs3[:len(fields)]],
                        coded_bytes_wrs3=int(sum(e["ntot_enc"] for e in encs3)), coded_bytes_wrs1=int(sum(e["ntot_enc"] for e in encs1)), same_bits=True,
                        device_bytes_formula=api.seg_batch_device_bytes_strands(count, fs[0].size, nlay, seg, 0, K),
                        device_bytes_formula_decode=api.seg_batch_device_bytes_strands(count, fs[0].size, nlay, seg, 0, K, True))
            coded3 = [api.pinned_array((max(int(e["ntot_enc"]), 16),), np.uint8) for e in encs3]
            coded1 = [api.pinned_array((max(int(e["ntot_enc"]), 16),), np.uint8) for e in encs1]
            continue
        t["wrs1_mixed"]["decode_s"].append(dt_d); t["wrs1_mixed"]["dec_coder_s"].append(tm_d["rangecoder"])
    out = dict(info)
    for who in whos:
        out[who] = {k: med(v) for k, v in t[who].items() if v}
    ratio = lambda a, b, k: round(out[a][k] / out[b][k], 2) if out[b].get(k) else None
    out["wrs1_batch_over_wrs3_batch"] = {k: ratio("wrs1_batch", "wrs3_batch", k) for k in ("encode_s", "decode_s", "enc_coder_s", "dec_coder_s")}
    out["wrs3_singles_over_wrs3_batch"] = {k: ratio("wrs3_singles", "wrs3_batch", k) for k in ("encode_s", "decode_s", "enc_coder_s", "dec_coder_s")}
    out["wrs1_batch_over_wrs1_mixed"] = {k: ratio("wrs1_batch", "wrs1_mixed", k) for k in ("decode_s", "dec_coder_s")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,128,256")
    ap.add_argument("--counts", default="1,8,64")
    ap.add_argument("--tols", default="1e-3,1e-7")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seg", type=int, default=0)
    ap.add_argument("--wrs2-at", default="128,8,1e-3", help="size,count,tol of the one WRS2 (brick 32) row; empty: none")
    ap.add_argument("--strands", type=int, default=None, help="K: measure the batch calls for WRS3 (0: the default strand count)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from waverange_amd import api
    api.set_verbosity(0)
    sizes, counts = [int(v) for v in a.sizes.split(",")], [int(v) for v in a.counts.split(",")]
    tols = [float(v) for v in a.tols.split(",")]
    wrs2 = a.wrs2_at.split(",") if a.wrs2_at else None
    res = {"argv": sys.argv[1:], "seg": a.seg or api.SEG_DEFAULT, "reps": a.reps, "distinct_fields": DISTINCT, "rows": {}}

    def emit():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                json.dump(res, fh, indent=1)
                fh.write("\n")

    with api.Context(0) as ctx:
        for n in sizes:
            shape = (n, n, n)
            fields = [api.pinned_array(shape) for _ in range(min(DISTINCT, max(counts)))]
            buf = ctx.alloc(fields[0].nbytes)
            for i, f in enumerate(fields):
                ctx.synth_field(buf, n, n, n, 2024 + i)
                f.reshape(-1)[:] = buf.download(np.float64, f.size)
            buf.free()
            recs = [api.pinned_array(shape) for _ in range(max(counts))]
            for tol in tols:
                for count in counts:
                    key = "%d^3 tol %g N=%d" % (n, tol, count)
                    if a.strands is not None:
                        res["rows"][key + " K=%d" % (a.strands or api.STRANDS_DEFAULT)] = strand_row(api, ctx, fields, recs, tol, count, a.reps, a.seg, a.strands)
                        emit()
                        print(key, "done", file=sys.stderr, flush=True)
                        continue
                    res["rows"][key + " wrs1"] = row(api, ctx, fields, recs, tol, count, a.reps, a.seg, None)
                    emit()
                    print(key, "done", file=sys.stderr, flush=True)
                    if wrs2 and (n, count, tol) == (int(wrs2[0]), int(wrs2[1]), float(wrs2[2])):
                        res["rows"][key + " wrs2 brick 32"] = row(api, ctx, fields, recs, tol, count, a.reps, a.seg, 32)
                        emit()
            del fields, recs
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
