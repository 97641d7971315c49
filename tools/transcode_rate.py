#!/usr/bin/env python3
"""Transcoding a coded field against the only conversion there was: decode the field, encode it again.

  transcode   Context.transcode of the source stream into the target format (wr_transcode_host: the planes are decoded and coded,
              nothing else)
  yardstick   inside the same repetition, decode_host / decode_host_seg of the source stream into a pinned field, then the
              target format's encode_host / encode_host_seg of that field at the same tolerance

Pairs: ref->wrs3, wrs3->ref, wrs1->wrs3, wrs1->wrs2, all at the formats' defaults.  One process, pinned field and stream buffers,
--reps repetitions after a warm-up round; medians of the wall time around each call and of the calls' own wr_timings.  In the
warm-up round every transcode's bytes and header are compared with the direct encode of the ORIGINAL field in the target format
(a difference ends the run), and whether the yardstick's bytes equal them is recorded: the yardstick codes the reconstruction,
which is quantized a second time with its own min / max -- that is the finding on re-quantization, not a failure.

    python tools/transcode_rate.py [--sizes 512,1024] [--tols 1e-3,1e-7] [--reps 5] [--pairs ref:wrs3,wrs3:ref,wrs1:wrs3,wrs1:wrs2] [--out FILE]

Prints one JSON object (and writes it to FILE)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ENCODE_KW = {"wrs1": {}, "wrs2": {"brick": 0}, "wrs3": {"strands": 0}}


def med(v, digits=4):
    return round(float(np.median(v)), digits)


def encode(ctx, fmt, f, tol, out):
    if fmt == "ref":
        return ctx.encode_host(f, tol, out=out)
    return ctx.encode_host_seg(f, tol, out=out, **ENCODE_KW[fmt])


def decode(ctx, fmt, out, enc):
    return (ctx.decode_host if fmt == "ref" else ctx.decode_host_seg)(out, enc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,1024")
    ap.add_argument("--tols", default="1e-3,1e-7")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pairs", default="ref:wrs3,wrs3:ref,wrs1:wrs3,wrs1:wrs2")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from waverange_amd import api
    api.set_verbosity(0)
    pairs = [tuple(p.split(":")) for p in a.pairs.split(",")]
    result = dict(tool="transcode_rate", reps=a.reps, rows=[])
    with api.Context(0) as ctx:
        for size in (int(s) for s in a.sizes.split(",")):
            shape = (size, size, size)
            n = size ** 3
            f = api.pinned_array(shape)
            buf = ctx.alloc(f.nbytes)
            ctx.synth_field(buf, size, size, size, 2024)
            f.reshape(-1)[:] = buf.download(np.float64, f.size)
            buf.free()
            rec = api.pinned_array(shape)
            for tol in (float(t) for t in a.tols.split(",")):
                formats = sorted({p[0] for p in pairs} | {p[1] for p in pairs})
                direct = {}
                for fmt in formats:  # the direct encodes of the original field: the sources, and what every transcode must equal
                    enc, _ = encode(ctx, fmt, f, tol, None)
                    data = api.pinned_array((max(enc["ntot_enc"], 1),), np.uint8)[:enc["ntot_enc"]]
                    data[...] = enc["data"]
                    direct[fmt] = dict(enc, data=data)
                    del enc
                # (any cap that holds the bytes produced will do; the yardstick codes other planes, so it gets room to spare)
                cap = 2 * max(d["ntot_enc"] for d in direct.values()) + (1 << 20)
                assert all(api.transcode_bound(n, direct[fmt]["nlay"], fmt) >= direct[fmt]["ntot_enc"] for fmt in formats)
                out_t, out_y = api.pinned_array((cap,), np.uint8), api.pinned_array((cap,), np.uint8)
                for src, dst in pairs:
                    s = direct[src]
                    row = dict(size=size, tol=tol, pair="%s->%s" % (src, dst), nlay=s["nlay"], bytes_in=s["ntot_enc"], bytes_out=direct[dst]["ntot_enc"])
                    wall_t, wall_y, wall_yd, wall_ye, tms = [], [], [], [], []
                    for rep in range(a.reps + 1):
                        tm = {}
                        t0 = time.perf_counter()
                        data, info = ctx.transcode(s, s["data"], dst, shape=shape, out=out_t, timings=tm)
                        t1 = time.perf_counter()
                        decode(ctx, src, rec, s)
                        t2 = time.perf_counter()
                        yenc, _ = encode(ctx, dst, rec, tol, out_y)
                        t3 = time.perf_counter()
                        if rep == 0:  # warm-up round: the checks
                            want = direct[dst]
                            same = data.size == want["data"].size and np.array_equal(data, want["data"]) and info["len_enc_vec"] == [int(v) for v in want["len_enc_vec"]]
                            if not same:
                                raise SystemExit("transcode %s->%s at %d^3 tol %g differs from the direct encode" % (src, dst, size, tol))
                            row["transcode_equals_direct_encode"] = True
                            row["yardstick_equals_direct_encode"] = bool(yenc["data"].size == want["data"].size and np.array_equal(yenc["data"], want["data"]))
                            row["yardstick_bytes_out"] = int(yenc["ntot_enc"])
                            row["yardstick_nlay"] = int(yenc["nlay"])
                            continue
                        wall_t.append(t1 - t0); wall_yd.append(t2 - t1); wall_ye.append(t3 - t2); wall_y.append(t3 - t1)
                        tms.append(tm)
                    row.update(transcode_s=med(wall_t), yardstick_s=med(wall_y), yardstick_decode_s=med(wall_yd), yardstick_encode_s=med(wall_ye),
                               speedup=round(float(np.median(wall_y) / np.median(wall_t)), 2),
                               transcode_coders_s=med([t["rangecoder"] for t in tms]), transcode_gpu_s=med([t["gpu"] for t in tms]),
                               transcode_h2d_ms=med([t["h2d_ms"] for t in tms], 2), transcode_d2h_ms=med([t["d2h_ms"] for t in tms], 2),
                               plane_coder_s=[med([t["plane_coder_s"][l] for t in tms]) for l in range(s["nlay"])])
                    result["rows"].append(row)
                    print(json.dumps(row), file=sys.stderr, flush=True)
                del direct, out_t, out_y
            del f, rec
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
