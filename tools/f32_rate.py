#!/usr/bin/env python3
"""fp32 fields on ONE GPU: the fp32 entry points against the fp64 ones on the same field (fp32-representable, widened).

  * wr_encode_host_f32 / wr_decode_host_f32 (4 bytes per sample over the bus, widened / narrowed in the transform kernels)
    against wr_encode_host / wr_decode_host on the widened field, 512^3 and 1024^3, tol 1e-3 and 1e-7: the calls' own
    timings (total, h2d_ms, d2h_ms, transform_ms), median of --reps calls on pinned buffers, one context, coder threads
    one per plane; the coded bytes and the narrowed reconstruction are checked equal.
  * wrenc + wrdec (waverange_amd/bin) wall time on an NF x n^3 PRECISION=1 raw file (default 8 x 512^3, tol 1e-5): the fp32
    records through wr_encoding_wrap_f32 / wr_decoding_wrap_f32, and the same binaries with WR_CLI_WIDEN_ON_HOST=1 (read
    into doubles, encoding_wrap / decoding_wrap, narrowed on write: the path before the fp32 entry points); the files are
    compared byte for byte.

    python tools/f32_rate.py [--sizes 512,1024] [--tols 1e-3,1e-7] [--reps 3] [--nf 8] [--cli-size 512] [--dir /tmp/wr_f32]

Prints one JSON object."""
import argparse
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BIN = os.path.join(ROOT, "waverange_amd", "bin")


def median_timings(calls):
    keys = ("total", "h2d_ms", "d2h_ms", "transform_ms")
    return {k: round(float(np.median([c[k] * (1e3 if k == "total" else 1.0) for c in calls])), 3) for k in keys}


def host_api(api, n, tols, reps):
    from waverange_amd import synth
    f32 = api.pinned_array((n, n, n), np.float32)
    f32[...] = synth.field(n, n, n)
    f64 = api.pinned_array((n, n, n), np.float64)
    f64[...] = f32
    out32 = api.pinned_array((n, n, n), np.float32)
    out64 = api.pinned_array((n, n, n), np.float64)
    res = {}
    with api.Context(0) as ctx:
        for tol in tols:
            row = {}
            t = {"enc32": [], "dec32": [], "enc64": [], "dec64": []}
            for r in range(reps + 1):  # the first round warms up (allocations, code objects)
                e32, a = ctx.encode_host_f32(f32, tol)
                e32["data"] = e32["data"].copy()
                b = ctx.decode_host_f32(out32, e32)
                e64, c = ctx.encode_host(f64, tol)
                e64["data"] = e64["data"].copy()
                d = ctx.decode_host(out64, e64)
                if r:
                    t["enc32"].append(a); t["dec32"].append(b); t["enc64"].append(c); t["dec64"].append(d)
            same_code = e32["len_enc_vec"] == e64["len_enc_vec"] and np.array_equal(e32["data"], e64["data"])
            same_rec = np.array_equal(out32.view(np.uint32), out64.astype(np.float32).view(np.uint32))
            row["encode_f32"], row["encode_f64"] = median_timings(t["enc32"]), median_timings(t["enc64"])
            row["decode_f32"], row["decode_f64"] = median_timings(t["dec32"]), median_timings(t["dec64"])
            row["nlay"] = e32["nlay"]
            row["identical"] = bool(same_code and same_rec)
            res["tol %g" % tol] = row
    return res


def timed(cmd, cwd, env):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, cwd=cwd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, env=env)
    dt = time.perf_counter() - t0
    if r.returncode:
        raise SystemExit("%s failed (%d): %s" % (cmd[0], r.returncode, r.stderr[-2000:]))
    return dt


def sha(path):
    h = hashlib.sha256()
    with open(path, "rb") as fh:
        for b in iter(lambda: fh.read(1 << 24), b""):
            h.update(b)
    return h.hexdigest()


def cli(nf, n, tol, workdir):
    from waverange_amd import synth
    d = tempfile.mkdtemp(dir=workdir)
    try:
        with open(os.path.join(d, "data.bin"), "wb") as fh:
            for k in range(nf):
                synth.field(n, n, n, seed=12345 + k).astype(np.float32).tofile(fh)
        argv = ["data.bin", "data.wrb", "data.wrh", "2", "0", str(nf), "1", str(n), str(n), str(n), "%g" % tol]
        out = {"file": "%d x %d^3 fp32, tol %g, %.2f GB" % (nf, n, tol, nf * 4 * n ** 3 / 1e9)}
        digests = {}
        for label, extra in (("f32_entry_points", {}), ("widen_on_host", {"WR_CLI_WIDEN_ON_HOST": "1"})):
            env = dict(os.environ, WR_QUIET="1", **extra)
            te = timed([os.path.join(BIN, "wrenc")] + argv, d, env)
            td = timed([os.path.join(BIN, "wrdec"), "data.wrb", "data.wrh", "datarec.bin", "2", "0"], d, env)
            out[label] = {"wrenc_s": round(te, 3), "wrdec_s": round(td, 3), "MBps_round_trip": round(nf * 4 * n ** 3 / 1e6 / (te + td), 1)}
            digests[label] = [sha(os.path.join(d, x)) for x in ("data.wrh", "data.wrb", "datarec.bin")]
        out["files_identical"] = digests["f32_entry_points"] == digests["widen_on_host"]
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,1024")
    ap.add_argument("--tols", default="1e-3,1e-7")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--nf", type=int, default=8)
    ap.add_argument("--cli-size", type=int, default=512)
    ap.add_argument("--cli-tol", type=float, default=1e-5)
    ap.add_argument("--dir", default=tempfile.gettempdir())
    a = ap.parse_args()
    from waverange_amd import api
    api.set_verbosity(0)
    res = {"host_api": {}, "units": "total in ms; h2d_ms / d2h_ms / transform_ms as the calls report them (wr_timings)"}
    for n in [int(s) for s in a.sizes.split(",") if s]:
        res["host_api"]["%d^3" % n] = host_api(api, n, [float(t) for t in a.tols.split(",")], a.reps)
    if a.nf > 0:
        res["cli"] = cli(a.nf, a.cli_size, a.cli_tol, a.dir)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
