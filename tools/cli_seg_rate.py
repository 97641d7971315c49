#!/usr/bin/env python3
"""Wall clock of wrenc / wrdec per stream format: the reference's plane streams (`ref`) next to the segmented formats
(`wrs1`, `wrs2`, `wrs3`) on the inputs of tools/cli_rate.py -- NF n^3 fp64 fields in one raw file, seeds 12345 .. -- on ONE GPU.

    python tools/cli_seg_rate.py [--inputs 8x512,1x1024] [--tol 1e-5] [--reps 5] [--dir /tmp/wr_cli_seg] [--tag NAME]

Per input: a warm-up round in which every format's decoded file is compared byte for byte with the `ref` format's, then
--reps repetitions, each running all formats one after the other (so that drift of the machine hits all rows alike): wrenc,
wrdec, and for the segmented files wrdec --roi of a centred 32^3 cube of field 0 and wrdec --level=2 of every field.  Medians
over the repetitions.  The yardstick of a segmented row is the `ref` row of the SAME run.  There is no gate.

Every step runs under its own `timeout`; the first step that fails ends the script with its status.  The tools' own phase
lines (WR_CLI_TIMING=1: seconds reading, inside codec calls summed over the fields in flight, writing) are recorded with the
wall clock: where `read` + `write` make up the wall time, the tool is bound by its single reading thread and the file system,
not by the codec.  An input the directory's file system or the host's memory cannot hold is skipped and said so.
The record goes to profiles/cli_seg/<tag>.json and to stdout."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BIN = os.path.join(ROOT, "waverange_amd", "bin")
FORMATS = ["ref", "wrs1", "wrs2", "wrs3"]


def step(cmd, cwd, env, limit):
    """One tool run under `timeout`; returns (wall seconds, phase seconds from the tool's timing line)."""
    t0 = time.perf_counter()
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=cwd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, env=env)
    dt = time.perf_counter() - t0
    if r.returncode:
        print("FAILED (%d) after %.1f s: %s\n%s" % (r.returncode, dt, " ".join(cmd), r.stderr[-2000:]), flush=True)
        raise SystemExit(r.returncode)
    phases = {}
    for line in r.stderr.splitlines():
        if line.startswith("timing tool="):
            phases = {k: float(v) for k, v in (kv.split("=") for kv in line.split()[2:])}
    return dt, phases


def mem_available():
    with open("/proc/meminfo") as fh:
        for line in fh:
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) * 1024
    return 0


def make_input(path, nf, n):
    from waverange_amd import api
    api.set_verbosity(0)
    with api.Context(0) as ctx, open(path, "wb") as fh:
        buf = ctx.alloc(n ** 3 * 8)
        host = api.pinned_array((n, n, n))
        for k in range(nf):  # the fields of bench.py's ranks: seed 12345 + k
            ctx.synth_field(buf, n, n, n, 12345 + k)
            ctx.sync()
            api._check(api.lib().wr_dev_download(ctx.h, host.ctypes.data, buf.ptr, host.nbytes))
            host.tofile(fh)
        buf.free()
        del host


def median_of(rows, key):
    vals = [r[key] for r in rows if key in r]
    return round(statistics.median(vals), 4) if vals else None


def measure(nf, n, args, d):
    size = nf * n ** 3 * 8
    free, mem = shutil.disk_usage(d).free, mem_available()
    # on disk at once: the input, two decoded files (one being compared with ref's) and four coded files
    if free < 3.6 * size or mem < 2.5 * size:
        return {"input": "%dx%d^3" % (nf, n), "skipped": "needs %.0f GB of disk and %.0f GB of memory; %.0f / %.0f GB available" %
                (3.6 * size / 1e9, 2.5 * size / 1e9, free / 1e9, mem / 1e9)}
    t0 = time.perf_counter()
    make_input(os.path.join(d, "data.bin"), nf, n)
    out = {"input": "%dx%d^3" % (nf, n), "workload": "NF = %d independent %d^3 fp64 fields in one raw file (TYPE 2), tol %s, one GPU" % (nf, n, args.tol),
           "field_MB": size / 1e6, "make_input_s": round(time.perf_counter() - t0, 2), "reps": args.reps, "rows": {}}
    env = dict(os.environ, WR_QUIET="1", WR_CLI_TIMING="1")
    env.pop("WR_STREAM_FORMAT", None)
    lo = n // 2 - 16
    roi = "--roi=%d:%d,%d:%d,%d:%d" % ((lo, lo + 32) * 3)

    def one(fmt, compare):
        row = {}
        enc = [os.path.join(BIN, "wrenc"), "--format=" + fmt, "data.bin", fmt + ".wrb", fmt + ".wrh", "2", "0", str(nf), "2", str(n), str(n), str(n), args.tol]
        row["wrenc_s"], ph = step(enc, d, env, args.limit)
        row.update({"wrenc_" + k: v for k, v in ph.items()})
        rec = "ref_rec.bin" if fmt == "ref" else "rec.bin"
        row["wrdec_s"], ph = step([os.path.join(BIN, "wrdec"), fmt + ".wrb", fmt + ".wrh", rec, "2", "0"], d, env, args.limit)
        row.update({"wrdec_" + k: v for k, v in ph.items()})
        if fmt != "ref":
            if compare:
                row["decoded_file_identical_to_ref"] = subprocess.run(["cmp", "-s", "rec.bin", "ref_rec.bin"], cwd=d).returncode == 0
                if not row["decoded_file_identical_to_ref"]:
                    print("FAILED: the decoded file of %s differs from ref's" % fmt, flush=True)
                    raise SystemExit(1)
            os.remove(os.path.join(d, "rec.bin"))
            row["wrdec_roi32_s"], _ = step([os.path.join(BIN, "wrdec"), roi, "--field=0", fmt + ".wrb", fmt + ".wrh", "part.bin", "2", "0"], d, env, args.limit)
            assert os.path.getsize(os.path.join(d, "part.bin")) == 32 ** 3 * 8
            row["wrdec_level2_s"], _ = step([os.path.join(BIN, "wrdec"), "--level=2", fmt + ".wrb", fmt + ".wrh", "part.bin", "2", "0"], d, env, args.limit)
        row["wrb_bytes"] = os.path.getsize(os.path.join(d, fmt + ".wrb"))
        return row

    out["warm_up"] = {fmt: one(fmt, True) for fmt in FORMATS}
    reps = [{fmt: one(fmt, False) for fmt in FORMATS} for _ in range(args.reps)]
    for fmt in FORMATS:
        rows = [r[fmt] for r in reps]
        keys = sorted({k for r in rows for k in r})
        med = {k: median_of(rows, k) for k in keys if k != "wrb_bytes"}
        med["wrb_bytes"] = rows[0]["wrb_bytes"]
        med["roundtrip_s"] = round(med["wrenc_s"] + med["wrdec_s"], 4)
        med["roundtrip_MBps"] = round(size / 1e6 / med["roundtrip_s"], 1)
        out["rows"][fmt] = med
    ref = out["rows"]["ref"]
    for fmt in FORMATS[1:]:
        r = out["rows"][fmt]
        r["roundtrip_vs_ref"] = round(ref["roundtrip_s"] / r["roundtrip_s"], 2)
        r["bytes_vs_ref"] = round(r["wrb_bytes"] / ref["wrb_bytes"], 4)
    for f in os.listdir(d):
        os.remove(os.path.join(d, f))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="8x512,1x1024", help="NFxN[,NFxN...]: NF fields of N^3")
    ap.add_argument("--tol", default="1e-5")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds a single tool run may take")
    ap.add_argument("--dir", default=os.path.join(os.environ.get("TMPDIR", "/tmp"), "wr_cli_seg"))
    ap.add_argument("--tag", default="cli_seg_rate")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "cli_seg"))
    args = ap.parse_args()
    os.makedirs(args.dir, exist_ok=True)
    record = {"tool": "tools/cli_seg_rate.py", "cpus": len(os.sched_getaffinity(0)), "dir": args.dir, "formats": FORMATS, "inputs": []}
    for item in args.inputs.split(","):
        nf, n = (int(v) for v in item.split("x"))
        record["inputs"].append(measure(nf, n, args, args.dir))
        os.makedirs(args.out_dir, exist_ok=True)
        with open(os.path.join(args.out_dir, args.tag + ".json"), "w") as fh:  # (after every input: a later failure keeps the earlier rows)
            json.dump(record, fh, indent=1)
            fh.write("\n")
    print(json.dumps(record), flush=True)


if __name__ == "__main__":
    main()
