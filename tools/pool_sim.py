#!/usr/bin/env python3
"""Closed-system model of the benchmark's host side on the coder pool (tools/native/pool_sim.cpp), no GPU needed: the real bit
planes of the synthetic field at the benchmark's tolerances come from the CPU oracle, L encoder and L decoder threads per
tolerance keep fields in flight on the pool.  Prints fields per second per direction and workers per loop kind.
usage: pool_sim.py [--size 256] [--tols 1e-3,1e-7] [--workers 16] [--lanes 6] [--seconds 10] [--csrc DIR]
--csrc: the coder sources to model (another checkout's waverange_amd/csrc), for a before / after on one box."""
import argparse
import os
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--tols", type=str, default="1e-3,1e-7")
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--lanes", type=int, default=6)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--dec-streams", type=int, default=4)
    ap.add_argument("--csrc", type=str, default=os.path.join(ROOT, "waverange_amd", "csrc"))
    args = ap.parse_args()
    from oracle.loader import Oracle
    from waverange_amd import synth
    o = Oracle()
    n = args.size
    f = synth.field(n, n, n, seed=12345)
    tols = [float(t) for t in args.tols.split(",")]
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "planes.bin")
        with open(path, "wb") as fh:
            fh.write(struct.pack("<I", len(tols)))
            for tol in tols:
                enc = o.encode(f, tol)
                fh.write(struct.pack("<IQ", enc["nlay"], f.size))
                off = 0
                for length in enc["len_enc_vec"]:
                    s = enc["data"][off:off + length]
                    off += length
                    p, got = o.range_decode(s, f.size)
                    assert got == f.size
                    fh.write(p.tobytes())
                    fh.write(struct.pack("<Q", s.size))
                    fh.write(s.tobytes())
        exe, vec_o = os.path.join(d, "pool_sim"), os.path.join(d, "vec.o")
        cxx = ["g++", "-std=c++17", "-O3", "-march=x86-64-v3"]
        subprocess.check_call(cxx + ["-mavx512f", "-mavx512bw", "-mavx512dq", "-mavx512vl", "-c", os.path.join(args.csrc, "wr_rangecoder_avx512.cpp"), "-o", vec_o])
        subprocess.check_call(cxx + ["-I" + args.csrc, os.path.join(ROOT, "tools", "native", "pool_sim.cpp"), os.path.join(args.csrc, "wr_rangecoder.cpp"), vec_o,
                                     "-o", exe, "-lpthread"])
        return subprocess.call([exe, path, str(args.workers), str(args.lanes), str(args.seconds), str(args.dec_streams)])


if __name__ == "__main__":
    sys.exit(main())
