"""The segmented plane stream ("WRS1", include/waverange_amd.h) without a GPU: the host reference of the format against
the format's definition built here from wr_range_encode on slices (which is pinned to the reference), its decoder, the
refusal of every malformed index, and the coder step shared with the kernels (csrc/wr_segcoder.h) under ASan + UBSan."""
import os
import shutil
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from util import ROOT, kat_plane
from waverange_amd import api

CSRC = os.path.join(ROOT, "waverange_amd", "csrc")
SEGS = [16, 4096, 59904, 59984]


def sizes(seg):
    return [0, 1, 15, seg - 1, seg, seg + 1, 3 * seg, 3 * seg + 7]


def planes(n, seg):
    """(name, plane) for a length: the kat_plane kinds where they exist (n >= 2) and seeded random planes."""
    out = []
    if n >= 2:
        out += [(k, kat_plane(k, n)) for k in ("uniform", "skewed", "sparse")]
    rng = np.random.default_rng(1000 * seg + n)
    out.append(("random", rng.integers(0, 256, n, dtype=np.uint8)))
    out.append(("random_narrow", (rng.integers(0, 256, n, dtype=np.uint8) & 7).astype(np.uint8)))
    return out


def blob_by_definition(plane, seg):
    """The normative layout, from wr_range_encode on the slices."""
    n = plane.size
    nseg = (n + seg - 1) // seg
    streams = [api.range_encode(plane[k * seg:min(n, (k + 1) * seg)]).tobytes() for k in range(nseg)]
    return b"WRS1" + struct.pack("<II", seg, nseg) + b"".join(struct.pack("<I", len(s)) for s in streams) + b"".join(streams)


@pytest.mark.parametrize("seg", SEGS)
def test_host_ref_is_the_format(seg):
    for n in sizes(seg):
        for name, p in planes(n, seg):
            blob = api.seg_encode_host_ref(p, seg)
            assert blob.tobytes() == blob_by_definition(p, seg), (seg, n, name)
            assert blob.size <= api.seg_bound(n, seg)
            back = api.seg_decode_host_ref(blob, n)
            assert np.array_equal(back, p), (seg, n, name)
            got_seg, streams = api.seg_split(blob)
            assert got_seg == seg and len(streams) == (n + seg - 1) // seg


def test_default_segment_length():
    p = kat_plane("skewed", 2 * 59904 + 5)
    assert api.SEG_DEFAULT == 59904
    assert api.seg_encode_host_ref(p, 0).tobytes() == blob_by_definition(p, 59904)


@pytest.mark.parametrize("seg", [8, 60000, 24, 59999, 1 << 20])
def test_bad_segment_length_is_refused(seg):
    assert api.seg_bound(1000, seg) == 0
    with pytest.raises(api.WaveRangeError):
        api.seg_encode_host_ref(kat_plane("uniform", 1000), seg)


def test_bound_is_the_range_coder_bound_per_segment():
    for seg in SEGS:
        for n in (0, 1, seg, 3 * seg + 7):
            nseg = (n + seg - 1) // seg
            assert api.seg_bound(n, seg) == 12 + nseg * (4 + api.lib().wr_range_encode_bound(seg))


def _refused(blob, n):
    with pytest.raises(api.WaveRangeError) as e:
        api.seg_decode_host_ref(np.frombuffer(bytes(blob), dtype=np.uint8), n)
    assert "error %d" % -4 in str(e.value) or "stream" in str(e.value).lower() or "segment" in str(e.value).lower(), str(e.value)
    return str(e.value)


def test_malformed_index_is_refused():
    seg, n = 4096, 3 * 4096 + 7
    p = kat_plane("skewed", n)
    good = bytearray(api.seg_encode_host_ref(p, seg).tobytes())
    nseg = 4
    lens = list(struct.unpack("<4I", good[12:28]))
    # wrong magic (a reference stream starts with byte 0)
    bad = bytearray(good); bad[0] = 0
    assert "magic" in _refused(bad, n)
    # seg out of range / not a multiple of 16
    for s in (8, 60000, 4097):
        bad = bytearray(good); bad[4:8] = struct.pack("<I", s)
        assert "segment length" in _refused(bad, n)
    # nseg != ceil(n / seg)
    bad = bytearray(good); bad[8:12] = struct.pack("<I", nseg + 1)
    assert "segment count" in _refused(bad, n)
    assert "segment count" in _refused(good, n + seg)
    # index longer than the blob
    assert "index longer" in _refused(good[:12 + 4 * nseg - 1], n)
    assert "header" in _refused(good[:11], n)
    # lengths that do not sum to the rest of the blob
    bad = bytearray(good); bad[12:16] = struct.pack("<I", lens[0] + 1)
    assert "add up" in _refused(bad, n)
    assert "add up" in _refused(good[:-1], n)
    assert "add up" in _refused(good + b"\0", n)
    # a length above wr_range_encode_bound(seg)
    over = api.lib().wr_range_encode_bound(seg) + 1
    bad = bytearray(good[:28]); bad[12:16] = struct.pack("<I", over)
    bad += bytes(over + sum(lens[1:]))
    assert "longer than a segment can be" in _refused(bad, n)
    # and the untouched blob still decodes
    assert np.array_equal(api.seg_decode_host_ref(np.frombuffer(bytes(good), dtype=np.uint8), n), p)


def test_corrupt_payload_is_refused_or_decodes_without_harm():
    """Flipped payload bytes behind a valid index: an error or n symbols, never anything else."""
    seg, n = 4096, 2 * 4096 + 100
    p = kat_plane("skewed", n)
    good = api.seg_encode_host_ref(p, seg)
    rng = np.random.default_rng(5)
    for _ in range(200):
        bad = good.copy()
        at = rng.integers(12 + 4 * 3, bad.size, 3)
        bad[at] ^= rng.integers(1, 256, 3).astype(np.uint8)
        try:
            back = api.seg_decode_host_ref(bad, n)
            assert back.size == n
        except api.WaveRangeError:
            pass


SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]  # tests/test_sanitizers.py


def _have_san():
    if shutil.which("g++") is None:
        return False
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        open(src, "w").write("int main(){return 0;}\n")
        return subprocess.run(["g++"] + SAN + [src, "-o", os.path.join(d, "t")], capture_output=True).returncode == 0


@pytest.mark.skipif(not _have_san(), reason="g++ with ASan/UBSan not available")
def test_segment_coder_under_sanitizers():
    """csrc/wr_segcoder.h -- the step code the kernels run -- compiled by g++: round trips against the host range coder,
    truncated, bit-flipped and random segment streams (tests/native/seg_fuzz.cpp)."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "seg_fuzz")
        vec_o = os.path.join(d, "vec.o")
        subprocess.check_call(["g++"] + SAN + ["-mavx512f", "-mavx512bw", "-mavx512dq", "-mavx512vl", "-c",
                                               os.path.join(CSRC, "wr_rangecoder_avx512.cpp"), "-o", vec_o])
        subprocess.check_call(["g++"] + SAN + ["-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "seg_fuzz.cpp"),
                                               os.path.join(CSRC, "wr_rangecoder.cpp"), os.path.join(CSRC, "wr_compat.cpp"), vec_o, "-o", exe, "-lpthread"])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "segment coder sanitizer run OK" in r.stdout
        assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
