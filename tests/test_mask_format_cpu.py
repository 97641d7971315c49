"""The mask blob of a masked record ("WRM1") on the host, no GPU: the 32-byte header followed by the WRS1 blob of the packed
bits, the parse that inverts it, every refusal a decoder owes a damaged blob -- each raised on a blob that is wrong in exactly
that way --, and the bound.  Sizes: a single sample, around one byte, around one wave's 64 samples, an odd size, and
59904 * 8 + 5, whose packed bits need a second segment at the default segment length."""
import struct

import numpy as np
import pytest

from waverange_amd import api

SIZES = [1, 7, 8, 9, 63, 64, 65, 1005, 59904 * 8 + 5]
SEGS = [0, 16]
ERR_STREAM = "error -4"


def flags_of(n):
    """a coherent region, a few isolated samples, and the last sample (its bit is the highest one in use)"""
    rng = np.random.default_rng(77 + n)
    f = np.zeros(n, dtype=bool)
    f[n // 4: n // 4 + max(n // 3, 1)] = True
    f[rng.integers(0, n, size=min(n, 5))] = True
    f[n - 1] = True
    return f


def header(n, undefined, pad, magic=b"WRM1", reserved=0):
    return np.frombuffer(magic + struct.pack("<IQQd", reserved, n, undefined, pad), dtype=np.uint8)


def packed(flags):
    return np.packbits(flags, bitorder="little")


@pytest.fixture(scope="module", params=SIZES)
def case(request):
    n = request.param
    f = flags_of(n)
    return n, f, {seg: api.mask_blob_host_ref(f, seg, pad=-1.25) for seg in SEGS}


@pytest.mark.parametrize("seg", SEGS)
def test_blob_is_the_header_and_the_wrs1_blob_of_the_packed_bits(case, seg):
    n, f, blobs = case
    want = np.concatenate([header(n, int(f.sum()), -1.25), api.seg_encode_host_ref(packed(f), seg)])
    assert np.array_equal(blobs[seg], want)
    assert len(header(n, 0, 0.0)) == api.MASK_HEADER_BYTES == 32
    assert api.mask_sniff(blobs[seg]) and not api.mask_sniff(blobs[seg][:31]) and not api.mask_sniff(want[32:])
    assert api.mask_bound(n, seg) >= blobs[seg].size
    if n % 8:  # the unused high bits of the last symbol
        assert packed(f)[-1] >> (n % 8) == 0


@pytest.mark.parametrize("seg", SEGS)
def test_parse_inverts_the_blob(case, seg):
    n, f, blobs = case
    got, undefined, pad = api.mask_parse_host_ref(blobs[seg], n)
    assert np.array_equal(got, f) and undefined == int(f.sum()) and pad == -1.25


def test_second_segment_at_the_default_length():
    n = 59904 * 8 + 5
    blob = api.mask_blob_host_ref(flags_of(n), 0)
    assert bytes(blob[32:36]) == b"WRS1" and struct.unpack("<II", bytes(blob[36:44])) == (59904, 2)


def refused(blob, n, what):
    with pytest.raises(api.WaveRangeError) as e:
        api.mask_parse_host_ref(blob, n)
    assert ERR_STREAM in str(e.value) and what in str(e.value), str(e.value)


@pytest.mark.parametrize("seg", SEGS)
def test_every_refusal_on_a_blob_wrong_in_exactly_that_way(case, seg):
    n, f, blobs = case
    blob = blobs[seg]
    count = int(f.sum())
    plane = blob[32:]
    refused(np.concatenate([header(n, count, -1.25, magic=b"WRM2"), plane]), n, "wrong magic")
    refused(np.concatenate([header(n, count, -1.25, reserved=1), plane]), n, "reserved")
    refused(np.concatenate([header(n + 1, count, -1.25), plane]), n, "sample count")
    refused(blob[:-1], n, "mask blob")                                             # truncated
    refused(blob[:20], n, "truncated header")
    refused(np.concatenate([blob, np.zeros(1, np.uint8)]), n, "mask blob")         # overlong
    # a WRS1 blob that does not decode: the index stays whole; a byte in the first segment's model (the 256 counts in front of
    # its symbols) does not, and the counts no longer add up to the segment
    nseg = struct.unpack("<I", bytes(blob[40:44]))[0]
    bad = blob.copy()
    bad[32 + 12 + 4 * nseg + 2] ^= 0x40
    refused(bad, n, "does not decode")
    # the bits altered and coded again, so that the blob is well formed and only the property under test is wrong
    bits = packed(f).copy()
    wrong = bits.copy()
    first_clear = int(np.flatnonzero(~f)[0]) if (~f).any() else None
    if first_clear is not None:  # one more sample marked than the header says
        wrong[first_clear >> 3] |= 1 << (first_clear & 7)
        refused(np.concatenate([header(n, count, -1.25), api.seg_encode_host_ref(wrong, seg)]), n, "count in its header")
    refused(np.concatenate([header(n, count - 1, -1.25), plane]), n, "count in its header")
    if n % 8:  # the last sample's bit moved beyond n: the population count still agrees with the header
        beyond = bits.copy()
        beyond[-1] = (int(beyond[-1]) & (0xFF ^ (1 << ((n - 1) & 7)))) | 0x80
        refused(np.concatenate([header(n, count, -1.25), api.seg_encode_host_ref(beyond, seg)]), n, "beyond")
    # more undefined samples than samples
    refused(np.concatenate([header(n, n + 1, -1.25), plane]), n, "more undefined")


def test_arguments():
    with pytest.raises(api.WaveRangeError):
        api.mask_blob_host_ref(np.ones(9, bool), seg=17)
    assert api.mask_bound(9, 17) == 0
    assert api.mask_bound(9, 16) == 32 + api.seg_bound(2, 16)
