"""The sizing function of the masked batch calls, without a GPU: wr_seg_batch_device_bytes_masked is the plain batch's size plus
the masks' share.  At nmasked = 0 only the once-terms it documents remain (an encode: the split partials of nfields fields, two
8-byte words per block of the split's grid; a decode: nothing); every masked field adds at least its bit plane and its blob;
the result never decreases in any argument and is 0 for each refused one.
(No host-only function came with the batch calls -- the tables are filled where they are launched -- so there is no native
fuzzer for them; the blob checks of a batch are wrmask::check_blobs', which tests/native/maskroibatch_fuzz.cpp runs.)"""
import itertools

from waverange_amd import api

masked = api.seg_batch_device_bytes_masked


def up256(v):
    return (v + 255) & ~255


def split_partials(nfields, n):
    grid = min(max(-(-(-(-n // 64)) // 4), 1), 2048)  # a block per 4 chunks of 64 samples, at most 2048
    return up256(nfields * 2 * grid * 8)


def test_no_masked_field_leaves_the_once_terms():
    for nf, n, nlay, seg, brick, strands in [(1, 5049, 3, 16, 0, 0), (4, 64 ** 3, 3, 0, 0, 0), (8, 64 ** 3, 2, 1024, 32, 0), (5, 64 ** 3, 4, 1024, 0, 4),
                                              (3, 128 ** 3, 1, 0, 8, 8), (1024, 4099, 0, 0, 0, 0)]:
        if strands:
            base = api.seg_batch_device_bytes_strands(nf, n, nlay, seg, brick, strands)
        else:  # an encode without strands makes WRS1 / WRS2 planes: the plain batch call's size
            base = api.seg_batch_device_bytes(nf, n, nlay, seg, brick)
        assert base > 0 or nlay == 0  # (fields that are constant: no plane, nothing to size)
        assert masked(nf, 0, n, nlay, seg, brick, strands) == base + split_partials(nf, n)
        # the decode is the mixed driver's, whatever the formats: with strands, seg_batch_device_bytes_strands and nothing more;
        # without, the same sum with the blobs at the WRS1 / WRS2 bound: at least the plain batch decode's planes, blobs and work
        if strands:
            assert masked(nf, 0, n, nlay, seg, brick, strands, True) == api.seg_batch_device_bytes_strands(nf, n, nlay, seg, brick, strands, True) > 0
        elif nlay:
            assert masked(nf, 0, n, nlay, seg, brick, 0, True) >= nf * nlay * (n + api.seg_bound(n, seg))


def test_every_masked_field_adds_its_plane_and_its_blob():
    n = 64 ** 3
    nsym = -(-n // 8)
    for decode in (False, True):
        for seg in (0, 48, 4096):
            prev = masked(6, 0, n, 3, seg, 0, 0, decode)
            for nm in range(1, 7):
                size = masked(6, nm, n, 3, seg, 0, 0, decode)
                blob = api.mask_bound(n, seg) if decode else api.seg_bound(nsym, seg)
                assert size >= prev + nsym + blob
                prev = size


def test_monotone_in_every_argument():
    nfs, nms, ns, nlays = (1, 2, 7, 64), (0, 1, 2, 7), (1, 63, 5049, 64 ** 3, 128 ** 3), (0, 1, 3, 8)
    for decode, (seg, brick, strands) in itertools.product((False, True), [(0, 0, 0), (1024, 0, 0), (1024, 32, 0), (1024, 0, 1), (1024, 0, 4), (1024, 8, 4)]):
        size = {}
        for nf, nm, n, nlay in itertools.product(nfs, nms, ns, nlays):
            if nm <= nf:
                size[nf, nm, n, nlay] = masked(nf, nm, n, nlay, seg, brick, strands, decode)
                # (a decode of unmasked constant records takes nothing from the device: 0 bytes, the one size that is not positive)
                assert size[nf, nm, n, nlay] > 0 or (decode and nm == 0 and nlay == 0)
        for (nf, nm, n, nlay), s in size.items():
            for axis, grid in enumerate((nfs, nms, ns, nlays)):
                key = [nf, nm, n, nlay]
                at = grid.index(key[axis])
                if at + 1 < len(grid):
                    key[axis] = grid[at + 1]
                    if tuple(key) in size:
                        assert size[tuple(key)] >= s, (decode, seg, brick, strands, (nf, nm, n, nlay), axis)
    # a brick edge adds a plane in stream order.  (seg, strands and decode choose a layout, they are no measure of the work:
    # a WRS3 encode at one strand stages less than a WRS1 encode.)
    n = 64 ** 3
    for decode in (False, True):
        assert masked(4, 4, n, 3, 1024, 32, 0, decode) >= masked(4, 4, n, 3, 1024, 0, 0, decode)


def test_refused_arguments_give_zero():
    n = 64 ** 3
    assert masked(4, 2, n, 3) > 0
    assert masked(0, 0, n, 3) == 0 and masked(api.SEG_BATCH_MAX + 1, 0, n, 3) == 0 and masked(-1, 0, n, 3) == 0
    assert masked(4, 5, n, 3) == 0 and masked(4, -1, n, 3) == 0
    assert masked(4, 2, 0, 3) == 0
    assert masked(4, 2, n, -1) == 0 and masked(4, 2, n, 99) == 0
    assert masked(4, 2, n, 3, seg=17) == 0 and masked(4, 2, n, 3, brick=3) == 0
    assert masked(4, 2, n, 3, strands=3) == 0 and masked(4, 2, n, 3, seg=16, strands=2) == 0
    for decode in (False, True):
        assert masked(4, 5, n, 3, decode=decode) == 0 and masked(4, 2, n, 3, seg=17, decode=decode) == 0
    assert masked(api.SEG_BATCH_MAX, api.SEG_BATCH_MAX, 4099, 1) > 0
