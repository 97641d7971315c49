"""Constant blocks in the product path: concurrent host-to-host round trips of a field whose first plane is mostly constant
blocks, on a coder pool of two workers -- so that the pool's sessions hold more streams than a scalar loop takes and run the
16-lane loops, which pass such blocks over in the header phase of a step.  Bytes, header scalars, reconstructions and the
pool's block accounting must be what they are without the pass."""
import threading

import numpy as np
import pytest

from util import bits_equal
from waverange_amd import synth

pytestmark = pytest.mark.gpu

BLOCK = 60000
SHAPE = (128, 128, 128)
TOLS = (1e-3, 1e-7)
THREADS = 8


def _blocks(api):
    s = api.pool_loop_stats()
    return (s["scalar_encoder"][1] + s["vector_encoder"][1], s["scalar_decoder"][1] + s["vector_decoder"][1])


def test_concurrent_round_trips_on_a_small_pool(oracle):
    from waverange_amd import api
    api.set_verbosity(0)
    f = synth.field(*SHAPE, seed=2024)
    want = {tol: oracle.encode(f, tol) for tol in TOLS}
    api.set_coder_pool(2, 4)
    try:
        # a lone call per tolerance: what every concurrent one must reproduce
        lone = {}
        with api.Context(0) as c:
            for tol in TOLS:
                enc, _ = c.encode_host(f, tol)
                enc["data"] = enc["data"].copy()
                out = np.empty_like(f)
                c.decode_begin(f.shape, enc)
                c.decode_finish_host(out)
                lone[tol] = out
        api.set_coder_pool(0)  # (joins the workers: every step is booked)
        enc0, dec0 = _blocks(api)
        api.set_coder_pool(2, 4)
        errors = []

        def worker(k):
            try:
                with api.Context(0) as c:
                    for tol in (TOLS if k % 2 == 0 else TOLS[::-1]):
                        enc, _ = c.encode_host(f, tol)
                        w = want[tol]
                        for key in ("tolabs", "midval", "halfspanval", "wlev", "nlay", "ntot_enc", "len_enc_vec"):
                            assert enc[key] == w[key], (k, tol, key)
                        assert bits_equal(enc["deps_vec"], w["deps_vec"]) and bits_equal(enc["minval_vec"], w["minval_vec"]), (k, tol)
                        assert np.array_equal(enc["data"], w["data"]), (k, tol, "coded bytes differ from the oracle's")
                        enc["data"] = enc["data"].copy()
                        out = np.empty_like(f)
                        c.decode_begin(f.shape, enc)
                        c.decode_finish_host(out)
                        assert bits_equal(out, lone[tol]), (k, tol, "reconstruction differs from a lone call's")
            except Exception as exc:  # noqa: BLE001
                errors.append((k, exc))

        ths = [threading.Thread(target=worker, args=(k,)) for k in range(THREADS)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
    finally:
        api.set_coder_pool(0)
    assert not errors, errors
    # stream-blocks advanced: a stream is in an encoder session for one step per block (the final, partial one included) and
    # in a decoder session for one more, in which it reads "no more blocks" -- whether blocks were passed over or not
    enc1, dec1 = _blocks(api)
    planes = THREADS * sum(want[tol]["nlay"] for tol in TOLS)
    steps = f.size // BLOCK + 1
    assert enc1 - enc0 == planes * steps, (enc1 - enc0, planes, steps)
    assert dec1 - dec0 == planes * (steps + 1), (dec1 - dec0, planes, steps + 1)
