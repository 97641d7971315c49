"""The range coder of the segmented formats restated in plain Python: the definition that the host reference (and through it
the kernels) is compared with.  The steps are rngcod13's in their classical form -- the carry is propagated back into the bytes
already written -- while the library keeps a held byte and a count of pending 0xff bytes (csrc/wr_segcoder.h, Enc).  Beside
its bytes the encoder counts which arm of Enc::renorm and Enc::finish the library takes at every step and how long the runs
of pending bytes are that it flushes, so that a test can say which branches of the library its cases reach (COUNTS)."""
import struct

import numpy as np

TOP, BOTTOM, SHIFT = 1 << 31, 1 << 23, 23

# Enc::renorm: "out" (low < 0xff << 23: the held byte goes out, pending bytes as 0xff), "carry" (low & kTop: held + 1, pending
# bytes as 0x00), "pend" (the byte is 0xff and nothing is known yet).  Enc::finish: "finish_carry" (t > 0xff) or "finish_plain".
# max_ff / max_00: the longest run of pending bytes flushed as 0xff / as 0x00, in renorm or in finish.
ARMS = ("out", "carry", "pend", "finish_carry", "finish_plain")
COUNTS = dict.fromkeys(ARMS + ("max_ff", "max_00"), 0)


def reset_counts():
    for k in COUNTS:
        COUNTS[k] = 0


class PyEnc:
    """rngcod13's encoder with the carry propagated back into the bytes already written (the library keeps a held byte and a
    count of pending 0xff bytes instead).  out[0] is the byte given to start_encoding."""

    def __init__(self):
        self.low, self.range, self.n, self.out = 0, TOP, 0, bytearray([0])
        self.pending = 0  # what the library's `pending` is at this point: bookkeeping for COUNTS, not used for the bytes

    def _carry(self):
        i = len(self.out) - 1
        while self.out[i] == 0xFF:
            self.out[i] = 0
            i -= 1
        self.out[i] += 1

    def _flushed(self, polarity):
        if self.pending > COUNTS[polarity]:
            COUNTS[polarity] = self.pending
        self.pending = 0

    def _renorm(self):
        while self.range <= BOTTOM:
            if self.low & TOP:
                self._carry()
                COUNTS["carry"] += 1
                self._flushed("max_00")
            elif self.low < (0xFF << SHIFT):
                COUNTS["out"] += 1
                self._flushed("max_ff")
            else:
                COUNTS["pend"] += 1
                self.pending += 1
            self.out.append((self.low >> SHIFT) & 0xFF)
            self.low = (self.low << 8) & (TOP - 1)
            self.range <<= 8
            self.n += 1

    def freq(self, sy, lt, tot):
        self._renorm()
        r = self.range // tot
        t = r * lt
        self.low += t
        self.range = r * sy if lt + sy < tot else self.range - t

    def short(self, v):
        self._renorm()
        r = self.range >> 16
        t = r * v
        self.low += t
        self.range = self.range - t if (v + 1) >> 16 else r

    def done(self):
        self._renorm()
        self.n += 5
        t = self.low >> SHIFT
        if (self.low & (BOTTOM - 1)) >= ((self.n & 0xFFFFFF) >> 1):
            t += 1
        if t > 0xFF:
            self._carry()
            COUNTS["finish_carry"] += 1
            self._flushed("max_00")
        else:
            COUNTS["finish_plain"] += 1
            self._flushed("max_ff")
        self.out.append(t & 0xFF)
        self.out += bytes([(self.n >> 16) & 0xFF, (self.n >> 8) & 0xFF, self.n & 0xFF])
        return bytes(self.out)


def model_of(sym):
    count = np.bincount(sym, minlength=256).tolist()
    cum = [0] * 256
    for s in range(1, 256):
        cum[s] = cum[s - 1] + count[s - 1]
    return count, cum


def py_wrs1_segment(sym):
    """One WRS1 segment: the reference's block structure around the restated steps."""
    count, cum = model_of(sym)
    e = PyEnc()
    e.freq(1, 1, 2)
    for s in range(256):
        e.short(count[s])
    bs = len(sym)
    for s in sym.tolist():
        e.freq(count[s], cum[s], bs)
    e.freq(1, 0, 2)
    return e.done()


def py_wrs1_blob(plane, seg):
    """'WRS1' | u32 seg | u32 nseg | u32 len[nseg] | the segment streams"""
    n = plane.size
    nseg = (n + seg - 1) // seg
    streams = [py_wrs1_segment(plane[k * seg:min(n, (k + 1) * seg)]) for k in range(nseg)]
    return b"WRS1" + struct.pack("<II", seg, nseg) + b"".join(struct.pack("<I", len(s)) for s in streams) + b"".join(streams)


def strand_len(seg, K):
    return 16 * ((seg + 16 * K - 1) // (16 * K))


def py_record(sym, seg, K):
    """record := u32 tlen | u32 slen[K] | T | S_0 .. | zero bytes up to a multiple of 4"""
    count, cum = model_of(sym)
    bs, L = len(sym), strand_len(seg, K)
    e = PyEnc()
    for s in range(256):
        e.short(count[s])
    T = e.done()
    strands = []
    for j in range(K):
        part = sym[j * L:min((j + 1) * L, bs)].tolist()
        if not part:
            strands.append(b"")
            continue
        e = PyEnc()
        for s in part:
            e.freq(count[s], cum[s], bs)
        e.freq(1, 0, 2)
        strands.append(e.done())
    body = struct.pack("<%dI" % (K + 1), len(T), *[len(s) for s in strands]) + T + b"".join(strands)
    return body + bytes(-len(body) % 4)


def py_blob(plane, seg, K, brick=0):
    n = plane.size
    nseg = (n + seg - 1) // seg
    recs = [py_record(plane[k * seg:min(n, (k + 1) * seg)], seg, K) for k in range(nseg)]
    return b"WRS3" + struct.pack("<IIII", seg, nseg, brick, K) + b"".join(struct.pack("<I", len(r)) for r in recs) + b"".join(recs)


class PyDec:
    """rngcod13's decoder; past the end of its bytes it reads zeros."""

    def __init__(self, data):
        self.d, self.pos = data, 1  # (the byte given to start_encoding)
        self.buffer = self._get()
        self.low, self.range, self.help = self.buffer >> 1, 1 << 7, 0

    def _get(self):
        b = self.d[self.pos] if self.pos < len(self.d) else 0
        self.pos += 1
        return b

    def _renorm(self):
        while self.range <= BOTTOM:
            self.low = (self.low << 8) | ((self.buffer << 7) & 0xFF)
            self.buffer = self._get()
            self.low |= self.buffer >> 1
            self.range <<= 8

    def culfreq(self, tot):
        self._renorm()
        self.help = self.range // tot
        return min(self.low // self.help, tot - 1)

    def culshort(self):
        self._renorm()
        self.help = self.range >> 16
        return min(self.low // self.help, 0xFFFF)

    def update(self, sy, lt, tot):
        t = self.help * lt
        self.low -= t
        self.range = self.help * sy if lt + sy < tot else self.range - t


def py_decode_model(T):
    d, count = PyDec(T), []
    for _ in range(256):
        c = d.culshort()
        d.update(1, c, 1 << 16)
        count.append(c)
    return count


def py_decode_strand(S, count, m):
    cum = np.concatenate(([0], np.cumsum(count)[:-1]))
    bs, d, out = int(sum(count)), PyDec(S), []
    for _ in range(m):
        cf = d.culfreq(bs)
        s = int(np.searchsorted(cum, cf, side="right")) - 1  # the last s whose cumulative count is <= cf
        d.update(count[s], int(cum[s]), bs)
        out.append(s)
    assert d.culfreq(2) == 0  # the zero flag
    return np.array(out, dtype=np.uint8)
