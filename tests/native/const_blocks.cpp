// Constant blocks -- full blocks of one symbol, which the host coder passes over in the header phase of a step -- through every
// entry point of wr_rangecoder.h.  Stand-alone (built plain and under ASan + UBSan by tests/test_const_blocks_cpu.py).  Every
// expected byte and every expected decoder result comes from the per-symbol block coder below, written on the exported
// rngcod13 primitives (wr_compat.cpp) with the block model of wrappers.cpp:85-128 / 153-224 -- never from the code under test.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "wr_rangecoder.h"
#include "waverange_amd.h"

typedef std::vector<uint8_t> Bytes;
static const size_t kB = wrrc::kBlock;
static unsigned long long rs = 0x9E3779B97F4A7C15ull;
static unsigned rnd() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return (unsigned)(rs >> 11); }
static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); if (++fails > 20) exit(1); } } while (0)

// ---- the reference: one coder step per symbol
// blocks: sizes of the blocks in order (the reference's encoder writes 60000, ..., 60000, rest -- rest may be 0); hdr_end[b]:
// stream position (a lower bound: bytes the coder had put out) behind block b's header
static Bytes ref_encode(const Bytes& p, const std::vector<unsigned>& blocks, std::vector<size_t>* hdr_end = nullptr)
{
    rangecoder rc;
    init_databuf(&rc, 2 * p.size() + 600 * (blocks.size() + 2) + 1024);
    start_encoding(&rc, 0, 0);
    size_t at = 0;
    for (unsigned bs : blocks) {
        encode_freq(&rc, 1, 1, 2);
        unsigned cnt[256] = {0}, cum[257];
        for (unsigned i = 0; i < bs; i++) cnt[p[at + i]]++;
        cum[0] = 0;
        for (int b = 0; b < 256; b++) { encode_shift(&rc, 1, cnt[b], 16); cum[b + 1] = cum[b] + cnt[b]; }
        if (hdr_end) hdr_end->push_back(rc.datapos);
        for (unsigned i = 0; i < bs; i++) encode_freq(&rc, cnt[p[at + i]], cum[p[at + i]], bs);
        at += bs;
    }
    encode_freq(&rc, 1, 0, 2);
    done_encoding(&rc);
    Bytes out(rc.databuf, rc.databuf + rc.datapos);
    free_databuf(&rc);
    return out;
}
static std::vector<unsigned> plain_blocks(size_t n)
{
    std::vector<unsigned> b(n / kB, (unsigned)kB);
    b.push_back((unsigned)(n % kB));
    return b;
}
// What a decoder reports for `in` and a plane of n symbols: the symbols the stream held (more than n: only n are written),
// (size_t)-1 for a block of more than 60000 symbols.  Reading past the end yields zeros.  *past: how far behind the stream's end
// the decoder read -- a stream that reads "far" past it (three bytes per symbol of a block and more) is given up by the product,
// where exactly is not part of the format: such inputs are compared for memory safety only.
static size_t ref_decode(const Bytes& in, size_t n, Bytes* out, size_t* past)
{
    const size_t pad = 4 * 3 * kB;
    Bytes buf(in.size() + pad + 4096, 0);
    memcpy(buf.data(), in.data(), in.size());
    rangecoder rc;
    memset(&rc, 0, sizeof rc);
    rc.databuf = buf.data(); rc.datalen = buf.size(); rc.datapos = 0;
    (void)start_decoding(&rc);
    out->assign(n, 0xEE);
    size_t produced = 0;
    *past = 0;
    for (;;) {
        if (rc.datapos > in.size() + pad - 3 * kB - 1024) { *past = pad; return produced; }  // (the caller does not compare)
        if (!decode_culfreq(&rc, 2)) break;
        decode_update(&rc, 1, 1, 2);
        unsigned cnt[256], cum[257], bs = 0;
        cum[0] = 0;
        for (int b = 0; b < 256; b++) { cnt[b] = decode_short(&rc); bs += cnt[b]; cum[b + 1] = bs; }
        if (bs > kB) return (size_t)-1;
        Bytes owner(bs + 1);  // the symbol whose interval a cumulative frequency lies in
        for (int b = 0; b < 256; b++) memset(owner.data() + cum[b], b, cnt[b]);
        for (unsigned i = 0; i < bs; i++) {
            const unsigned cf = decode_culfreq(&rc, bs);
            const int s = owner[cf];
            decode_update(&rc, cnt[s], cum[s], bs);
            if (produced + i < n) (*out)[produced + i] = (uint8_t)s;
        }
        produced += bs;
        if (rc.datapos > in.size()) *past = rc.datapos - in.size();
    }
    done_decoding(&rc);
    if (rc.datapos > in.size() && rc.datapos - in.size() > *past) *past = rc.datapos - in.size();
    return produced;
}

// ---- planes.  A pattern is one letter per full block: 0 / m / f constant blocks of symbol 0 / 97 / 255, d dominant symbol,
// q four symbols, n noise; `rest` symbols of kind `rk` follow.
static void fill(uint8_t* p, size_t n, char kind)
{
    for (size_t i = 0; i < n; i++) {
        const unsigned r = rnd();
        p[i] = kind == '0' ? 0 : kind == 'm' ? 97 : kind == 'f' ? 255 : kind == 'd' ? ((r & 63) ? 97 : 98 + (r >> 8 & 1)) : kind == 'q' ? (uint8_t)(253 + (r & 3) - ((r & 3) == 3 ? 200 : 0)) : (uint8_t)(r & 255);
    }
}
struct Plane {
    Bytes sym, ref;
    std::vector<uint16_t> hist;
    size_t n = 0, limit = 0;
};
static Plane make_plane(const std::string& pattern, size_t rest = 0, char rk = 'n')
{
    Plane pl;
    pl.n = pattern.size() * kB + rest;
    pl.sym.resize(pl.n ? pl.n : 1);
    for (size_t b = 0; b < pattern.size(); b++) fill(pl.sym.data() + b * kB, kB, pattern[b]);
    fill(pl.sym.data() + pattern.size() * kB, rest, rk);
    pl.hist.assign((pl.n / kB + 1) * 256, 0);
    for (size_t i = 0; i < pl.n; i++) pl.hist[(i / kB) * 256 + pl.sym[i]]++;
    Bytes s(pl.sym.begin(), pl.sym.begin() + pl.n);
    pl.ref = ref_encode(s, plain_blocks(pl.n));
    pl.limit = wrrc::encode_bound_hist(pl.hist.data(), pl.n);
    return pl;
}

// ---- windows: exact-size buffers allocated afresh for every window, so ASan sees an access outside a window or to one that
// was handed back; refuses from `allow` on
struct Win {
    const uint8_t* plane; uint8_t* out; size_t chunk, allow; uint8_t* cur; size_t cur_first, cur_count;
    static uint8_t* fn(void* u, size_t first, size_t* count)
    {
        Win* w = (Win*)u;
        if (w->out && w->cur) memcpy(w->out + w->cur_first, w->cur, w->cur_count);
        delete[] w->cur; w->cur = nullptr;
        if (*count == 0 || first >= w->allow) return nullptr;
        const size_t c = *count < w->chunk ? *count : w->chunk;
        w->cur = new uint8_t[c]; w->cur_first = first; w->cur_count = c;
        if (w->plane) memcpy(w->cur, w->plane + first, c); else memset(w->cur, 0xEE, c);
        *count = c;
        return w->cur;
    }
};
static Win enc_win(const Plane& p, size_t blocks, size_t allow = (size_t)-1) { return Win{p.sym.data(), nullptr, blocks * kB, allow, nullptr, 0, 0}; }
static Win dec_win(uint8_t* out, size_t blocks, size_t allow = (size_t)-1) { return Win{nullptr, out, blocks * kB, allow, nullptr, 0, 0}; }

enum Route { kOne, kScalar, kVec, kPool };
static const char* route_name[] = {"plane", "planes", "planes_vec", "pool"};
static const size_t kGuard = 64;

// Encodes the planes by `route`: with their histograms (and limits) or without, whole or through windows of `wblocks` blocks.
// Output buffers have the documented size exactly.  lens[k] as the entry point reports.
static void encode_by(Route route, const std::vector<const Plane*>& ps, bool hist, size_t wblocks, std::vector<Bytes>* outs, std::vector<size_t>* lens,
                      const std::vector<const std::vector<uint16_t>*>* other_hists = nullptr, size_t allow = (size_t)-1)
{
    const int count = (int)ps.size();
    outs->assign(count, Bytes()); lens->assign(count, 0);
    std::vector<Win> win(count);
    std::vector<wrrc::PlaneWindow> io(count);
    std::vector<wrrc::PlaneJob> jobs(count);
    for (int k = 0; k < count; k++) {
        const uint16_t* h = hist ? (other_hists ? (*other_hists)[k]->data() : ps[k]->hist.data()) : nullptr;
        const size_t lim = h ? wrrc::encode_bound_hist(h, ps[k]->n) : 0;
        (*outs)[k].assign(h ? lim + wrrc::kFailedBlockSlack : wrrc::encode_bound(ps[k]->n), 0xEE);
        (*outs)[k].shrink_to_fit();
        wrrc::PlaneJob& j = jobs[k];
        j.kind = wrrc::PlaneJob::kEncode; j.src = ps[k]->sym.data(); j.n = ps[k]->n; j.dst = (*outs)[k].data(); j.hist = h; j.dst_limit = lim;
        if (wblocks) { win[k] = enc_win(*ps[k], wblocks, allow); io[k] = wrrc::PlaneWindow{Win::fn, &win[k]}; j.io = &io[k]; j.src = nullptr; }
    }
    if (route == kOne) {
        for (int k = 0; k < count; k++) {
            wrrc::PlaneJob& j = jobs[k];
            if (!wblocks && !hist) (*lens)[k] = wrrc::encode_plane(j.src, j.n, j.dst, nullptr);
            else if (!wblocks) (*lens)[k] = wrrc::encode_plane(j.src, j.n, j.dst, j.hist);
            else wrrc::encode_planes(1, &j.src, j.n, &j.dst, &j.hist, &(*lens)[k], &j.io, &j.dst_limit);
        }
    } else if (route == kScalar) {  // (encode_planes takes planes of one length)
        std::vector<const uint8_t*> sp(count); std::vector<uint8_t*> op(count); std::vector<const uint16_t*> hp(count);
        std::vector<const wrrc::PlaneWindow*> pio(count); std::vector<size_t> lim(count);
        for (int k = 0; k < count; k++) { sp[k] = jobs[k].src; op[k] = jobs[k].dst; hp[k] = jobs[k].hist; pio[k] = jobs[k].io; lim[k] = jobs[k].dst_limit; }
        wrrc::encode_planes(count, sp.data(), ps[0]->n, op.data(), hp.data(), lens->data(), pio.data(), lim.data());
    } else if (route == kVec) {  // (no histograms on this entry point)
        std::vector<const uint8_t*> sp(count); std::vector<uint8_t*> op(count); std::vector<size_t> ns(count);
        std::vector<const wrrc::PlaneWindow*> pio(count);
        for (int k = 0; k < count; k++) { sp[k] = jobs[k].src; op[k] = jobs[k].dst; ns[k] = jobs[k].n; pio[k] = jobs[k].io; }
        if (!wrrc::encode_planes_vec(count, sp.data(), ns.data(), op.data(), lens->data(), pio.data()))
            for (int k = 0; k < count; k++) { (*lens)[k] = ps[k]->ref.size(); memcpy((*outs)[k].data(), ps[k]->ref.data(), ps[k]->ref.size()); }  // no AVX-512 here
    } else {
        CHECK(wrrc::pool_run(jobs.data(), count), "the pool refused the jobs");
        for (int k = 0; k < count; k++) (*lens)[k] = jobs[k].result;
    }
    for (int k = 0; k < count; k++) { delete[] win[k].cur; win[k].cur = nullptr; }
}

// Decodes streams by `route` into planes of ns[k] symbols with guard bytes behind; whole or through windows.
static void decode_by(Route route, const std::vector<const Bytes*>& ins, const std::vector<size_t>& ns, size_t wblocks, std::vector<Bytes>* outs,
                      std::vector<size_t>* got, size_t allow = (size_t)-1)
{
    const int count = (int)ins.size();
    outs->assign(count, Bytes()); got->assign(count, 0);
    std::vector<Win> win(count);
    std::vector<wrrc::PlaneWindow> io(count);
    std::vector<wrrc::PlaneJob> jobs(count);
    std::vector<Bytes> exact(count);
    for (int k = 0; k < count; k++) {
        exact[k] = *ins[k]; exact[k].shrink_to_fit();  // exact size: ASan sees a read past len
        (*outs)[k].assign(ns[k] + kGuard, 0xEE);
        wrrc::PlaneJob& j = jobs[k];
        j.kind = wrrc::PlaneJob::kDecode; j.src = exact[k].data(); j.src_len = exact[k].size(); j.dst = (*outs)[k].data(); j.n = ns[k];
        if (wblocks) { win[k] = dec_win((*outs)[k].data(), wblocks, allow); io[k] = wrrc::PlaneWindow{Win::fn, &win[k]}; j.io = &io[k]; j.dst = nullptr; }
    }
    std::vector<const uint8_t*> ip(count); std::vector<uint8_t*> op(count); std::vector<size_t> len(count);
    std::vector<const wrrc::PlaneWindow*> pio(count);
    for (int k = 0; k < count; k++) { ip[k] = jobs[k].src; op[k] = jobs[k].dst; len[k] = jobs[k].src_len; pio[k] = jobs[k].io; }
    if (route == kOne) {
        for (int k = 0; k < count; k++) {
            if (!wblocks) (*got)[k] = wrrc::decode_plane(ip[k], len[k], op[k], ns[k]);
            else wrrc::decode_planes(1, &ip[k], &len[k], &op[k], ns[k], &(*got)[k], &pio[k]);
        }
    } else if (route == kScalar) wrrc::decode_planes(count, ip.data(), len.data(), op.data(), ns[0], got->data(), pio.data());
    else if (route == kVec) {
        if (!wrrc::decode_planes_vec(count, ip.data(), len.data(), op.data(), ns.data(), got->data(), pio.data()))
            for (int k = 0; k < count; k++) wrrc::decode_planes(1, &ip[k], &len[k], &op[k], ns[k], &(*got)[k], &pio[k]);  // no AVX-512 here
    } else {
        CHECK(wrrc::pool_run(jobs.data(), count), "the pool refused the jobs");
        for (int k = 0; k < count; k++) (*got)[k] = jobs[k].result;
    }
    for (int k = 0; k < count; k++) { delete[] win[k].cur; win[k].cur = nullptr; }
    for (int k = 0; k < count; k++)
        for (size_t g = 0; g < kGuard; g++) CHECK((*outs)[k][ns[k] + g] == 0xEE, "%s: decoder wrote past n (stream %d)", route_name[route], k);
}

static void expect_streams(const char* what, Route route, const std::vector<const Plane*>& ps, const std::vector<Bytes>& outs, const std::vector<size_t>& lens)
{
    for (size_t k = 0; k < ps.size(); k++)
        CHECK(lens[k] == ps[k]->ref.size() && !memcmp(outs[k].data(), ps[k]->ref.data(), lens[k]), "%s via %s: stream %zu differs from the per-symbol coder (len %zu, want %zu)",
              what, route_name[route], k, lens[k], ps[k]->ref.size());
}
static void expect_symbols(const char* what, Route route, const std::vector<const Plane*>& ps, const std::vector<Bytes>& outs, const std::vector<size_t>& got)
{
    for (size_t k = 0; k < ps.size(); k++)
        CHECK(got[k] == ps[k]->n && !memcmp(outs[k].data(), ps[k]->sym.data(), ps[k]->n), "%s via %s: decoded plane %zu differs (got %zu of %zu)", what, route_name[route], k, got[k], ps[k]->n);
}
// a set of planes through one route, both directions, with and without histograms, whole and through windows
static void round_trips(const char* what, Route route, const std::vector<const Plane*>& ps, const std::vector<size_t>& windows)
{
    std::vector<Bytes> outs; std::vector<size_t> lens;
    std::vector<const Bytes*> ins; std::vector<size_t> ns;
    for (const Plane* p : ps) { ins.push_back(&p->ref); ns.push_back(p->n); }
    for (size_t w : windows) {
        for (int hist = 0; hist < 2; hist++) {
            if (hist && route == kVec) continue;
            encode_by(route, ps, hist != 0, w, &outs, &lens);
            expect_streams(what, route, ps, outs, lens);
        }
        decode_by(route, ins, ns, w, &outs, &lens);
        expect_symbols(what, route, ps, outs, lens);
    }
}

// stream-blocks of two loop kinds so far.  (A worker books a step after the step's streams have reported their ends, so the
// figures are complete only once the workers have been joined: the pool is stopped and started again.)
static double pool_blocks(int kind_a, int kind_b)
{
    wrrc::pool_configure(0, 0);
    wrrc::pool_configure(2, 4);
    double s[wrrc::kLoopKinds], b[wrrc::kLoopKinds];
    wrrc::pool_loop_stats(s, b);
    return b[kind_a] + b[kind_b];
}

int main()
{
    // ---- the planes: 4 to 12 blocks
    std::vector<Plane> eq;  // six blocks and a rest: one length, for the entry points that take one
    for (const char* pat : {"mmmmmm", "mmmdnq", "dnmmmq", "dqnmmm", "0dfnmq", "mdmnmq", "0f0f0f"}) eq.push_back(make_plane(pat, 4321, 'd'));
    eq.push_back(make_plane("dnmmmm", 4321, 'm'));  // a constant run in front of a partial block that is constant too
    std::vector<Plane> mixed;  // any lengths
    mixed.push_back(make_plane("mmmm"));             // exactly k x 60000: the empty final block follows a constant one
    mixed.push_back(make_plane("ffffffffffff"));
    mixed.push_back(make_plane("0000d", 17, '0'));
    mixed.push_back(make_plane("dmmmmmmn", 59999, 'n'));
    mixed.push_back(make_plane("nnmmq", 1, 'f'));
    mixed.push_back(make_plane("mdmdmdmd", 30000, 'm'));
    mixed.push_back(make_plane("qqqq0000", 0));
    mixed.push_back(make_plane("fmf0mf0", 777, 'q'));
    mixed.push_back(make_plane("dddd", 5000, 'd'));
    std::vector<const Plane*> all;
    for (const Plane& p : eq) all.push_back(&p);
    for (const Plane& p : mixed) all.push_back(&p);

    // ---- every plane alone
    round_trips("alone", kOne, all, {0, 1, 2, 5});
    // ---- encode_planes / decode_planes: 2, 3 and 4 streams of different patterns (and more than a loop holds)
    for (int count : {2, 3, 4, 8})
        for (int first = 0; first + count <= (int)eq.size(); first += 2) {
            std::vector<const Plane*> ps;
            for (int k = 0; k < count; k++) ps.push_back(&eq[first + k]);
            round_trips("interleaved", kScalar, ps, first ? std::vector<size_t>{0, 2} : std::vector<size_t>{0, 1, 2, 5});
        }
    // ---- the 16-lane loops: 5 and 16 streams of mixed patterns and unequal lengths
    for (int count : {5, 16}) {
        std::vector<const Plane*> ps;
        for (int k = 0; k < count; k++) ps.push_back(all[(k * 5 + count) % all.size()]);
        round_trips("16 lanes", kVec, ps, {0, 1, 2, 5});
    }
    // ---- the pool: 2 workers, a hand-over as soon as one of them is idle; block counts as without the pass
    {
        wrrc::pool_configure(2, 4);
        wrrc::pool_test_steal_idle_min(1);
        std::vector<const Plane*> ps;
        for (int rep = 0; rep < 2; rep++) for (const Plane* p : all) ps.push_back(p);
        double blocks = 0;
        for (const Plane* p : ps) blocks += (double)(p->n / kB + 1);
        const unsigned long moved0 = wrrc::pool_streams_moved();
        for (int rep = 0; rep < 3; rep++) {
            std::vector<Bytes> outs; std::vector<size_t> lens;
            for (int hist = 0; hist < 2; hist++) {
                const double e0 = pool_blocks(0, 3);
                encode_by(kPool, ps, hist != 0, rep == 1 ? 2 : 0, &outs, &lens);
                expect_streams("pool", kPool, ps, outs, lens);
                // a stream is in its session for one step per block, the final (partial or empty) one included
                CHECK(pool_blocks(0, 3) - e0 == blocks, "pool: encoder stream-blocks %.0f, want %.0f", pool_blocks(0, 3) - e0, blocks);
            }
            std::vector<const Bytes*> ins; std::vector<size_t> ns;
            for (const Plane* p : ps) { ins.push_back(&p->ref); ns.push_back(p->n); }
            const double d0 = pool_blocks(1, 2);
            decode_by(kPool, ins, ns, rep == 1 ? 2 : 0, &outs, &lens);
            expect_symbols("pool", kPool, ps, outs, lens);
            // ... and one more in which it reads "no more blocks"
            CHECK(pool_blocks(1, 2) - d0 == blocks + (double)ps.size(), "pool: decoder stream-blocks %.0f, want %.0f", pool_blocks(1, 2) - d0, blocks + (double)ps.size());
        }
        printf("streams that changed workers: %lu\n", wrrc::pool_streams_moved() - moved0);
        wrrc::pool_test_steal_idle_min(0);
        wrrc::pool_configure(0, 0);
    }

    // ---- a window that is refused in the middle of a pass: the stream is given up, its neighbours are not disturbed
    {
        std::vector<const Plane*> ps = {&eq[0], &eq[1], &eq[2], &eq[3], &eq[4]};  // eq[0]: all constant; windows of one block, refused from block 3 on
        std::vector<const Bytes*> ins; std::vector<size_t> ns;
        for (const Plane* p : ps) { ins.push_back(&p->ref); ns.push_back(p->n); }
        for (Route route : {kOne, kScalar, kVec}) {
            std::vector<Bytes> outs; std::vector<size_t> lens;
            encode_by(route, ps, false, 1, &outs, &lens, nullptr, 3 * kB);
            for (size_t k = 0; k < ps.size(); k++) CHECK(lens[k] == (size_t)-1, "refused window, encoder via %s: stream %zu reports %zu", route_name[route], k, lens[k]);
            decode_by(route, ins, ns, 1, &outs, &lens, 3 * kB);
            for (size_t k = 0; k < ps.size(); k++) CHECK(lens[k] == (size_t)-1, "refused window, decoder via %s: stream %zu reports %zu", route_name[route], k, lens[k]);
        }
    }
    // ---- a decoder window with less than a block of room when a constant block comes: blocks shorter than 60000 symbols in
    // mid-stream (the format allows them) shift the constant blocks against the windows
    for (int trial = 0; trial < 4; trial++) {
        std::vector<Plane> rag(5);
        std::vector<const Plane*> ps;
        for (int k = 0; k < 5; k++) {
            std::vector<unsigned> blocks = {(unsigned)kB, 1234u + 100u * k, (unsigned)kB, (unsigned)kB, 0u, (unsigned)kB, 59000u, (unsigned)kB, (unsigned)kB, 77u};
            if (trial & 1) blocks.insert(blocks.begin(), 1u);
            Plane& pl = rag[k];
            for (unsigned bs : blocks) pl.n += bs;
            pl.sym.resize(pl.n);
            size_t at = 0;
            for (size_t b = 0; b < blocks.size(); b++) { fill(pl.sym.data() + at, blocks[b], (b + k + trial) % 3 == 0 ? 'd' : "0mf"[(b + k) % 3]); at += blocks[b]; }
            pl.ref = ref_encode(pl.sym, blocks);
            ps.push_back(&pl);
        }
        std::vector<const Bytes*> ins; std::vector<size_t> ns;
        for (const Plane* p : ps) { ins.push_back(&p->ref); ns.push_back(p->n); }
        for (Route route : {kOne, kVec})
            for (size_t w : {(size_t)0, (size_t)1, (size_t)2, (size_t)5}) {
                std::vector<Bytes> outs; std::vector<size_t> got;
                decode_by(route, ins, ns, w, &outs, &got);
                expect_symbols("short blocks in mid-stream", route, ps, outs, got);
            }
    }

    // ---- histograms that say "constant" over symbols that are not: (size_t)-1, writes inside the documented bound
    {
        wrrc::pool_configure(2, 4);
        const size_t victim_block = 2;  // eq[0] and eq[1] are constant (97) there
        for (int variant = 0; variant < 4; variant++) {
            // one symbol differs at the first, a middle, the last position; or all symbols are another one than the histogram says
            std::vector<Plane> planes = {eq[0], eq[1], eq[2], eq[0], eq[5]};
            std::vector<int> victims = {0, 1, 3};
            for (int v : victims) {
                uint8_t* blk = planes[v].sym.data() + victim_block * kB;
                if (variant == 0) blk[0] = 96; else if (variant == 1) blk[31234] = 98; else if (variant == 2) blk[kB - 1] = 255; else memset(blk, 98, kB);
            }
            for (int extra = 0; extra < 16; extra++) planes.push_back(eq[(extra * 3 + 1) % eq.size()]);  // (enough for a 16-lane session in the pool)
            std::vector<const Plane*> ps;
            for (const Plane& p : planes) ps.push_back(&p);
            for (Route route : {kOne, kScalar, kPool}) {
                std::vector<Bytes> outs; std::vector<size_t> lens;
                encode_by(route, ps, true, 0, &outs, &lens);
                for (size_t k = 0; k < ps.size(); k++) {
                    const bool victim = k == 0 || k == 1 || k == 3;
                    if (victim) CHECK(lens[k] == (size_t)-1, "wrong histogram (variant %d) via %s: stream %zu did not fail (%zu)", variant, route_name[route], k, lens[k]);
                    else CHECK(lens[k] == ps[k]->ref.size() && !memcmp(outs[k].data(), ps[k]->ref.data(), lens[k]), "wrong histogram next door (variant %d) via %s: healthy stream %zu differs", variant, route_name[route], k);
                }
            }
        }
        wrrc::pool_configure(0, 0);
    }

    // ---- corrupt streams: cut at every byte of a header inside a constant run, bits flipped in such headers, and a forged stream
    // whose headers say "constant" for more blocks than the plane holds.  What the decoder reports and writes must be what the
    // per-symbol decoder does; no write past n, no read past len (exact-size buffers, guard bytes).
    {
        const Plane healthy[4] = {make_plane("mmmm", 5, 'm'), make_plane("dfff", 100, 'd'), make_plane("0000"), make_plane("mdmd", 60, 'q')};
        // (a stream of a few KB: the product then reads its end from a zero-padded copy and gives a stream up only when it has read
        // three blocks' worth of bytes past the end, far beyond what `comparable` below admits)
        Plane vic = make_plane("dmmm", 300, 'd');
        std::vector<size_t> hdr_end;
        (void)ref_encode(Bytes(vic.sym.begin(), vic.sym.begin() + vic.n), plain_blocks(vic.n), &hdr_end);
        // the header of block 2 lies between the positions behind the headers of blocks 1 and 2 (both constant: nothing but headers there)
        const size_t h0 = hdr_end[1] - 8, h1 = hdr_end[2] + 8;
        std::vector<Bytes> bad;
        for (size_t cut = h0; cut <= h1; cut++) bad.push_back(Bytes(vic.ref.begin(), vic.ref.begin() + cut));
        for (int f = 0; f < 300; f++) {
            Bytes b(vic.ref);
            b[h0 + rnd() % (h1 - h0)] ^= (uint8_t)(1u << (rnd() & 7));
            if (f % 3 == 0) b[hdr_end[2] + rnd() % (hdr_end[3] - hdr_end[2])] ^= (uint8_t)(1u << (rnd() & 7));
            bad.push_back(b);
        }
        size_t compared = 0;
        for (size_t t = 0; t < bad.size(); t++) {
            Bytes want; size_t past = 0;
            const size_t res = ref_decode(bad[t], vic.n, &want, &past);
            const bool comparable = past <= kB;
            compared += comparable;
            for (Route route : {kOne, kVec}) {
                std::vector<const Bytes*> ins = {&bad[t]}; std::vector<size_t> ns = {vic.n};
                if (route == kVec) for (const Plane& h : healthy) { ins.push_back(&h.ref); ns.push_back(h.n); }
                if (route == kVec && !wrrc::decode_planes_vec(0, nullptr, nullptr, nullptr, nullptr, nullptr)) continue;
                std::vector<Bytes> outs; std::vector<size_t> got;
                decode_by(route, ins, ns, t % 5 == 4 ? 1 : 0, &outs, &got);
                if (comparable) {
                    CHECK(got[0] == res, "corrupt stream %zu via %s: reports %zu, the per-symbol decoder %zu", t, route_name[route], got[0], res);
                    const size_t written = res == (size_t)-1 ? 0 : res < vic.n ? res : vic.n;
                    if (res != (size_t)-1 && !(t % 5 == 4)) CHECK(!memcmp(outs[0].data(), want.data(), written), "corrupt stream %zu via %s: symbols differ from the per-symbol decoder's", t, route_name[route]);
                }
                for (size_t k = 1; k < ins.size(); k++)
                    CHECK(got[k] == ns[k] && !memcmp(outs[k].data(), healthy[k - 1].sym.data(), ns[k]), "corrupt stream %zu via %s: healthy stream %zu disturbed", t, route_name[route], k);
            }
        }
        CHECK(compared * 10 >= bad.size() * 9, "only %zu of %zu corrupt streams were comparable", compared, bad.size());
        // forged: nine constant blocks, planes of 6 blocks, of 6 blocks and a bit, of 5 blocks and most of one
        Bytes nine(9 * kB, 97);
        const Bytes forged = ref_encode(nine, std::vector<unsigned>(9, (unsigned)kB));
        for (size_t n : {6 * kB, 6 * kB + 100, 6 * kB - 1, (size_t)100}) {
            Bytes want; size_t past = 0;
            const size_t res = ref_decode(forged, n, &want, &past);
            CHECK(res == 9 * kB, "the per-symbol decoder on the forged stream: %zu", res);
            for (Route route : {kOne, kScalar, kVec})
                for (size_t w : {(size_t)0, (size_t)1, (size_t)2}) {
                    if (w && n < kB) continue;
                    std::vector<const Bytes*> ins(route == kOne ? 1 : 5, &forged); std::vector<size_t> ns(ins.size(), n);
                    std::vector<Bytes> outs; std::vector<size_t> got;
                    decode_by(route, ins, ns, w, &outs, &got);
                    for (size_t k = 0; k < ins.size(); k++)
                        CHECK(got[k] == res && !memcmp(outs[k].data(), want.data(), n), "forged stream via %s (n %zu, windows of %zu): reports %zu, want %zu", route_name[route], n, w, got[k], res);
                }
        }
    }
    if (fails) { printf("constant blocks: %d check(s) FAILED\n", fails); return 1; }
    printf("constant blocks run OK\n");
    return 0;
}
