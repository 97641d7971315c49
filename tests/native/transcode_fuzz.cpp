// ASan/UBSan harness for the transcoder's host code (csrc/wr_transcode.h: the definition of wr_transcode_host, the containers
// of the segmented formats, the validation both forms of the call share), compiled by g++ into a program of its own.  Random
// planes and parameters go through every ordered pair of formats with exact-size buffers -- any over-read or over-write is
// ASan's -- and truncated and bit-flipped segmented inputs must be refused, or transcode to something, inside their bounds.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "wr_transcode.h"
static unsigned long long s = 88172645463325252ull;
static unsigned rnd() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (unsigned)(s >> 11); }

struct Stream {
    wr_enc_info info;
    std::vector<uint8_t> data;  // exact size
};

// the stream of `planes` in a normalised format, built plane by plane from the encoders the transcoder must agree with
static Stream make(const std::vector<std::vector<uint8_t>>& planes, int nx, int ny, int nz, int wlev, const wrtc::StreamFormat& f)
{
    Stream st;
    memset(&st.info, 0, sizeof st.info);
    st.info.tolabs = 1e-3; st.info.midval = 0.25; st.info.halfspanval = 2; st.info.wlev = (unsigned char)wlev; st.info.nlay = (unsigned char)planes.size();
    const size_t n = (size_t)nx * ny * nz;
    std::vector<uint8_t> out(wrtc::plane_bound(n, f)), perm(n);
    for (size_t l = 0; l < planes.size(); l++) {
        st.info.deps_vec[l] = 1.0 / (double)(l + 1); st.info.minval_vec[l] = -(double)l;
        const uint8_t* sym = planes[l].data();
        if (f.format != WR_FORMAT_REF && f.brick) { wrblk::reorder_host(wrblk::order_of(nx, ny, nz, wlev, f.brick), sym, perm.data(), false); sym = perm.data(); }
        int code = 0;
        std::string why;
        const size_t len = f.format == WR_FORMAT_REF ? wrrc::encode_plane(sym, n, out.data(), nullptr)
                           : f.format == WR_FORMAT_WRS3 ? wrtc::strands_encode_ref(sym, n, f.seg, f.brick, f.strands, out.data(), &code, &why)
                                                        : wrtc::seg_encode_ref(sym, n, f.seg, f.brick, out.data(), &code, &why);
        if (!len || len > out.size()) { printf("encoder failed: %s\n", why.c_str()); exit(1); }
        st.info.len_enc_vec[l] = len;
        st.info.ntot_enc += len;
        st.data.insert(st.data.end(), out.begin(), out.begin() + len);
    }
    st.data.shrink_to_fit();
    return st;
}

static wrtc::StreamFormat fmt(int format, unsigned seg, unsigned brick, unsigned strands)
{
    wrtc::StreamFormat f;
    f.format = format; f.seg = seg; f.brick = brick; f.strands = strands;
    std::string why;
    if (!wrtc::format_normalise(&f, &why)) { printf("format refused: %s\n", why.c_str()); exit(1); }
    return f;
}

static int run(const Stream& src, int nx, int ny, int nz, const wrtc::StreamFormat& t, wr_enc_info* info, std::vector<uint8_t>& out, std::string* why)
{
    return wrtc::transcode_ref(nx, ny, nz, &src.info, src.data.data(), src.data.size(), t.format, t.seg, t.brick, t.strands, info, out.data(), out.size(), why);
}

int main()
{
    const int shapes[][4] = {{1, 1, 1, 0}, {17, 1, 1, 0}, {9, 7, 5, 4}, {33, 18, 20, 4}, {40, 50, 30, 4}, {64, 31, 33, 0}};  // nx, ny, nz, wlev
    unsigned pairs = 0, refused = 0, survived = 0;
    for (const auto& sh : shapes) {
        const int nx = sh[0], ny = sh[1], nz = sh[2], wlev = sh[3];
        const size_t n = (size_t)nx * ny * nz;
        const int nlay = 1 + (int)(rnd() % 3);
        std::vector<std::vector<uint8_t>> planes((size_t)nlay, std::vector<uint8_t>(n));
        for (int l = 0; l < nlay; l++)
            for (size_t i = 0; i < n; i++) {
                const unsigned r = rnd();
                planes[l][i] = l == 0 ? ((r & 255) < 200 ? 128 : 120 + (r >> 8 & 15)) : l == 1 ? (uint8_t)(r & 255) : (uint8_t)((r & 1023) == 0 ? 255 : 1);
            }
        const unsigned seg = (rnd() & 1) ? 4096 : 16 * (1 + rnd() % 40), seg2 = n > 60000 ? 0 : 16 * (1 + rnd() % 300);
        const unsigned K = seg >= 512 ? 8 : 1;
        const wrtc::StreamFormat formats[] = {fmt(WR_FORMAT_REF, 0, 0, 0), fmt(WR_FORMAT_WRS1, seg, 0, 0), fmt(WR_FORMAT_WRS2, seg2, 8, 0), fmt(WR_FORMAT_WRS3, seg, 0, K),
                                              fmt(WR_FORMAT_WRS3, seg2, 16, 0 + (seg2 && seg2 < 128 ? 1 : 0))};
        std::vector<Stream> streams;
        for (const auto& f : formats) streams.push_back(make(planes, nx, ny, nz, wlev, f));
        for (size_t a = 0; a < streams.size(); a++)
            for (size_t b = 0; b < streams.size(); b++) {
                const Stream& want = streams[b];
                std::string why;
                wr_enc_info info;
                memset(&info, 0x5a, sizeof info);
                std::vector<uint8_t> out(want.data.size());  // exactly the bytes produced
                if (int rc = run(streams[a], nx, ny, nz, formats[b], &info, out, &why)) { printf("pair %zu -> %zu refused (%d): %s\n", a, b, rc, why.c_str()); return 1; }
                if (out != want.data || info.ntot_enc != want.info.ntot_enc || memcmp(info.len_enc_vec, want.info.len_enc_vec, sizeof info.len_enc_vec) ||
                    info.nlay != want.info.nlay || info.wlev != want.info.wlev || memcmp(info.deps_vec, want.info.deps_vec, sizeof info.deps_vec) ||
                    memcmp(info.minval_vec, want.info.minval_vec, sizeof info.minval_vec) || info.tolabs != want.info.tolabs || info.midval != want.info.midval ||
                    info.halfspanval != want.info.halfspanval) { printf("pair %zu -> %zu differs from the target's encoder (n=%zu)\n", a, b, n); return 1; }
                pairs++;
                // one byte short: refused, info_out untouched, nothing written past the buffer
                if (!out.empty()) {
                    std::vector<uint8_t> tight(want.data.size() - 1);
                    wr_enc_info keep;
                    memset(&keep, 0x5a, sizeof keep);
                    wr_enc_info got = keep;
                    if (run(streams[a], nx, ny, nz, formats[b], &got, tight, &why) != WR_ERR_OVERFLOW || memcmp(&got, &keep, sizeof keep)) { printf("short cap not refused\n"); return 1; }
                }
            }
        // damaged segmented sources: truncated (the lengths say so, or not) and bit-flipped, into every target
        for (size_t a = 1; a < streams.size(); a++)
            for (int trial = 0; trial < 40; trial++) {
                Stream bad = streams[a];
                const int what = trial % 4;
                if (what == 0) {  // cut short, the header not knowing
                    bad.data.resize(1 + rnd() % (bad.data.size() - 1));
                } else if (what == 1) {  // cut short, the header knowing: the last plane loses bytes
                    const size_t cut = 1 + rnd() % bad.info.len_enc_vec[nlay - 1];
                    bad.data.resize(bad.data.size() - cut); bad.info.len_enc_vec[nlay - 1] -= cut; bad.info.ntot_enc -= cut;
                } else if (what == 2) {  // flips in a header or index
                    size_t at = 0;
                    const int plane = (int)(rnd() % nlay);
                    for (int l = 0; l < plane; l++) at += bad.info.len_enc_vec[l];
                    bad.data[at + rnd() % (bad.data.size() - at < 40 ? bad.data.size() - at : 40)] ^= (uint8_t)(1 + rnd() % 255);
                } else {  // flips anywhere
                    for (int k = 0; k < 1 + trial / 8; k++) bad.data[rnd() % bad.data.size()] ^= (uint8_t)(1 + rnd() % 255);
                }
                bad.data.shrink_to_fit();
                const wrtc::StreamFormat& t = formats[rnd() % 5];
                std::vector<uint8_t> out(wrtc::plane_bound(n, t) * (size_t)nlay);
                out.shrink_to_fit();
                wr_enc_info info;
                std::string why;
                // (the true length is given: len_in = 0 trusts ntot_enc, as the decoders' data_len = 0 does)
                const int rc = wrtc::transcode_ref(nx, ny, nz, &bad.info, bad.data.data(), bad.data.size(), t.format, t.seg, t.brick, t.strands, &info, out.data(), out.size(), &why);
                if (what == 0) {
                    if (rc != WR_ERR_STREAM) { printf("a stream shorter than ntot_enc was not refused\n"); return 1; }
                    refused++;
                    continue;
                }
                if (rc == WR_OK) survived++;  // (a flip the coder cannot see: e.g. in a segment's unused last bytes)
                else if (rc == WR_ERR_STREAM && why.compare(0, 6, "plane ") == 0) refused++;
                else { printf("damaged input gave %d: %s\n", rc, why.c_str()); return 1; }
            }
    }
    // arguments
    {
        std::vector<std::vector<uint8_t>> planes(2, std::vector<uint8_t>(300, 3));
        const Stream st = make(planes, 10, 10, 3, 4, fmt(WR_FORMAT_WRS1, 64, 0, 0));
        std::vector<uint8_t> out(4096);
        wr_enc_info info;
        std::string why;
        if (wrtc::transcode_ref(10, 10, 3, &st.info, st.data.data(), st.data.size(), WR_FORMAT_WRS1, 17, 0, 0, &info, out.data(), out.size(), &why) != WR_ERR_ARG ||
            wrtc::transcode_ref(10, 10, 3, &st.info, st.data.data(), st.data.size(), WR_FORMAT_REF, 0, 8, 0, &info, out.data(), out.size(), &why) != WR_ERR_ARG ||
            wrtc::transcode_ref(10, 0, 3, &st.info, st.data.data(), st.data.size(), WR_FORMAT_REF, 0, 0, 0, &info, out.data(), out.size(), &why) != WR_ERR_ARG ||
            wrtc::transcode_ref(10, 10, 3, &st.info, st.data.data(), st.data.size(), WR_FORMAT_REF, 0, 0, 0, &info, const_cast<uint8_t*>(st.data.data()) + 5, 100, &why) != WR_ERR_ARG ||
            wrtc::transcode_ref(10, 10, 3, nullptr, st.data.data(), st.data.size(), WR_FORMAT_REF, 0, 0, 0, &info, out.data(), out.size(), &why) != WR_ERR_ARG) {
            printf("a bad argument was not refused\n");
            return 1;
        }
        // a trivial field: the header, nothing else is looked at
        wr_enc_info triv;
        memset(&triv, 0, sizeof triv);
        triv.midval = 7;
        if (wrtc::transcode_ref(10, 10, 3, &triv, nullptr, 0, WR_FORMAT_WRS3, 0, 0, 0, &info, nullptr, 0, &why) != WR_OK || info.midval != 7 || info.ntot_enc != 0) {
            printf("trivial field\n");
            return 1;
        }
    }
    printf("pairs=%u refused=%u survived=%u\n", pairs, refused, survived);
    if (!pairs || !refused) return 1;
    printf("transcode sanitizer run OK\n");
    return 0;
}
