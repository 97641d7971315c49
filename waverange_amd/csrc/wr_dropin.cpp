// wr_dropin.cpp -- Part 1 of include/waverange_amd.h: the reference's own entry points (same unmangled symbols, argument
// order and meaning as libwaverange, src/core/wrappers.h:53,70,75,95,111,119; waveletcdf97_3d) on host pointers, on top of
// wr_encode_host / wr_decode_host / wr_transform_host.  "void + fatal" error behaviour as the reference's.  Also their fp32
// counterparts wr_encoding_wrap_f32 / wr_decoding_wrap_f32 (Part 2 of the header: not symbols of the reference).
// The implicit-context encoders write the process-wide stream format (wr_set_stream_format / WR_STREAM_FORMAT: the reference's
// stream unless told otherwise); the decoders read whatever format the coded bytes say.
#include "wr_blocked.h"
#include "wr_internal.h"
#include "wr_segcoder.h"
#include "wr_transcode.h"

using namespace wri;

namespace {

// The reference's entry points are re-entrant on distinct buffers (wrappers.cpp works on locals only).
// Here every call borrows a context from a free list (created on demand, kept for reuse), so concurrent
// callers never share staging; their device stages serialise on the per-GPU stage locks.
std::mutex g_free_mu;
std::vector<wr_ctx*> g_free_ctx;

[[noreturn]] void fatal(const char* where)
{
    fprintf(stderr, "libwaverange_amd: %s: %s\n", where, last_error().c_str());
    abort();
}

struct ImplicitCtx {
    wr_ctx* c = nullptr;
    explicit ImplicitCtx(const char* where)
    {
        {
            std::lock_guard<std::mutex> lk(g_free_mu);
            if (!g_free_ctx.empty()) { c = g_free_ctx.back(); g_free_ctx.pop_back(); }
        }
        if (!c) {
            int dev = 0;
            if (const char* e = getenv("WR_DEVICE")) dev = atoi(e);
            if (wr_ctx_create(&c, dev, nullptr) != WR_OK) fatal(where);
        }
    }
    ~ImplicitCtx()
    {
        std::lock_guard<std::mutex> lk(g_free_mu);
        g_free_ctx.push_back(c);
    }
};

// ---- the stream format of the implicit-context encoders (its normalisation is shared with the transcoder: wr_transcode.h)
using wrtc::StreamFormat;
using wrtc::kFormatNames;
using wrtc::format_normalise;

// The grammar of include/waverange_amd.h: NAME[:seg=N][:brick=B][:strands=K], keys in any order, each at most once.
bool format_parse(const char* text, StreamFormat* out, std::string* why)
{
    if (!text) { *why = "null format text"; return false; }
    const std::string s(text);
    const std::string where = "stream format \"" + s + "\": ";
    size_t at = s.find(':');
    const std::string name = s.substr(0, at);
    StreamFormat f;
    int k = 0;
    while (k < 4 && name != kFormatNames[k]) k++;
    if (k == 4) { *why = where + "unknown format name '" + name + "' (ref, wrs1, wrs2, wrs3)"; return false; }
    f.format = k;
    bool seen[3] = {false, false, false};
    while (at != std::string::npos) {
        const size_t next = s.find(':', at + 1);
        const std::string tok = s.substr(at + 1, next == std::string::npos ? std::string::npos : next - at - 1);
        at = next;
        const size_t eq = tok.find('=');
        const std::string key = tok.substr(0, eq), val = eq == std::string::npos ? "" : tok.substr(eq + 1);
        static const char* const keys[3] = {"seg", "brick", "strands"};
        int which = 0;
        while (which < 3 && key != keys[which]) which++;
        if (which == 3 || eq == std::string::npos) { *why = where + "'" + tok + "' is not seg=N, brick=B or strands=K"; return false; }
        if (seen[which]) { *why = where + "'" + tok + "': " + key + " is given twice"; return false; }
        seen[which] = true;
        if (val.empty() || val.size() > 9 || val.find_first_not_of("0123456789") != std::string::npos) { *why = where + "'" + tok + "': the value is not a number"; return false; }
        const unsigned v = (unsigned)strtoul(val.c_str(), nullptr, 10);
        std::string bad;
        if (f.format == WR_FORMAT_REF) bad = "ref takes no parameters";
        else if (which == 1 && f.format == WR_FORMAT_WRS1) bad = "wrs1 has no brick";
        else if (which == 2 && f.format != WR_FORMAT_WRS3) bad = "only wrs3 has strands";
        else if (which == 0 && !wrseg::seg_ok(v)) bad = "segment length must be a multiple of 16 in [16, 59999]";
        else if (which == 1 && !wrblk::brick_ok(v) && !(v == 0 && f.format == WR_FORMAT_WRS3)) bad = f.format == WR_FORMAT_WRS3 ? "brick edge must be one of 0, 8, 16, 32, 64" : "brick edge must be one of 8, 16, 32, 64";
        else if (which == 2 && !(v >= 1 && v <= wrseg::kStrandsMax && (v & (v - 1)) == 0)) bad = "strands must be one of 1, 2, 4, 8, 16, 32";
        if (!bad.empty()) { *why = where + "'" + tok + "': " + bad; return false; }
        (which == 0 ? f.seg : which == 1 ? f.brick : f.strands) = v;
    }
    std::string detail;
    if (!format_normalise(&f, &detail)) { *why = where + "'" + detail.substr(0, detail.find(':')) + "'" + detail.substr(std::min(detail.find(':'), detail.size())); return false; }
    *out = f;
    return true;
}

std::mutex g_fmt_mu;
StreamFormat g_fmt;            // what the implicit-context encoders write
int g_fmt_state = 0;           // 0: WR_STREAM_FORMAT not looked at yet; 1: g_fmt holds (from it, or from wr_set_stream_format); 2: it did not parse
std::string g_fmt_env_error;   // state 2: the parser's message

// The format in force; the environment is read once, by the first caller.  false: WR_STREAM_FORMAT did not parse (*why).
bool format_in_force(StreamFormat* out, std::string* why)
{
    std::lock_guard<std::mutex> lk(g_fmt_mu);
    if (g_fmt_state == 0) {
        g_fmt_state = 1;
        const char* e = getenv("WR_STREAM_FORMAT");
        if (e && *e && !format_parse(e, &g_fmt, &g_fmt_env_error)) { g_fmt_env_error = "WR_STREAM_FORMAT: " + g_fmt_env_error; g_fmt_state = 2; }
    }
    if (g_fmt_state == 2) { *why = g_fmt_env_error; return false; }
    *out = g_fmt;
    return true;
}

StreamFormat format_or_fatal(const char* where)
{
    StreamFormat f;
    std::string why;
    if (!format_in_force(&f, &why)) { last_error() = why; fatal(where); }  // no silent fall back to the reference's stream
    return f;
}

using wrtc::sniff;

}  // namespace

extern "C" {

int wr_stream_format_parse(const char* text, int* format, unsigned* seg, unsigned* brick, unsigned* strands)
{
    StreamFormat f;
    std::string why;
    if (!format_parse(text, &f, &why)) return fail(WR_ERR_ARG, why);
    if (format) *format = f.format;
    if (seg) *seg = f.seg;
    if (brick) *brick = f.brick;
    if (strands) *strands = f.strands;
    return WR_OK;
}

int wr_set_stream_format(int format, unsigned seg, unsigned brick, unsigned strands)
{
    StreamFormat f;
    f.format = format; f.seg = seg; f.brick = brick; f.strands = strands;
    std::string why;
    if (!format_normalise(&f, &why)) return fail(WR_ERR_ARG, "wr_set_stream_format: " + why);
    std::lock_guard<std::mutex> lk(g_fmt_mu);
    g_fmt = f;
    g_fmt_state = 1;  // overrides WR_STREAM_FORMAT, read or not
    return WR_OK;
}

int wr_get_stream_format(int* format, unsigned* seg, unsigned* brick, unsigned* strands)
{
    StreamFormat f;
    std::string why;
    if (!format_in_force(&f, &why)) return fail(WR_ERR_ARG, why);
    if (format) *format = f.format;
    if (seg) *seg = f.seg;
    if (brick) *brick = f.brick;
    if (strands) *strands = f.strands;
    return WR_OK;
}

int wr_stream_sniff(const unsigned char* data, size_t len) { return sniff(data, len); }

void setup_wr(int nx, int ny, int nz, unsigned char* nlaymax, unsigned long* ntot_enc_max)
{
    const unsigned long ntot = (unsigned long)nx * (unsigned long)ny * (unsigned long)nz;
    *nlaymax = WR_NLAYMAX;
    *ntot_enc_max = kSafetyBufferFactor * WR_NLAYMAX * (ntot < 1024ul ? 1024ul : ntot);
}

void encoding_wrap(int nx, int ny, int nz, double* fld_1d, int wtflag, int mx, int my, int mz, double* cutoffvec,
                   double* tolabs, double* midval, double* halfspanval, unsigned char* wlev, unsigned char* nlay,
                   unsigned long* ntot_enc, double* deps_vec, double* minval_vec, unsigned long* len_enc_vec,
                   unsigned char* data_enc)
{
    if (mx < 1 || my < 1 || mz < 1) { last_error() = "mx, my, mz must be >= 1"; fatal("encoding_wrap"); }
    const StreamFormat fmt = format_or_fatal("encoding_wrap");
    ImplicitCtx ic("encoding_wrap");
    unsigned char nl; unsigned long cap;
    setup_wr(nx, ny, nz, &nl, &cap);
    wr_enc_info info;
    ic.c->keep_residual = writeback_residual() != 0;  // fld_1d ends up holding the residual (wrappers.cpp:397-398)
    // (a segmented encode writes the residual back for fp64 host fields as wr_encode_host does, and an oversized stream
    // fails with the same message: only the bytes actually produced count against setup_wr's bound)
    const int rc = fmt.format == WR_FORMAT_WRS1 ? wr_encode_host_seg(ic.c, fld_1d, nx, ny, nz, wtflag, mx, my, mz, cutoffvec, fmt.seg, &info, data_enc, cap, nullptr)
                 : fmt.format == WR_FORMAT_WRS2 ? wr_encode_host_seg_blocked(ic.c, fld_1d, nx, ny, nz, wtflag, mx, my, mz, cutoffvec, fmt.seg, fmt.brick, &info, data_enc, cap, nullptr)
                 : fmt.format == WR_FORMAT_WRS3 ? wr_encode_host_seg_strands(ic.c, fld_1d, nx, ny, nz, wtflag, mx, my, mz, cutoffvec, fmt.seg, fmt.brick, fmt.strands, &info, data_enc, cap, nullptr)
                 : wr_encode_host(ic.c, fld_1d, nx, ny, nz, wtflag, mx, my, mz, cutoffvec, &info, data_enc, cap, nullptr);
    if (rc) fatal("encoding_wrap");
    *tolabs = info.tolabs; *midval = info.midval; *halfspanval = info.halfspanval;
    *wlev = info.wlev; *nlay = info.nlay; *ntot_enc = info.ntot_enc;
    for (int l = 0; l < info.nlay; l++) {
        deps_vec[l] = info.deps_vec[l];
        minval_vec[l] = info.minval_vec[l];
        len_enc_vec[l] = info.len_enc_vec[l];
    }
}

void decoding_wrap(int nx, int ny, int nz, double* fld_1d, double* tolabs, double* midval, double* halfspanval,
                   unsigned char* wlev, unsigned char* nlay, unsigned long* ntot_enc, double* deps_vec,
                   double* minval_vec, unsigned long* len_enc_vec, unsigned char* data_enc)
{
    (void)tolabs; (void)halfspanval;  // unused by the reference too (wrappers.h:62-64)
    ImplicitCtx ic("decoding_wrap");
    wr_enc_info info;
    memset(&info, 0, sizeof info);
    info.midval = *midval; info.wlev = *wlev; info.nlay = *nlay; info.ntot_enc = *ntot_enc;
    if (info.nlay > WR_NLAYMAX) { last_error() = "nlay > 8"; fatal("decoding_wrap"); }
    for (int l = 0; l < info.nlay; l++) {
        info.deps_vec[l] = deps_vec[l];
        info.minval_vec[l] = minval_vec[l];
        info.len_enc_vec[l] = len_enc_vec[l];
    }
    // the coded bytes say which format they are, whatever the encoders' setting is
    const bool segmented = info.ntot_enc >= 4 && sniff(data_enc, 4) > WR_FORMAT_REF;
    if (segmented ? wr_decode_host_seg(ic.c, fld_1d, nx, ny, nz, &info, data_enc, 0, nullptr)
                  : wr_decode_host(ic.c, fld_1d, nx, ny, nz, &info, data_enc, 0, nullptr))
        fatal("decoding_wrap");
}

void wr_encoding_wrap_f32(int nx, int ny, int nz, const float* fld_1d, int wtflag, int mx, int my, int mz, double* cutoffvec,
                          double* tolabs, double* midval, double* halfspanval, unsigned char* wlev, unsigned char* nlay,
                          unsigned long* ntot_enc, double* deps_vec, double* minval_vec, unsigned long* len_enc_vec,
                          unsigned char* data_enc)
{
    if (mx < 1 || my < 1 || mz < 1) { last_error() = "mx, my, mz must be >= 1"; fatal("wr_encoding_wrap_f32"); }
    const StreamFormat fmt = format_or_fatal("wr_encoding_wrap_f32");
    ImplicitCtx ic("wr_encoding_wrap_f32");
    unsigned char nl; unsigned long cap;
    setup_wr(nx, ny, nz, &nl, &cap);
    wr_enc_info info;
    ic.c->keep_residual = false;  // an fp32 field never takes the residual back
    const int rc = fmt.format == WR_FORMAT_WRS1 ? wr_encode_host_seg_f32(ic.c, fld_1d, nx, ny, nz, wtflag, mx, my, mz, cutoffvec, fmt.seg, &info, data_enc, cap, nullptr)
                 : fmt.format == WR_FORMAT_WRS2 ? wr_encode_host_seg_blocked_f32(ic.c, fld_1d, nx, ny, nz, wtflag, mx, my, mz, cutoffvec, fmt.seg, fmt.brick, &info, data_enc, cap, nullptr)
                 : fmt.format == WR_FORMAT_WRS3 ? wr_encode_host_seg_strands_f32(ic.c, fld_1d, nx, ny, nz, wtflag, mx, my, mz, cutoffvec, fmt.seg, fmt.brick, fmt.strands, &info, data_enc, cap, nullptr)
                 : wr_encode_host_f32(ic.c, fld_1d, nx, ny, nz, wtflag, mx, my, mz, cutoffvec, &info, data_enc, cap, nullptr);
    if (rc) fatal("wr_encoding_wrap_f32");
    *tolabs = info.tolabs; *midval = info.midval; *halfspanval = info.halfspanval;
    *wlev = info.wlev; *nlay = info.nlay; *ntot_enc = info.ntot_enc;
    for (int l = 0; l < info.nlay; l++) {
        deps_vec[l] = info.deps_vec[l];
        minval_vec[l] = info.minval_vec[l];
        len_enc_vec[l] = info.len_enc_vec[l];
    }
}

void wr_decoding_wrap_f32(int nx, int ny, int nz, float* fld_1d, double* tolabs, double* midval, double* halfspanval,
                          unsigned char* wlev, unsigned char* nlay, unsigned long* ntot_enc, double* deps_vec,
                          double* minval_vec, unsigned long* len_enc_vec, unsigned char* data_enc)
{
    (void)tolabs; (void)halfspanval;
    ImplicitCtx ic("wr_decoding_wrap_f32");
    wr_enc_info info;
    memset(&info, 0, sizeof info);
    info.midval = *midval; info.wlev = *wlev; info.nlay = *nlay; info.ntot_enc = *ntot_enc;
    if (info.nlay > WR_NLAYMAX) { last_error() = "nlay > 8"; fatal("wr_decoding_wrap_f32"); }
    for (int l = 0; l < info.nlay; l++) {
        info.deps_vec[l] = deps_vec[l];
        info.minval_vec[l] = minval_vec[l];
        info.len_enc_vec[l] = len_enc_vec[l];
    }
    const bool segmented = info.ntot_enc >= 4 && sniff(data_enc, 4) > WR_FORMAT_REF;
    if (segmented ? wr_decode_host_seg_f32(ic.c, fld_1d, nx, ny, nz, &info, data_enc, 0, nullptr)
                  : wr_decode_host_f32(ic.c, fld_1d, nx, ny, nz, &info, data_enc, 0, nullptr))
        fatal("wr_decoding_wrap_f32");
}

void setup_wr_f(int* nx, int* ny, int* nz, int* nlaymax, long* ntot_enc_max)
{
    const long ntot = (long)(*nx) * (long)(*ny) * (long)(*nz);
    *nlaymax = WR_NLAYMAX;
    *ntot_enc_max = (long)kSafetyBufferFactor * WR_NLAYMAX * (ntot < 1024L ? 1024L : ntot);
}

void encoding_wrap_f(int* nx, int* ny, int* nz, double* fld, int* wtflag, double* tolrel, double* tolabs,
                     double* midval, double* halfspanval, unsigned char* wlev, unsigned char* nlay, long* ntot_enc,
                     double* deps_vec, double* minval_vec, long* len_enc_vec, unsigned char* data_enc)
{
    unsigned long ne = 0, lens[WR_NLAYMAX] = {0};
    double cutoff = *tolrel;
    encoding_wrap(*nx, *ny, *nz, fld, *wtflag, 1, 1, 1, &cutoff, tolabs, midval, halfspanval, wlev, nlay, &ne,
                  deps_vec, minval_vec, lens, data_enc);
    *ntot_enc = (long)ne;
    for (int j = 0; j < WR_NLAYMAX; j++) len_enc_vec[j] = (long)lens[j];  // all 8, as wrappers.cpp:561-562
}

void decoding_wrap_f(int* nx, int* ny, int* nz, double* fld, double* midval, double* halfspanval,
                     unsigned char* wlev, unsigned char* nlay, long* ntot_enc, double* deps_vec,
                     double* minval_vec, long* len_enc_vec, unsigned char* data_enc)
{
    double tolabs = 0;
    unsigned long ne = (unsigned long)*ntot_enc, lens[WR_NLAYMAX];
    for (int j = 0; j < WR_NLAYMAX; j++) lens[j] = (unsigned long)len_enc_vec[j];
    decoding_wrap(*nx, *ny, *nz, fld, &tolabs, midval, halfspanval, wlev, nlay, &ne, deps_vec, minval_vec, lens, data_enc);
}

void waveletcdf97_3d(int n1, int n2, int n3, int lvl, double* x)
{
    ImplicitCtx ic("waveletcdf97_3d");
    if (wr_transform_host(ic.c, x, n1, n2, n3, lvl)) fatal("waveletcdf97_3d");
}

}  // extern "C"
