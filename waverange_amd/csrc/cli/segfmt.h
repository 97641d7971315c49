// segfmt.h -- what wrenc / wrdec need to speak the segmented stream formats (WRS1 / WRS2 / WRS3, include/waverange_amd.h):
// the `--` options of their command lines, the library's stream-format and partial-decode symbols bound weakly, a read-only
// mapping of the .wrb file, and the tools' phase clock.
//
// The same sources link against the reference's libwaverange (tests/util.py::build_cli), which has none of these symbols:
// every one is declared weak here, as in batch.h, and is null there.  A tool asked for something that needs a null symbol
// says "not supported by this codec library" and exits with status 2 before it writes anything.
#pragma once
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../../include/waverange_amd.h"

extern "C" {
const char* wr_last_error(void) __attribute__((weak));
int wr_stream_format_parse(const char* text, int* format, unsigned* seg, unsigned* brick, unsigned* strands) __attribute__((weak));
int wr_set_stream_format(int format, unsigned seg, unsigned brick, unsigned strands) __attribute__((weak));
int wr_get_stream_format(int* format, unsigned* seg, unsigned* brick, unsigned* strands) __attribute__((weak));
int wr_stream_sniff(const unsigned char* data, size_t len) __attribute__((weak));
int wr_ctx_create(wr_ctx** ctx, int device, void* hip_stream) __attribute__((weak));
void wr_ctx_destroy(wr_ctx* ctx) __attribute__((weak));
int wr_lowres_dims(int nx, int ny, int nz, int level, int* bx, int* by, int* bz) __attribute__((weak));
int wr_decode_host_seg(wr_ctx* ctx, double* h_fld, int nx, int ny, int nz, const wr_enc_info* info, const unsigned char* data_enc, size_t data_len,
                       wr_timings* tm) __attribute__((weak));
int wr_decode_host_seg_f32(wr_ctx* ctx, float* h_fld, int nx, int ny, int nz, const wr_enc_info* info, const unsigned char* data_enc, size_t data_len,
                           wr_timings* tm) __attribute__((weak));
int wr_decode_host_seg_lowres(wr_ctx* ctx, double* h_out, int nx, int ny, int nz, int level, int max_planes, const wr_enc_info* info,
                              const unsigned char* data_enc, size_t data_len, wr_timings* tm) __attribute__((weak));
int wr_decode_host_seg_lowres_f32(wr_ctx* ctx, float* h_out, int nx, int ny, int nz, int level, int max_planes, const wr_enc_info* info,
                                  const unsigned char* data_enc, size_t data_len, wr_timings* tm) __attribute__((weak));
int wr_decode_host_seg_roi(wr_ctx* ctx, double* h_out, int nx, int ny, int nz, int level, int max_planes, const wr_box* roi,
                           const wr_enc_info* info, const unsigned char* data_enc, size_t data_len, wr_timings* tm) __attribute__((weak));
int wr_decode_host_seg_roi_f32(wr_ctx* ctx, float* h_out, int nx, int ny, int nz, int level, int max_planes, const wr_box* roi,
                               const wr_enc_info* info, const unsigned char* data_enc, size_t data_len, wr_timings* tm) __attribute__((weak));
}

// an encode to a byte budget (wrenc --ratio)
extern "C" {
int wr_encode_host_seg_budget(wr_ctx* ctx, const double* h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, size_t max_bytes,
                              double tol_min, unsigned seg, wr_enc_info* info, unsigned char* data_enc, size_t cap, wr_timings* tm,
                              wr_budget_result* res) __attribute__((weak));
int wr_encode_host_seg_budget_f32(wr_ctx* ctx, const float* h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, size_t max_bytes,
                                  double tol_min, unsigned seg, wr_enc_info* info, unsigned char* data_enc, size_t cap, wr_timings* tm,
                                  wr_budget_result* res) __attribute__((weak));
}

// an encode to a pointwise error bound (wrenc --maxerr)
extern "C" {
int wr_encode_host_seg_bounded(wr_ctx* ctx, const double* h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, double max_abs_err,
                               double tol_min, unsigned seg, unsigned brick, unsigned strands, wr_enc_info* info, unsigned char* data_enc, size_t cap,
                               wr_timings* tm, wr_bounded_result* res) __attribute__((weak));
int wr_encode_host_seg_bounded_f32(wr_ctx* ctx, const float* h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, double max_abs_err,
                                   double tol_min, unsigned seg, unsigned brick, unsigned strands, wr_enc_info* info, unsigned char* data_enc, size_t cap,
                                   wr_timings* tm, wr_bounded_result* res) __attribute__((weak));
}

// an encode to an RMS error or PSNR target (wrenc --rmse, --psnr)
extern "C" {
int wr_encode_host_seg_quality(wr_ctx* ctx, const double* h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, int norm, double target,
                               double tol_min, unsigned seg, unsigned brick, unsigned strands, wr_enc_info* info, unsigned char* data_enc, size_t cap,
                               wr_timings* tm, wr_quality_result* res) __attribute__((weak));
int wr_encode_host_seg_quality_f32(wr_ctx* ctx, const float* h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, int norm, double target,
                                   double tol_min, unsigned seg, unsigned brick, unsigned strands, wr_enc_info* info, unsigned char* data_enc, size_t cap,
                                   wr_timings* tm, wr_quality_result* res) __attribute__((weak));
}

// masked fields (wrenc_mssg --mask=bits, wrdec_mssg)
extern "C" {
size_t wr_mask_bound(size_t n, unsigned seg) __attribute__((weak));
int wr_mask_sniff(const unsigned char* data, size_t len) __attribute__((weak));
int wr_encode_host_seg_masked(wr_ctx* ctx, const double* h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, const double* cutoffvec,
                              unsigned seg, unsigned brick, unsigned strands, double below, wr_enc_info* info, unsigned char* data_enc, size_t cap,
                              wr_timings* tm, wr_mask_result* res) __attribute__((weak));
int wr_decode_host_seg_masked(wr_ctx* ctx, double* h_fld, int nx, int ny, int nz, const wr_enc_info* info, const unsigned char* data_enc, size_t data_len,
                              double fill, wr_timings* tm, wr_mask_result* res) __attribute__((weak));
// a masked field to a pointwise, RMS or PSNR target (wrenc_mssg --mask=bits --maxerr, --rmse, --psnr)
int wr_encode_host_seg_quality_masked(wr_ctx* ctx, const double* h_fld, int nx, int ny, int nz, int wtflag, int mx, int my, int mz, int norm, double target,
                                      double tol_min, unsigned seg, unsigned brick, unsigned strands, double below, wr_enc_info* info, unsigned char* data_enc,
                                      size_t cap, wr_timings* tm, wr_quality_result* res, wr_mask_result* mres) __attribute__((weak));
// the masked region / low-resolution decode (wrdec_mssg --level, --roi, --planes)
int wr_decode_host_seg_roi_masked(wr_ctx* ctx, double* h_out, int nx, int ny, int nz, int level, int max_planes, const wr_box* roi,
                                  const wr_enc_info* info, const unsigned char* data_enc, size_t data_len, double fill, wr_timings* tm,
                                  wr_mask_result* res) __attribute__((weak));
}

// the region decode over a batch of fields (wrdec --batch)
extern "C" {
int wr_decode_host_seg_roi_batch(wr_ctx* ctx, double* h_out, int nfields, int nx, int ny, int nz, int level, int max_planes, const wr_box* rois, int nroi,
                                 const wr_enc_info* infos, const unsigned char* const* data_encs, const size_t* data_lens, wr_timings* tm) __attribute__((weak));
int wr_decode_host_seg_roi_batch_f32(wr_ctx* ctx, float* h_out, int nfields, int nx, int ny, int nz, int level, int max_planes, const wr_box* rois, int nroi,
                                     const wr_enc_info* infos, const unsigned char* const* data_encs, const size_t* data_lens, wr_timings* tm) __attribute__((weak));
size_t wr_seg_roi_batch_device_bytes(int nfields, size_t n, int planes, unsigned seg, unsigned brick, unsigned strands, size_t out_elems) __attribute__((weak));
size_t wr_ctx_device_free_bytes(wr_ctx* ctx) __attribute__((weak));
// ... of masked records (wrdec_mssg --batch)
int wr_decode_host_seg_roi_batch_masked(wr_ctx* ctx, double* h_out, int nfields, int nx, int ny, int nz, int level, int max_planes, const wr_box* rois, int nroi,
                                        const wr_enc_info* infos, const unsigned char* const* data_encs, const size_t* data_lens, double fill, wr_timings* tm,
                                        wr_mask_result* res) __attribute__((weak));
size_t wr_seg_roi_batch_device_bytes_masked(int nfields, int nmasked, size_t n, int planes, unsigned seg, unsigned brick, unsigned strands, unsigned mask_seg,
                                            size_t out_elems) __attribute__((weak));
// the masked encode over a batch of fields (wrenc_mssg --mask=bits --batch)
int wr_encode_host_seg_batch_masked(wr_ctx* ctx, int nfields, const double* const* h_flds, int nx, int ny, int nz, int wtflag, int mx, int my, int mz,
                                    const double* const* cutoffvecs, unsigned seg, unsigned brick, unsigned strands, double below, wr_enc_info* infos,
                                    unsigned char* const* data_encs, const size_t* caps, wr_timings* tm, wr_mask_result* results) __attribute__((weak));
size_t wr_seg_batch_device_bytes_masked(int nfields, int nmasked, size_t n, int nlay, unsigned seg, unsigned brick, unsigned strands, int decode)
    __attribute__((weak));
}

namespace wrcli {

constexpr const char* kNotSupported = "not supported by this codec library";

// Takes the arguments that start with "--" out of argv (the reference's tools count their arguments: options must not be
// seen by that count) and returns the new argc.
inline int take_options(int argc, char** argv, std::vector<std::string>& options)
{
    int kept = 1;
    for (int i = 1; i < argc; i++) {
        if (strncmp(argv[i], "--", 2) == 0) options.push_back(argv[i]);
        else argv[kept++] = argv[i];
    }
    return kept;
}

// "--name=value": true and the value if `opt` is that option
inline bool option_value(const std::string& opt, const char* name, std::string* value)
{
    const std::string head = std::string("--") + name + "=";
    if (opt.compare(0, head.size(), head) != 0) return false;
    *value = opt.substr(head.size());
    return true;
}

// a whole decimal number (no sign, no blanks, at most 9 digits)
inline bool parse_uint(const std::string& s, int* v)
{
    if (s.empty() || s.size() > 9 || s.find_first_not_of("0123456789") != std::string::npos) return false;
    *v = atoi(s.c_str());
    return true;
}

// "x0:x1,y0:y1,z0:z1" -> box (half-open, in the order NX NY NZ)
inline bool parse_roi(const std::string& s, wr_box* b)
{
    int v[6], k = 0;
    size_t at = 0;
    for (int axis = 0; axis < 3; axis++) {
        const size_t comma = axis < 2 ? s.find(',', at) : s.size();
        if (comma == std::string::npos) return false;
        const std::string part = s.substr(at, comma - at);
        const size_t colon = part.find(':');
        if (colon == std::string::npos) return false;
        if (!parse_uint(part.substr(0, colon), &v[k]) || !parse_uint(part.substr(colon + 1), &v[k + 1])) return false;
        k += 2;
        at = comma + 1;
    }
    b->x0 = v[0]; b->x1 = v[1]; b->y0 = v[2]; b->y1 = v[3]; b->z0 = v[4]; b->z1 = v[5];
    return true;
}

// The stream format wrenc writes: --format=TEXT if given, else what the library's setting says (WR_STREAM_FORMAT, or the
// reference's stream).  false and a message for the user if the text does not parse or the library cannot do it.
inline bool choose_stream_format(const std::string* text, int* format, std::string* why)
{
    *format = 0;
    if (text) {
        if (!wr_stream_format_parse || !wr_set_stream_format) {
            if (*text == "ref") return true;  // the reference's stream is what every codec library writes
            *why = "--format=" + *text + ": " + kNotSupported;
            return false;
        }
        unsigned seg = 0, brick = 0, strands = 0;
        if (wr_stream_format_parse(text->c_str(), format, &seg, &brick, &strands) != 0 || wr_set_stream_format(*format, seg, brick, strands) != 0) {
            *why = std::string("--format: ") + wr_last_error();
            return false;
        }
        return true;
    }
    if (wr_get_stream_format && wr_get_stream_format(format, nullptr, nullptr, nullptr) != 0) {
        *why = wr_last_error();
        return false;
    }
    return true;
}

// whether a coded field is one of the segmented formats (what wr_stream_sniff says, for tools on a library without it)
inline bool is_segmented(const unsigned char* data, size_t len)
{
    return len >= 4 && data[0] == 'W' && data[1] == 'R' && data[2] == 'S' && data[3] >= '1' && data[3] <= '3';
}

// Explicit contexts for the tool's concurrent codec calls: one per call in flight, created on demand and kept
class ContextPool {
public:
    ContextPool() = default;
    ContextPool(const ContextPool&) = delete;
    ContextPool& operator=(const ContextPool&) = delete;
    ~ContextPool() { for (wr_ctx* c : free_) wr_ctx_destroy(c); }
    wr_ctx* borrow()  // nullptr: wr_last_error() says why
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (!free_.empty()) { wr_ctx* c = free_.back(); free_.pop_back(); return c; }
        }
        int dev = 0;
        if (const char* e = getenv("WR_DEVICE")) dev = atoi(e);
        wr_ctx* c = nullptr;
        return wr_ctx_create(&c, dev, nullptr) == 0 ? c : nullptr;
    }
    void give(wr_ctx* c) { std::lock_guard<std::mutex> lk(mu_); free_.push_back(c); }

private:
    std::mutex mu_;
    std::vector<wr_ctx*> free_;
};

// A file mapped read only: only the pages a reader touches are ever read.
class MappedFile {
public:
    MappedFile() = default;
    MappedFile(const MappedFile&) = delete;
    MappedFile& operator=(const MappedFile&) = delete;
    ~MappedFile()
    {
        if (p_ != MAP_FAILED && size_) munmap(p_, size_);
        if (fd_ >= 0) close(fd_);
    }
    bool open(const std::string& path)
    {
        fd_ = ::open(path.c_str(), O_RDONLY);
        if (fd_ < 0) return false;
        struct stat st;
        if (fstat(fd_, &st) != 0) return false;
        size_ = (size_t)st.st_size;
        if (!size_) return true;
        p_ = mmap(nullptr, size_, PROT_READ, MAP_PRIVATE, fd_, 0);
        return p_ != MAP_FAILED;
    }
    const unsigned char* data() const { return size_ ? static_cast<const unsigned char*>(p_) : nullptr; }
    size_t size() const { return size_; }

private:
    int fd_ = -1;
    void* p_ = MAP_FAILED;
    size_t size_ = 0;
};

// WR_CLI_TIMING=1: one line on stderr when the tool ends, with the seconds its threads have spent reading the input, inside
// the codec calls (summed over the fields, which overlap) and writing the output, and the wall time
class PhaseClock {
public:
    enum Phase { kRead = 0, kCodec = 1, kWrite = 2 };
    explicit PhaseClock(const char* tool) : tool_(tool), t0_(now())
    {
        const char* e = getenv("WR_CLI_TIMING");
        on_ = e && atoi(e);
    }
    ~PhaseClock()
    {
        if (on_) fprintf(stderr, "timing tool=%s read=%.3f codec_sum=%.3f write=%.3f total=%.3f\n", tool_, s_[0], s_[1], s_[2], now() - t0_);
    }
    static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    void add(Phase p, double since)
    {
        const double dt = now() - since;
        std::lock_guard<std::mutex> lk(mu_);
        s_[p] += dt;
    }

private:
    const char* tool_;
    double t0_, s_[3] = {0, 0, 0};
    bool on_ = false;
    std::mutex mu_;
};

}  // namespace wrcli
