// wrdec_mssg -- restore MSSG output compressed by wrenc_mssg / wrmssgenc; command line, prompts and files
// of the reference's wrmssgdec (src/mssg/mssg_dec.cpp):
//
//   wrdec_mssg ENCODED_NAME_PREFIX ENCODED_NAME_EXT EXTRACTED_NAME_PREFIX TYPE PRECISION ENDIANFLIP PROCID
//
// TYPE 0: PREFIX.ctl + PREFIX_h.enc + PREFIX_f.enc -> OUT.grd (+ a copy of the control file as OUT.ctl)
// TYPE 1: PREFIX.nmlst + PREFIX_h.enc/_f.enc      -> OUT.p_NNNN for every subdomain
// TYPE 2: PREFIX.nmlst + PREFIX_hNNNN.enc/_fNNNN.enc -> OUT.p_NNNN for subdomain PROCID
//
// A TYPE 0 "mask" record whose payload is a WRM1 blob (wrenc_mssg --mask=bits) is decoded together with the field record behind
// it by wr_decode_host_seg_masked, the undefined points coming back as the control file's `undef`; no option is needed.
//
// Options (taken out of the command line before its arguments are counted; TYPE 0 only, sets in a segmented stream format):
//   --level=R               the low-pass box of level R (0..4, default 0: the field's own resolution)
//   --roi=x0:x1,y0:y1,z0:z1 a half-open box in the coordinates of the box of level R, in the order NX NY NZ (default: all of it)
//   --planes=P              the first P quantizer planes only (default 0: all)
//   --batch=N               with one of the three above: up to N consecutive time records go through ONE call of
//                           wr_decode_host_seg_roi_batch_masked (at most two coder launches and one restore launch for all of
//                           them, masked or not); groups are cut further so that wr_seg_roi_batch_device_bytes_masked fits the
//                           device's free memory.  Default 1: a call per record.  OUT.grd is byte for byte the same; the records
//                           of a call that failed go the --batch=1 way, with its messages.
// With any of the first three OUT.grd holds that region of every time record; a bit-mask record and its field go through
// wr_decode_host_seg_roi_masked (undefined points: the control file's `undef`), an unmasked record through the plain region /
// low-resolution call.  The control file is not copied (its extents would be wrong): the region's extents are printed.  The
// run is refused with status 2, nothing written, for TYPE 1 / 2, for a record in the reference's stream format, for a mask
// record of the old kind (a coded field of doubles) and on a codec library without these calls.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <limits>
#include <sstream>
#include <string>
#include <vector>

#include "../../../include/waverange_amd.h"
#include "mssg_io.h"
#include "segfmt.h"

using namespace wrmssg;

namespace {

struct Params {
    std::string in_prefix, ext, out_prefix;
    int filetype = 0, outtype = 1, flip = 0, proc = 0;
};

struct Partial {  // --level, --roi, --planes, --batch
    int level = 0, planes = 0, batch = 1;
    bool have_roi = false;
    wr_box roi{0, 0, 0, 0, 0, 0};
};

[[noreturn]] void refuse(const std::string& why)
{
    std::cout << "Error: " << why << std::endl;
    std::cerr << "Error: " << why << std::endl;
    std::exit(2);
}

void get_params(int argc, char** argv, Params* p)
{
    std::cout << "usage: ./wrmssgdec ENCODED_NAME_PREFIX ENCODED_NAME_EXT EXTRACTED_NAME_PREFIX TYPE PRECISION ENDIANFLIP PROCID\n";
    std::cout << "where TYPE=(0: regular output; 1: backup united; 2: backup divided), PRECISION=(1:single; 2:double), "
                 "ENDIANFLIP=(0:no; 1:yes) and PROCID=(this proc id)\n";
    std::cout << "interactive mode if not enough arguments are passed.\n";
    std::string v[4];
    if (argc == 8) {  // mssg_dec.cpp:103-114
        std::cout << "automatic mode.";
        p->in_prefix = argv[1];
        p->ext = argv[2];
        p->out_prefix = argv[3];
        for (int k = 0; k < 4; k++) v[k] = argv[4 + k];
    } else {  // mssg_dec.cpp:116-131
        const char* ask[7] = {"Enter encoded data file name prefix []: ", "Enter encoded data file extension name [.enc]: ",
                              "Enter extracted data file name prefix []: ",
                              "Enter file type (0: regular output; 1: backup merged; 2: backup separated) [0]: ",
                              "Enter extracted data type (1: float; 2: double) [2]: ",
                              "Enter endian conversion (0: do not perform; 1: inversion) [1]: ", "Enter id of this proc [0]: "};
        std::string ans[7];
        for (int k = 0; k < 7; k++) { std::cout << ask[k]; std::getline(std::cin, ans[k]); }
        p->in_prefix = ans[0];
        p->ext = ans[1];
        p->out_prefix = ans[2];
        for (int k = 0; k < 4; k++) v[k] = ans[3 + k];
    }
    std::stringstream(v[0]) >> p->filetype;
    std::stringstream(v[1]) >> p->outtype;
    std::stringstream(v[2]) >> p->flip;
    std::stringstream(v[3]) >> p->proc;
}

void open_or_die(std::ifstream& f, const std::string& path, std::ios::openmode mode)
{
    f.open(path.c_str(), mode);
    if (!f) { std::cout << "Cannot read from " << path << std::endl; std::exit(1); }
}

// the ntot_enc payload bytes of a data set into buf (nothing to read for a constant field)
void read_dataset(std::ifstream& payload, const Coding& c, std::vector<unsigned char>& buf, size_t at = 0)
{
    if (buf.size() < at + c.ntot_enc) buf.resize(at + c.ntot_enc);
    payload.read(reinterpret_cast<char*>(buf.data() + at), (std::streamsize)c.ntot_enc);
}

// ... decoded into fld
void decode_buffer(const Coding& c, int nx, int ny, int nz, double* fld, std::vector<unsigned char>& buf)
{
    Coding m = c;  // decoding_wrap takes non-const pointers
    decoding_wrap(nx, ny, nz, fld, &m.tolabs, &m.midval, &m.halfspanval, &m.wlev, &m.nlay, &m.ntot_enc, m.deps_vec, m.minval_vec,
                  m.len_enc_vec, buf.data());
}

void decode_dataset(std::ifstream& payload, const Coding& c, int nx, int ny, int nz, double* fld, std::vector<unsigned char>& buf)
{
    read_dataset(payload, c, buf);
    decode_buffer(c, nx, ny, nz, fld, buf);
}

// wr_mask_sniff, or for a codec library without it the magic alone (decode_masked then says that the library cannot read it)
bool is_mask_blob(const std::vector<unsigned char>& buf, size_t len)
{
    return wr_mask_sniff ? wr_mask_sniff(buf.data(), len) != 0 : len >= 4 && memcmp(buf.data(), "WRM1", 4) == 0;
}

// A masked record: the WRM1 blob of `mask_len` bytes is in `blob`; the field record `c` follows in the payload.  The planes go in
// front of the blob, as wr_decode_host_seg_masked reads them.
void decode_masked(std::ifstream& payload, const Coding& c, size_t mask_len, int nx, int ny, int nz, double undef, double* fld,
                   std::vector<unsigned char>& blob, std::vector<unsigned char>& buf)
{
    if (!(wr_decode_host_seg_masked && wr_mask_sniff && wr_ctx_create && wr_ctx_destroy && wr_last_error)) {
        std::cout << "Error: a bit-mask record (WRM1): " << wrcli::kNotSupported << std::endl;
        std::exit(2);
    }
    read_dataset(payload, c, buf);
    if (buf.size() < c.ntot_enc + mask_len) buf.resize(c.ntot_enc + mask_len);
    memcpy(buf.data() + c.ntot_enc, blob.data(), mask_len);
    wr_enc_info info;
    memset(&info, 0, sizeof info);
    info.tolabs = c.tolabs; info.midval = c.midval; info.halfspanval = c.halfspanval;
    info.wlev = c.wlev; info.nlay = c.nlay; info.ntot_enc = c.ntot_enc;
    for (int l = 0; l < c.nlay && l < kNlayMax; l++) { info.deps_vec[l] = c.deps_vec[l]; info.minval_vec[l] = c.minval_vec[l]; info.len_enc_vec[l] = c.len_enc_vec[l]; }
    int dev = 0;
    if (const char* e = getenv("WR_DEVICE")) dev = atoi(e);
    wr_ctx* ctx = nullptr;
    int rc = wr_ctx_create(&ctx, dev, nullptr);
    if (rc == 0) {
        rc = wr_decode_host_seg_masked(ctx, fld, nx, ny, nz, &info, buf.data(), c.ntot_enc + mask_len, undef, nullptr, nullptr);
        if (rc != 0) std::cout << "Error: " << wr_last_error() << std::endl;
        wr_ctx_destroy(ctx);
    } else {
        std::cout << "Error: " << wr_last_error() << std::endl;
    }
    if (rc != 0) std::exit(1);
}

// ---- TYPE 0 (mssg_dec.cpp:152-331)
int regular_output(const Params& p, int nbytes)
{
    const std::string control = p.in_prefix + ".ctl";
    const GradsControl g = read_grads_control(control);
    std::cout << std::endl << "=== Parameters read from control file ===" << std::endl;
    std::cout << " dset=" << g.dset << " nx=" << g.nx << " ny=" << g.ny << " nz=" << g.nz << " nt=" << g.nt << " undef=" << g.undef
              << std::endl;
    const size_t ntot = (size_t)g.nx * (size_t)g.ny * (size_t)g.nz;
    if (p.in_prefix != p.out_prefix) copy_text_file(control, p.out_prefix + ".ctl");
    const std::string out_name = p.out_prefix + ".grd";
    std::ifstream header, payload;
    open_or_die(header, p.in_prefix + "_h" + p.ext, std::ios::in);
    open_or_die(payload, p.in_prefix + "_f" + p.ext, std::ios::in | std::ios::binary);
    std::string line;
    for (int j = 0; j < 8; j++) std::getline(header, line);  // the preamble written by the encoder
    std::vector<double> fld(ntot), mask;
    std::vector<unsigned char> buf, blob;
    for (int it = 0; it < g.nt; it++) {
        Coding c;
        std::string name = read_header_record(header, it, &c);
        for (size_t j = 0; j < ntot; j++) fld[j] = c.midval;
        bool masked = false;
        double mask_mid = 0;
        if (name == "mask") {  // a mask record precedes the field record of the same number (mssg_dec.cpp:233-273)
            if (c.ntot_enc > 0) read_dataset(payload, c, blob);
            if (c.ntot_enc > 0 && is_mask_blob(blob, c.ntot_enc)) {  // the undefined points as bits: one call restores the field
                const size_t mask_len = c.ntot_enc;
                name = read_header_record(header, it, &c);
                std::cout << "  decoding mask bits and fld_1d_rec, it=" << it << std::endl;
                decode_masked(payload, c, mask_len, g.nx, g.ny, g.nz, g.undef, fld.data(), blob, buf);
                write_field(out_name, p.flip != 0, nbytes, it, g.nx, g.ny, g.nz, g.nx, g.ny, 0, 0, fld.data());
                std::cout << "  wrote: fld_1d_rec[0]=" << fld[0] << " fld_1d_rec[last]=" << fld[ntot - 1] << std::endl;
                continue;
            }
            masked = true;
            mask.assign(ntot, c.midval);
            if (c.ntot_enc > 0) {
                std::cout << "  decoding mask_1d_rec, it=" << it << std::endl;
                decode_buffer(c, g.nx, g.ny, g.nz, mask.data(), blob);
                mask_mid = c.midval;
                // the two mask values sit on either side of the middle value: back to {undef, 0}
                for (size_t j = 0; j < ntot; j++) mask[j] = (mask[j] < c.midval) ? g.undef : 0;
                std::cout << "        min=" << g.undef << " max=" << 0 << std::endl;
                name = read_header_record(header, it, &c);
            }
        }
        if (c.ntot_enc > 0) {
            std::cout << "  decoding fld_1d_rec, it=" << it << std::endl;
            decode_dataset(payload, c, g.nx, g.ny, g.nz, fld.data(), buf);
            double lo = fld[0], hi = fld[0];
            for (size_t j = 0; j < ntot; j++) { lo = std::fmin(lo, fld[j]); hi = std::fmax(hi, fld[j]); }
            std::cout << "        min=" << lo << " max=" << hi << std::endl;
        }
        if (masked)
            for (size_t j = 0; j < ntot; j++)
                if (mask[j] < mask_mid) fld[j] = mask[j];
        write_field(out_name, p.flip != 0, nbytes, it, g.nx, g.ny, g.nz, g.nx, g.ny, 0, 0, fld.data());
        std::cout << "  wrote: fld_1d_rec[0]=" << fld[0] << " fld_1d_rec[last]=" << fld[ntot - 1] << std::endl;
    }
    return 0;
}

wr_enc_info info_of(const Coding& c)
{
    wr_enc_info info;
    memset(&info, 0, sizeof info);
    info.tolabs = c.tolabs; info.midval = c.midval; info.halfspanval = c.halfspanval;
    info.wlev = c.wlev; info.nlay = c.nlay; info.ntot_enc = c.ntot_enc;
    for (int l = 0; l < c.nlay && l < kNlayMax; l++) { info.deps_vec[l] = c.deps_vec[l]; info.minval_vec[l] = c.minval_vec[l]; info.len_enc_vec[l] = c.len_enc_vec[l]; }
    return info;
}

// ---- TYPE 0 with --level / --roi / --planes: a region of every time record
int regular_output_region(const Params& p, int nbytes, const Partial& pd)
{
    if (!(wr_decode_host_seg_roi_masked && wr_decode_host_seg_roi && wr_decode_host_seg_lowres && wr_lowres_dims && wr_ctx_create && wr_ctx_destroy &&
          wr_last_error))
        refuse(std::string("--level / --roi / --planes: ") + wrcli::kNotSupported);
    const std::string control = p.in_prefix + ".ctl";
    const GradsControl g = read_grads_control(control);
    std::cout << std::endl << "=== Parameters read from control file ===" << std::endl;
    std::cout << " dset=" << g.dset << " nx=" << g.nx << " ny=" << g.ny << " nz=" << g.nz << " nt=" << g.nt << " undef=" << g.undef
              << std::endl;
    int bx = 0, by = 0, bz = 0;
    if (wr_lowres_dims(g.nx, g.ny, g.nz, pd.level, &bx, &by, &bz) != 0) refuse(std::string("--level: ") + wr_last_error());
    wr_box roi{0, 0, 0, bx, by, bz};
    if (pd.have_roi) {
        roi = pd.roi;
        if (!(roi.x0 < roi.x1 && roi.x1 <= bx && roi.y0 < roi.y1 && roi.y1 <= by && roi.z0 < roi.z1 && roi.z1 <= bz))
            refuse("--roi: the region is empty or reaches outside the box of the level");
    }
    const int cx = roi.x1 - roi.x0, cy = roi.y1 - roi.y0, cz = roi.z1 - roi.z0;
    std::ifstream header, payload;
    open_or_die(header, p.in_prefix + "_h" + p.ext, std::ios::in);
    open_or_die(payload, p.in_prefix + "_f" + p.ext, std::ios::in | std::ios::binary);
    std::string line;
    // first the whole set's records are looked at, then the first byte is written
    struct Record { Coding c; size_t mask_len; std::streamoff at; };  // at: where its bytes start in the payload (the blob, then the planes)
    std::vector<Record> recs;
    std::streamoff at = 0;
    for (int j = 0; j < 8; j++) std::getline(header, line);  // the preamble written by the encoder
    auto starts_with = [&](unsigned long len, unsigned char* head4) {
        memset(head4, 0, 4);
        payload.read(reinterpret_cast<char*>(head4), (std::streamsize)(len < 4 ? len : 4));
        payload.seekg((std::streamoff)(len < 4 ? 0 : len - 4), std::ios::cur);
    };
    for (int it = 0; it < g.nt; it++) {
        Record r;
        r.mask_len = 0;
        unsigned char head4[4];
        std::string name = read_header_record(header, it, &r.c);
        if (name == "mask") {
            starts_with(r.c.ntot_enc, head4);
            if (r.c.ntot_enc < 4 || memcmp(head4, "WRM1", 4) != 0)
                refuse("time record " + std::to_string(it + 1) + ": a mask record of the old kind (a coded field): encode with --mask=bits for --level / --roi / --planes");
            r.mask_len = r.c.ntot_enc;
            (void)read_header_record(header, it, &r.c);
        }
        starts_with(r.c.ntot_enc, head4);
        if (r.c.ntot_enc > 0 && !wrcli::is_segmented(head4, r.c.ntot_enc < 4 ? r.c.ntot_enc : 4))
            refuse("time record " + std::to_string(it + 1) + ": --level / --roi / --planes need a segmented stream format (WR_STREAM_FORMAT=wrs1, wrs2 or wrs3 when encoding)");
        if (pd.planes > (int)r.c.nlay) refuse("--planes exceeds the planes of time record " + std::to_string(it + 1));
        if (pd.level > (int)r.c.wlev) refuse("--level exceeds the transform depth of time record " + std::to_string(it + 1));
        r.at = at;
        at += (std::streamoff)(r.mask_len + r.c.ntot_enc);
        recs.push_back(r);
    }
    payload.clear();
    payload.seekg(0, std::ios::beg);
    std::cout << " region: level=" << pd.level << " x=" << roi.x0 << ":" << roi.x1 << " y=" << roi.y0 << ":" << roi.y1 << " z=" << roi.z0 << ":" << roi.z1
              << " nx=" << cx << " ny=" << cy << " nz=" << cz << " nt=" << g.nt << std::endl;
    const std::string out_name = p.out_prefix + ".grd";
    int dev = 0;
    if (const char* e = getenv("WR_DEVICE")) dev = atoi(e);
    wr_ctx* ctx = nullptr;
    if (wr_ctx_create(&ctx, dev, nullptr) != 0) { std::cout << "Error: " << wr_last_error() << std::endl; std::exit(1); }
    const size_t count = (size_t)cx * cy * cz;
    std::vector<double> out(count);
    std::vector<unsigned char> buf;
    // the planes in front of the blob, as the masked calls read them; in the payload the blob comes first
    auto load = [&](const Record& r, std::vector<unsigned char>& to) {
        to.resize(r.c.ntot_enc + r.mask_len + 1);
        payload.clear();
        payload.seekg(r.at, std::ios::beg);
        payload.read(reinterpret_cast<char*>(to.data() + r.c.ntot_enc), (std::streamsize)r.mask_len);
        payload.read(reinterpret_cast<char*>(to.data()), (std::streamsize)r.c.ntot_enc);
    };
    auto wrote = [&](int it, const double* v) {
        write_field(out_name, p.flip != 0, nbytes, it, cx, cy, cz, cx, cy, 0, 0, v);
        std::cout << "  wrote: fld_1d_rec[0]=" << v[0] << " fld_1d_rec[last]=" << v[count - 1] << std::endl;
    };
    // a record through a call of its own (--batch=1, and the records of a batch call that failed)
    auto decode_one = [&](int it, const std::vector<unsigned char>& data) {
        const Record& r = recs[(size_t)it];
        const wr_enc_info info = info_of(r.c);
        const wr_box* box = pd.have_roi ? &roi : nullptr;
        int rc;
        if (r.mask_len) {
            std::cout << "  decoding mask bits and fld_1d_rec, it=" << it << std::endl;
            rc = wr_decode_host_seg_roi_masked(ctx, out.data(), g.nx, g.ny, g.nz, pd.level, pd.planes, box, &info, data.data(), r.c.ntot_enc + r.mask_len,
                                               g.undef, nullptr, nullptr);
        } else {
            std::cout << "  decoding fld_1d_rec, it=" << it << std::endl;
            rc = box ? wr_decode_host_seg_roi(ctx, out.data(), g.nx, g.ny, g.nz, pd.level, pd.planes, box, &info, data.data(), r.c.ntot_enc, nullptr)
                     : wr_decode_host_seg_lowres(ctx, out.data(), g.nx, g.ny, g.nz, pd.level, pd.planes, &info, data.data(), r.c.ntot_enc, nullptr);
        }
        if (rc != 0) { std::cout << "Error: " << wr_last_error() << std::endl; return rc; }
        wrote(it, out.data());
        return 0;
    };
    int rc = 0;
    if (pd.batch <= 1) {
        for (int it = 0; it < g.nt && rc == 0; it++) {
            load(recs[(size_t)it], buf);
            rc = decode_one(it, buf);
        }
        wr_ctx_destroy(ctx);
        return rc ? 1 : 0;
    }
    // ---- --batch=N: up to N consecutive records per call, cut further by the device's free memory and the job limit
    const size_t n = (size_t)g.nx * g.ny * g.nz;
    // what a record's call takes, by the headers of its used planes (magic, seg, nseg, then brick in a WRS2 / WRS3 header and
    // strands in a WRS3 one) and of its blob's plane; the library validates them, here they only size a call
    auto size_of = [&](const Record& r, const std::vector<unsigned char>& data, int* jobs) {
        const int used = r.c.ntot_enc ? (pd.planes ? pd.planes : (int)r.c.nlay) : 0;  // (a constant field has no job)
        unsigned seg = 0, brick = 0, strands = 0, mask_seg = 0;
        size_t off = 0;
        for (int l = 0; l < used && l < kNlayMax; off += r.c.len_enc_vec[l], l++) {
            if (off + 20 > r.c.ntot_enc) break;
            uint32_t w[5];
            memcpy(w, data.data() + off, sizeof w);
            if (!seg || w[1] < seg) seg = w[1];
            if (memcmp(data.data() + off, "WRS1", 4) != 0) brick = w[3];
            if (memcmp(data.data() + off, "WRS3", 4) == 0) strands = w[4];
        }
        if (r.mask_len >= 32 + 12) memcpy(&mask_seg, data.data() + r.c.ntot_enc + 32 + 4, 4);
        *jobs = used + (r.mask_len ? 1 : 0);
        return wr_seg_roi_batch_device_bytes_masked(1, r.mask_len ? 1 : 0, n, used, seg, brick, strands, mask_seg, count);
    };
    std::vector<std::vector<unsigned char>> datas;
    std::vector<double> outs;
    int a = 0;
    while (a < g.nt && rc == 0) {
        const int most = a + pd.batch < g.nt ? a + pd.batch : g.nt;
        const size_t budget = wr_ctx_device_free_bytes(ctx) / 4 * 3;
        datas.resize((size_t)(most - a));
        size_t need = 0, jobs = 0;
        int b = a;
        while (b < most) {
            // every record is sized as a call of its own and the sum holds the tables and the output once per record: an upper
            // bound of the group's call
            load(recs[(size_t)b], datas[(size_t)(b - a)]);
            int j = 0;
            const size_t one = size_of(recs[(size_t)b], datas[(size_t)(b - a)], &j);
            if (!one || need + one > budget || jobs + (size_t)j > WR_SEG_BATCH_MAX) break;  // (0: headers the library will refuse)
            need += one; jobs += (size_t)j; b++;
        }
        bool done = false;
        if (b - a >= 2) {
            const size_t nf = (size_t)(b - a);
            std::vector<wr_enc_info> infos(nf);
            std::vector<const unsigned char*> ptrs(nf);
            std::vector<size_t> lens(nf);
            for (size_t f = 0; f < nf; f++) {
                const Record& r = recs[(size_t)a + f];
                infos[f] = info_of(r.c); ptrs[f] = datas[f].data(); lens[f] = r.c.ntot_enc + r.mask_len;
            }
            outs.resize(nf * count);
            done = wr_decode_host_seg_roi_batch_masked(ctx, outs.data(), (int)nf, g.nx, g.ny, g.nz, pd.level, pd.planes, &roi, 1, infos.data(), ptrs.data(),
                                                       lens.data(), g.undef, nullptr, nullptr) == 0;
            for (size_t f = 0; f < nf && done; f++) {
                const int it = a + (int)f;
                std::cout << (recs[(size_t)it].mask_len ? "  decoding mask bits and fld_1d_rec, it=" : "  decoding fld_1d_rec, it=") << it << std::endl;
                wrote(it, outs.data() + f * count);
            }
        }
        if (!done) {
            if (b == a) b = a + 1;  // (its bytes are in datas[0])
            for (int it = a; it < b && rc == 0; it++) rc = decode_one(it, datas[(size_t)(it - a)]);
        }
        a = b;
    }
    wr_ctx_destroy(ctx);
    return rc ? 1 : 0;
}

// ---- TYPE 1 and 2 (mssg_dec.cpp:334-548)
int restart_set(const Params& p, int nbytes)
{
    const std::string control = p.in_prefix + ".nmlst";
    const RestartControl r = read_restart_control(control);
    const int nxloc = r.nx / r.nprocx, nyloc = r.ny / r.nprocy;
    const int ndset = (int)r.dsets.size();
    std::cout << std::endl << "=== Parameters read from control file ===" << std::endl;
    std::cout << "nx = " << r.nx << "; ny = " << r.ny << "; nr(=nz) = " << r.nz << "; dim_size(=nprocx,nprocy) = " << r.nprocx << ", "
              << r.nprocy << "; ndset = " << ndset << std::endl;
    for (int j = 0; j < ndset; j++) std::cout << "record number = " << j + 1 << "; field = " << r.dsets[j] << std::endl;
    const bool united = p.filetype == 1;
    const int fx = united ? r.nx : nxloc, fy = united ? r.ny : nyloc;
    const size_t ntot = (size_t)fx * (size_t)fy * (size_t)r.nz;
    if (p.in_prefix != p.out_prefix) copy_text_file(control, p.out_prefix + ".nmlst");
    const std::string lbl = subdomain_label(p.proc);
    std::ifstream header, payload;
    open_or_die(header, p.in_prefix + "_h" + (united ? "" : lbl) + p.ext, std::ios::in);
    open_or_die(payload, p.in_prefix + "_f" + (united ? "" : lbl) + p.ext, std::ios::in | std::ios::binary);
    std::vector<double> fld(ntot);
    std::vector<unsigned char> buf;
    for (int idset = 0; idset < ndset; idset++) {
        std::fill(fld.begin(), fld.end(), 0.0);
        if (united) std::cout << " dset=" << r.dsets[idset] << " nx=" << r.nx << " ny=" << r.ny << " nz=" << r.nz << std::endl;
        else std::cout << " dset=" << r.dsets[idset] << " nxloc=" << nxloc << " nyloc=" << nyloc << " nz=" << r.nz << std::endl;
        if (idset == 0) {
            // the time record comes back from the header text; every subdomain file starts with it
            // (mssg_dec.cpp:415-446)
            std::string line;
            for (int j = 0; j < 12; j++) std::getline(header, line);
            for (int j = 0; j < kTimeRecLen; j++) header >> fld[j];
            std::getline(header, line);
            std::cout << "  'time' record = ";
            for (int j = 0; j < kTimeRecLen; j++)
                std::cout << " " << std::setprecision(std::numeric_limits<long double>::digits10 + 1) << fld[j];
            std::cout << std::endl;
            if (united)
                for (int py = 0; py < r.nprocy; py++)
                    for (int px = 0; px < r.nprocx; px++)
                        if (px + py > 0)
                            for (int ix = 0; ix < kTimeRecLen; ix++)
                                fld[(size_t)(ix + px * nxloc) + (size_t)r.nx * (size_t)(py * nyloc)] = fld[ix];
        } else {
            Coding c;
            (void)read_header_record(header, idset, &c);
            if (c.ntot_enc > 0) {
                decode_dataset(payload, c, fx, fy, r.nz, fld.data(), buf);
                std::cout << "  decode: fld_1d_rec[0]=" << fld[0] << " fld_1d_rec[last]=" << fld[ntot - 1] << std::endl;
            } else {
                std::fill(fld.begin(), fld.end(), c.midval);  // all elements are equal (mssg_dec.cpp:492-496)
            }
        }
        if (united) {
            for (int py = 0; py < r.nprocy; py++)
                for (int px = 0; px < r.nprocx; px++)
                    write_field(p.out_prefix + ".p_" + subdomain_label(px + r.nprocx * py), p.flip != 0, nbytes, idset, r.nx, r.ny, r.nz,
                                nxloc, nyloc, px * nxloc, py * nyloc, fld.data());
        } else {
            write_field(p.out_prefix + ".p_" + lbl, p.flip != 0, nbytes, idset, nxloc, nyloc, r.nz, nxloc, nyloc, 0, 0, fld.data());
        }
        std::cout << "  wrote: fld_1d_rec[0]=" << fld[0] << " fld_1d_rec[last]=" << fld[ntot - 1] << std::endl;
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    std::vector<std::string> options;
    argc = wrcli::take_options(argc, argv, options);
    Partial pd;
    bool partial = false, batch = false;
    for (const std::string& o : options) {
        std::string v;
        bool good = false;
        if (wrcli::option_value(o, "level", &v)) good = wrcli::parse_uint(v, &pd.level) && pd.level <= 4;
        else if (wrcli::option_value(o, "roi", &v)) good = pd.have_roi = wrcli::parse_roi(v, &pd.roi);
        else if (wrcli::option_value(o, "planes", &v)) good = wrcli::parse_uint(v, &pd.planes);
        else if (wrcli::option_value(o, "batch", &v)) { good = wrcli::parse_uint(v, &pd.batch) && pd.batch >= 1; batch = true; }
        if (!good) {
            std::cout << "options (TYPE 0, segmented stream formats): --level=R (0..4) --roi=x0:x1,y0:y1,z0:z1 --planes=P --batch=N\n";
            refuse("bad option " + o);
        }
        if (!wrcli::option_value(o, "batch", &v)) partial = true;
    }
    if (batch && !partial) refuse("--batch groups the time records of a partial decode: give --level, --roi or --planes with it");
    if (pd.batch > 1 && !(wr_decode_host_seg_roi_batch_masked && wr_seg_roi_batch_device_bytes_masked && wr_ctx_device_free_bytes))
        refuse(std::string("--batch is ") + wrcli::kNotSupported);
    Params p;
    get_params(argc, argv, &p);
    const int nbytes = p.outtype == 1 ? 4 : 8;
    if (partial && p.filetype != 0) refuse("--level / --roi / --planes apply to TYPE 0 (regular output) only");
    std::cout << std::endl << "=== Decoding parameters ===" << std::endl;
    std::cout << "Encoded file name prefix: " << p.in_prefix << std::endl;
    std::cout << "Encoded file extension name: " << p.ext << std::endl;
    std::cout << "Extracted file name prefix: " << p.out_prefix << std::endl;
    std::cout << "File type (0: regular output; 1: backup merged; 2: backup separated): " << p.filetype << std::endl;
    std::cout << "Output files contain " << nbytes << "-byte floating point data" << std::endl;
    if (p.flip) std::cout << "Convert big endian to little endian or vice versa" << std::endl;
    std::cout << "This proc id: " << p.proc << std::endl;
    int rc = 0;
    if (p.filetype == 0) rc = partial ? regular_output_region(p, nbytes, pd) : regular_output(p, nbytes);
    else if (p.filetype == 1 || p.filetype == 2) rc = restart_set(p, nbytes);
    else std::cout << "Error: unknown file type" << std::endl;
    std::cout << "=== End of decompression ===\n";
    return rc;
}
