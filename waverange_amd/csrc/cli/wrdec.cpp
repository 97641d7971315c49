// wrdec -- generic decoder command-line tool on top of libwaverange_amd.
//
// Same command line, prompts and output files as the reference's generic decoder
// (src/generic/gen_dec.cpp):   wrdec ENCODED_FILE HEADER_FILE EXTRACTED_FILE TYPE ENDIANFLIP
// A full decode needs no option: every coded field is whatever its bytes say, field by field -- the reference's plane streams go
// through the drop-in decoders, a segmented stream through wr_decode_host_seg on a context of the tool's, so that a damaged
// stream ends the tool with a message and exit status 1 (the drop-in decoders, void + fatal, abort the process).
// Arguments that start with "--" are options of this tool, taken out before the arguments are counted.  They select a PARTIAL
// decode of fields coded as segmented streams (waverange_amd.h: low-resolution and region decode):
//   --level=R               the low-pass box of level R (0..4, default 0: the field's own resolution)
//   --roi=x0:x1,y0:y1,z0:z1 a half-open box in the coordinates of the box of level R, in the order NX NY NZ (default: all of it);
//                           a field with nh > 1 is addressed as the array it was coded as, z in [0, nz*nh)
//   --planes=P              the first P quantizer planes only (default 0: all)
//   --field=K               field K only (default: every field)
//   --batch=N               up to N consecutive selected fields of one shape and precision go through ONE region-decode call
//                           (wr_decode_host_seg_roi_batch: at most two coder launches for all of them); groups are cut
//                           further so that wr_seg_roi_batch_device_bytes fits the device's free memory.  Default 1: a call
//                           per field.  The output file is byte for byte the same whatever N is.
// Any of --level > 0, --roi, --planes selects the partial path.  The output file then holds one record per selected field: the
// region's elements, x fastest, in the field's precision, with record markers for the region's byte count; the header's
// dimension inversion (idinv) is not applied.  The coded bytes are mapped, not read: only what the region needs is touched.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <future>
#include <memory>
#include <thread>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../../include/waverange_amd.h"
#include "batch.h"
#include "gen_io.h"
#include "segfmt.h"

using std::cout;
using std::endl;
using std::string;

namespace {

struct Partial {
    int level = 0, planes = 0, field = -1, batch = 1;
    bool have_roi = false, have_planes = false;
    wr_box roi{0, 0, 0, 0, 0, 0};
    bool selected() const { return level > 0 || have_roi || have_planes; }
};

// a selected field of the partial path that has passed the tool's checks
struct Ready {
    int it = 0, nx = 0, ny = 0, nz = 0, bx = 0, by = 0, bz = 0, nbytes = 8;
    unsigned nlay = 0;
    wr_box box{0, 0, 0, 0, 0, 0};
    wr_enc_info info;
    const unsigned char* data = nullptr;
    size_t len = 0;
    unsigned seg = 0, brick = 0, strands = 0;  // as the planes' headers say (the shortest seg of the used planes): what --batch sizes by
    wrio::FieldSpec record() const  // the record that is written: the region as an array of its own
    {
        wrio::FieldSpec rs;
        rs.nbytes = nbytes; rs.nx = box.x1 - box.x0; rs.ny = box.y1 - box.y0; rs.nz = box.z1 - box.z0; rs.nh = 1; rs.idinv = 0;
        return rs;
    }
    // seg, brick, strands from the front of the used planes' blobs (magic, seg, nseg, then brick in a WRS2 / WRS3 header and
    // strands in a WRS3 one); the library validates them, here they only size a call
    void read_headers(int max_planes)
    {
        const int used = max_planes ? max_planes : (int)nlay;
        size_t at = 0;
        for (int l = 0; l < used && l < WR_NLAYMAX; at += info.len_enc_vec[l], l++) {
            if (at + 20 > len) break;
            const unsigned char* const h = data + at;
            uint32_t w[5];
            memcpy(w, h, sizeof w);
            if (!seg || w[1] < seg) seg = w[1];
            if (memcmp(h, "WRS1", 4) != 0) brick = w[3];
            if (memcmp(h, "WRS3", 4) == 0) strands = w[4];
        }
    }
    // whether `next` may share a batch call with this one: the shape, the precision and hence the region are the same
    bool joins(const Ready& next) const { return nx == next.nx && ny == next.ny && nz == next.nz && nbytes == next.nbytes; }
};

void usage()
{
    cout << "usage: ./wrdec ENCODED_FILE HEADER_FILE EXTRACTED_FILE TYPE ENDIANFLIP\n";
    cout << "where TYPE=(0: Fortran sequential w 4-byte recl; 1: Fortran sequential w 8-byte recl; 2: C/C++) and ENDIANFLIP=(0:no; 1:yes)\n";
    cout << "interactive mode if not enough arguments are passed.\n";
}

void usage_options()
{
    cout << "options (partial decode of segmented streams): --level=R (0..4) --roi=x0:x1,y0:y1,z0:z1 --planes=P --field=K --batch=N\n";
}

// The partial path: one record per selected field.  Returns the exit status: 0, or 1 if any selected field was refused (a
// message names it and nothing is written for it).
int partial_decode(const Partial& pd, const string& in_name, const string& header_name, const string& out_name, int file_type, bool flip)
{
    std::ifstream fheader(header_name);
    if (!fheader.is_open()) { cout << "Cannot open " << header_name << endl; return 1; }
    const int nf = wrio::read_header_preamble(fheader);
    wrcli::MappedFile wrb;
    if (!wrb.open(in_name)) { cout << "Cannot open " << in_name << endl; return 1; }
    if (pd.field >= nf) { cout << "Error: field " << pd.field << " is not in the file (" << nf << " fields)" << endl; return 1; }
    wrcli::ContextPool contexts;
    wr_ctx* ctx = nullptr;
    int status = 0;
    bool first = true;
    size_t at = 0;  // of the field's bytes in the .wrb
    // a field that has passed the checks: decoded and written by decode_one, or with its neighbours by flush (--batch)
    auto write_record = [&](const Ready& r, const double* out, const float* out32) {
        cout << "  partial decode, field " << r.it << ": region [" << r.box.x0 << "," << r.box.x1 << ") x [" << r.box.y0 << "," << r.box.y1 << ") x [" << r.box.z0
             << "," << r.box.z1 << ") of the " << r.bx << " x " << r.by << " x " << r.bz << " box of level " << pd.level << ", ";
        if (pd.planes) cout << pd.planes << " of " << r.nlay << " planes"; else cout << "all " << r.nlay << " planes";
        cout << "; the order of the dimensions is not inverted (idinv is not applied to a partial output)" << endl;
        const wrio::FieldSpec rs = r.record();
        unsigned char recl[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // record markers of the region's byte count, native byte order
        const unsigned long long bytes = (unsigned long long)rs.count() * (unsigned long long)r.nbytes;
        memcpy(recl, &bytes, 8);
        if (out32) wrio::write_field(out_name, first, file_type, flip, rs, recl, out32);
        else wrio::write_field(out_name, first, file_type, flip, rs, recl, out);
        first = false;
    };
    auto decode_one = [&](const Ready& r) {
        const size_t count = r.record().count();
        std::unique_ptr<double[]> out;
        std::unique_ptr<float[]> out32;
        int rc;
        if (r.nbytes == 4) {
            out32.reset(new float[count]);
            rc = pd.have_roi ? wr_decode_host_seg_roi_f32(ctx, out32.get(), r.nx, r.ny, r.nz, pd.level, pd.planes, &r.box, &r.info, r.data, r.len, nullptr)
                             : wr_decode_host_seg_lowres_f32(ctx, out32.get(), r.nx, r.ny, r.nz, pd.level, pd.planes, &r.info, r.data, r.len, nullptr);
        } else {
            out.reset(new double[count]);
            rc = pd.have_roi ? wr_decode_host_seg_roi(ctx, out.get(), r.nx, r.ny, r.nz, pd.level, pd.planes, &r.box, &r.info, r.data, r.len, nullptr)
                             : wr_decode_host_seg_lowres(ctx, out.get(), r.nx, r.ny, r.nz, pd.level, pd.planes, &r.info, r.data, r.len, nullptr);
        }
        if (rc != 0) { cout << "Error: field " << r.it << ": " << wr_last_error() << endl; status = 1; return; }
        write_record(r, out.get(), out32.get());
    };
    std::vector<Ready> group;  // --batch: consecutive fields of one shape, precision and region, waiting for one call
    // the fields [a, b) of the group through one batch call; false: the call failed, nothing was written
    auto decode_many = [&](size_t a, size_t b) {
        const Ready& r0 = group[a];
        const size_t count = r0.record().count(), nfields = b - a;
        std::vector<wr_enc_info> infos(nfields);
        std::vector<const unsigned char*> datas(nfields);
        std::vector<size_t> lens(nfields);
        for (size_t f = 0; f < nfields; f++) { infos[f] = group[a + f].info; datas[f] = group[a + f].data; lens[f] = group[a + f].len; }
        std::unique_ptr<double[]> out;
        std::unique_ptr<float[]> out32;
        int rc;
        if (r0.nbytes == 4) {
            out32.reset(new float[count * nfields]);
            rc = wr_decode_host_seg_roi_batch_f32(ctx, out32.get(), (int)nfields, r0.nx, r0.ny, r0.nz, pd.level, pd.planes, &r0.box, 1, infos.data(), datas.data(), lens.data(), nullptr);
        } else {
            out.reset(new double[count * nfields]);
            rc = wr_decode_host_seg_roi_batch(ctx, out.get(), (int)nfields, r0.nx, r0.ny, r0.nz, pd.level, pd.planes, &r0.box, 1, infos.data(), datas.data(), lens.data(), nullptr);
        }
        if (rc != 0) return false;
        for (size_t f = 0; f < nfields; f++) write_record(group[a + f], out ? out.get() + f * count : nullptr, out32 ? out32.get() + f * count : nullptr);
        return true;
    };
    // The group in field order: cut into calls that fit the device's free memory and the job limit (a call of one field, and
    // the fields of a call that failed, go the way --batch=1 goes: the same messages, the same records)
    auto flush = [&]() {
        size_t a = 0;
        while (a < group.size()) {
            const Ready& r0 = group[a];
            const size_t budget = wr_ctx_device_free_bytes(ctx) / 4 * 3, n = (size_t)r0.nx * r0.ny * r0.nz, count = r0.record().count();
            size_t b = a, need = 0, jobs = 0;
            while (b < group.size()) {
                // every field is sized as a call of its own by what its headers say -- its used planes, its shortest seg, its brick
                // and strands --, and the sum holds the tables and the output once per field: an upper bound of the group's call
                const Ready& r = group[b];
                const int used = r.len ? (pd.planes ? pd.planes : (int)r.nlay) : 0;  // (a constant field has no job)
                const size_t one = wr_seg_roi_batch_device_bytes(1, n, used, r.seg, r.brick, r.strands, count);
                if (!one || need + one > budget || jobs + (size_t)used > WR_SEG_BATCH_MAX) break;  // (0: headers the library will refuse)
                need += one; jobs += (size_t)used; b++;
            }
            if (b - a < 2 || !decode_many(a, b)) {
                if (b == a) b = a + 1;
                for (size_t k = a; k < b; k++) decode_one(group[k]);
            }
            a = b;
        }
        group.clear();
    };
    for (int it = 0; it < nf; it++) {
        wrio::FieldHeader h;
        try { wrio::read_field_header(fheader, it, h); } catch (...) { status = 1; break; }
        const wrio::FieldSpec& s = h.spec;
        const size_t here = at, len = s.icomp ? (size_t)h.ntot_enc : s.count() * (size_t)s.nbytes;
        at += len;
        if (here + len > wrb.size()) { cout << "Error: field " << it << ": " << in_name << " is shorter than its header says" << endl; status = 1; break; }
        if (pd.field >= 0 && it != pd.field) continue;
        auto refuse = [&](const string& why) { flush(); cout << "Error: field " << it << ": " << why << endl; status = 1; };
        if (!s.icomp) { refuse("stored uncompressed (icomp = 0): there is no partial decode of it"); continue; }
        static const unsigned char kNoBytes[4] = {0, 0, 0, 0};
        const unsigned char* data = len ? wrb.data() + here : kNoBytes;  // (a constant field has no coded bytes)
        if (len > 0 && (len < 4 || wr_stream_sniff(data, len) < 1)) { refuse("not a segmented stream: the reference's plane streams decode only as a whole"); continue; }
        const int nx = s.nx, ny = s.ny, nz = s.nz * s.nh;  // nh > 1 folds into z, as it was coded
        if (len > 0 && pd.level > (int)h.wlev) { refuse("level " + std::to_string(pd.level) + " is above the stream's " + std::to_string(h.wlev) + " transform levels"); continue; }
        int bx = 0, by = 0, bz = 0;
        if (wr_lowres_dims(nx, ny, nz, pd.level, &bx, &by, &bz) != 0) { refuse(wr_last_error()); continue; }
        wr_box box{0, 0, 0, bx, by, bz};
        if (pd.have_roi) {
            box = pd.roi;
            if (box.x0 >= box.x1 || box.y0 >= box.y1 || box.z0 >= box.z1 || box.x1 > bx || box.y1 > by || box.z1 > bz) {
                refuse("the region is empty or outside the box of level " + std::to_string(pd.level) + ", " + std::to_string(bx) + " x " + std::to_string(by) + " x " + std::to_string(bz));
                continue;
            }
        }
        if (pd.planes > (int)h.nlay) { refuse(std::to_string(pd.planes) + " planes asked, the stream has " + std::to_string(h.nlay)); continue; }
        if (!ctx && !(ctx = contexts.borrow())) { cout << "Error: " << wr_last_error() << endl; return 1; }
        Ready r;
        r.it = it; r.nlay = h.nlay; r.nbytes = s.nbytes;
        r.nx = nx; r.ny = ny; r.nz = nz; r.bx = bx; r.by = by; r.bz = bz;
        r.box = box; r.data = data; r.len = len;
        memset(&r.info, 0, sizeof r.info);
        r.info.tolabs = h.tolabs; r.info.midval = h.midval; r.info.halfspanval = h.halfspanval;
        r.info.wlev = (unsigned char)h.wlev; r.info.nlay = (unsigned char)h.nlay; r.info.ntot_enc = h.ntot_enc;
        for (unsigned l = 0; l < h.nlay; l++) { r.info.deps_vec[l] = h.deps_vec[l]; r.info.minval_vec[l] = h.minval_vec[l]; r.info.len_enc_vec[l] = h.len_enc_vec[l]; }
        if (pd.batch <= 1) { decode_one(r); continue; }
        r.read_headers(pd.planes);
        if (!group.empty() && ((int)group.size() >= pd.batch || !group.back().joins(r))) flush();
        group.push_back(r);
    }
    flush();
    if (ctx) contexts.give(ctx);
    return status;
}

}  // namespace

int main(int argc, char** argv)
{
    std::vector<string> options;
    argc = wrcli::take_options(argc, argv, options);
    Partial pd;
    bool have_field = false;
    for (const string& o : options) {
        string v;
        bool good;
        if (wrcli::option_value(o, "level", &v)) good = wrcli::parse_uint(v, &pd.level) && pd.level <= 9;
        else if (wrcli::option_value(o, "roi", &v)) good = pd.have_roi = wrcli::parse_roi(v, &pd.roi);
        else if (wrcli::option_value(o, "planes", &v)) good = pd.have_planes = wrcli::parse_uint(v, &pd.planes);
        else if (wrcli::option_value(o, "field", &v)) good = have_field = wrcli::parse_uint(v, &pd.field);
        else if (wrcli::option_value(o, "batch", &v)) good = wrcli::parse_uint(v, &pd.batch) && pd.batch >= 1;
        else { usage(); usage_options(); cout << "Error: unknown option " << o << endl; return 2; }
        if (!good) { usage(); usage_options(); cout << "Error: " << o << " is not understood" << endl; return 2; }
    }
    if (have_field && !pd.selected()) { usage(); usage_options(); cout << "Error: --field selects fields of a partial decode: give --level, --roi or --planes with it" << endl; return 2; }
    if (pd.selected() && !(wr_stream_sniff && wr_ctx_create && wr_ctx_destroy && wr_lowres_dims && wr_last_error && wr_decode_host_seg_lowres &&
                           wr_decode_host_seg_lowres_f32 && wr_decode_host_seg_roi && wr_decode_host_seg_roi_f32)) {
        usage(); usage_options();
        cout << "Error: a partial decode is " << wrcli::kNotSupported << endl;
        return 2;
    }
    if (pd.batch > 1 && !pd.selected()) { usage(); usage_options(); cout << "Error: --batch groups fields of a partial decode: give --level, --roi or --planes with it" << endl; return 2; }
    if (pd.batch > 1 && !(wr_decode_host_seg_roi_batch && wr_decode_host_seg_roi_batch_f32 && wr_seg_roi_batch_device_bytes && wr_ctx_device_free_bytes)) {
        usage(); usage_options();
        cout << "Error: --batch is " << wrcli::kNotSupported << endl;
        return 2;
    }
    wrcli::PhaseClock clock("wrdec");
    string in_name = "data.wrb", header_name = "data.wrh", out_name = "datarec.bin";
    int file_type = 0, flip = 0;
    usage();
    if (argc == 6) {  // gen_dec.cpp:105-117
        cout << "automatic mode.";
        in_name = argv[1]; header_name = argv[2]; out_name = argv[3];
        std::stringstream(string(argv[4])) >> file_type;
        std::stringstream(string(argv[5])) >> flip;
    } else {  // gen_dec.cpp:118-135
        auto ask = [](const char* prompt) { cout << prompt; string s; std::getline(std::cin, s); return s; };
        string s;
        s = ask("Enter encoded data file name [data.wrb]: "); if (!s.empty()) in_name = s;
        s = ask("Enter encoding header file name [data.wrh]: "); if (!s.empty()) header_name = s;
        s = ask("Enter extracted (output) data file name [datarec.bin]: "); if (!s.empty()) out_name = s;
        s = ask("Enter file type (0: Fortran sequential w 4-byte recl; 1: Fortran sequential w 8-byte recl; 2: C/C++) [0]: ");
        if (!s.empty()) std::stringstream(s) >> file_type;
        s = ask("Enter endian conversion (0: do not perform; 1: inversion) [0]: ");
        if (!s.empty()) std::stringstream(s) >> flip;
    }
    cout << endl << "=== Decoding parameters ===" << endl;
    cout << "Encoded data file name " << in_name << endl;
    cout << "Encoding header file name " << header_name << endl;
    cout << "Extracted (output) data file name: " << out_name << endl;
    cout << "File type (0: Fortran sequential w 4-byte recl; 1: Fortran sequential w 8-byte recl; 2: C/C++): " << file_type << endl;
    if (flip) cout << "Convert big endian to little endian or vice versa" << endl;
    if (file_type < 0 || file_type > 2) {
        cout << "Error: unknown file type" << endl;
        cout << "=== End of decompression ===\n";
        return 0;
    }
    if (pd.selected()) {
        const int status = partial_decode(pd, in_name, header_name, out_name, file_type, flip != 0);
        cout << (status ? "=== decompression failed ===\n" : "=== End of decompression ===\n");
        return status;
    }

    std::ifstream fheader(header_name);
    if (!fheader.is_open()) { cout << "Cannot open " << header_name << endl; return 1; }
    const int nf = wrio::read_header_preamble(fheader);
    std::ifstream finput(in_name, std::ios::binary | std::ios::in);
    if (!finput.is_open()) { cout << "Cannot open " << in_name << endl; return 1; }

    // Field pipeline, as in wrenc (the reference decodes one field after the other, gen_dec.cpp:180-260): the main
    // thread reads field k's header record and coded bytes and hands them to a worker thread (decoding_wrap: host range
    // decoder, GPU kernels, download; min/max for the log), a writer thread writes finished fields to the output file
    // in field order; up to `depth` fields in flight (wr_autotune_batch, which also starts the library's coder pool;
    // WR_CLI_PIPELINE overrides, 0 = strictly one after the other).
    // fp32 records that were coded are decoded into fp32 by wr_decoding_wrap_f32 and written as they are (batch.h)
    const char* widen_env = getenv("WR_CLI_WIDEN_ON_HOST");
    const bool f32_codec = wr_decoding_wrap_f32 != nullptr && !(widen_env && atoi(widen_env));
    struct Item {
        wrio::FieldHeader h;
        std::unique_ptr<double[]> fld;   // not zero-filled: decoding_wrap writes every element
        std::unique_ptr<float[]> fld32;  // instead of fld: a coded fp32 record, decoded by wr_decoding_wrap_f32
        wrcli::RawBuffer data_enc;
        std::future<void> done;
        bool decoded = false;
        std::ostringstream log;
    };
    wrcli::ContextPool contexts;  // for the segmented fields (declared before the items, whose futures wait for the calls that use it)
    std::vector<Item> items(nf);
    auto report = [](std::exception_ptr e) {
        try { if (e) std::rethrow_exception(e); } catch (const std::exception& x) { cout << "Error: " << x.what() << endl; } catch (...) {}
        cout << "=== decompression failed ===\n";
    };
    // the field sizes are only known record by record; the first record sizes the pipeline
    int depth = -1;
    wrcli::InFlight* gate = nullptr;
    std::unique_ptr<wrcli::InFlight> gate_owner;
    std::thread writer;
    std::exception_ptr writer_error;
    auto tail = [&](Item& im, std::ostream& os) {  // after the decode: what the reference prints about the field
        const size_t ntot = im.h.spec.count();
        double lo, hi;
        if (im.fld32) {
            os << "  decode: fld_1d_rec[0]=" << (double)im.fld32[0] << " fld_1d_rec[last]=" << (double)im.fld32[ntot - 1] << endl;
            wrcli::minmax(im.fld32.get(), ntot, &lo, &hi);
        } else {
            if (im.decoded) os << "  decode: fld_1d_rec[0]=" << im.fld[0] << " fld_1d_rec[last]=" << im.fld[ntot - 1] << endl;
            wrcli::minmax(im.fld.get(), ntot, &lo, &hi);
        }
        os << "        min=" << lo << " max=" << hi << endl;
    };
    auto finish = [&](int it) {
        Item& im = items[it];
        const wrio::FieldSpec& s = im.h.spec;
        const size_t ntot = s.count();
        if (im.done.valid()) im.done.get();
        cout << im.log.str();
        const double t_write = wrcli::PhaseClock::now();
        if (im.fld32) {
            wrio::write_field(out_name, it == 0, file_type, flip != 0, s, im.h.recl, im.fld32.get());
            cout << "  wrote: fld_1d_rec[0]=" << (double)im.fld32[0] << " fld_1d_rec[last]=" << (double)im.fld32[ntot - 1] << endl;
        } else {
            wrio::write_field(out_name, it == 0, file_type, flip != 0, s, im.h.recl, im.fld.get());
            cout << "  wrote: fld_1d_rec[0]=" << im.fld[0] << " fld_1d_rec[last]=" << im.fld[ntot - 1] << endl;
        }
        clock.add(wrcli::PhaseClock::kWrite, t_write);
        im.fld.reset();
        im.fld32.reset();
        im.data_enc.release();
    };
    try {
    for (int it = 0; it < nf; it++) {
        Item& im = items[it];
        wrio::FieldHeader& h = im.h;
        wrio::read_field_header(fheader, it, h);
        const wrio::FieldSpec& s = h.spec;
        if (depth < 0) {
            depth = wrcli::fields_in_flight(s.count(), nf);
            if (depth > 0) {
                setenv("WR_QUIET", "1", 0);
                gate_owner.reset(new wrcli::InFlight(depth));
                gate = gate_owner.get();
                writer = std::thread([&]() {
                    try {
                        for (int k = 0; k < nf; k++) { gate->wait_launched(k); finish(k); gate->leave(); }
                    } catch (...) { writer_error = std::current_exception(); gate->abort(); }
                });
            }
        }
        if (gate && !gate->enter()) break;
        std::ostream& os = depth > 0 ? static_cast<std::ostream&>(im.log) : cout;
        // echo of the header values, gen_aux.cpp:626-643
        os << "  tolabs; midval; halfspanval; wlev; nlay; ntot_enc;";
        if (h.ntot_enc > 0) os << " deps_vec(1:nlay); minval_vec(1:nlay); len_enc_vec(1:nlay)" << endl; else os << endl;
        os << "  " << h.tolabs << " " << h.midval << " " << h.halfspanval << " " << h.wlev << " " << h.nlay << " " << h.ntot_enc << endl;
        if (h.ntot_enc > 0) {
            os << "  "; for (unsigned j = 0; j < h.nlay; j++) os << h.deps_vec[j] << " "; os << endl;
            os << "  "; for (unsigned j = 0; j < h.nlay; j++) os << h.minval_vec[j] << " "; os << endl;
            os << "  "; for (unsigned j = 0; j < h.nlay; j++) os << h.len_enc_vec[j] << " "; os << endl;
        }
        os << "  contains " << s.nbytes << "-byte floating point data" << endl;
        os << "  nx=" << s.nx << "  ny=" << s.ny << "  nz=" << s.nz << "  nh=" << s.nh;
        if (s.idinv) os << " and reordering" << endl; else os << endl;
        const size_t ntot = s.count();
        const double t_read = wrcli::PhaseClock::now();
        if (f32_codec && s.nbytes == 4 && s.icomp && h.ntot_enc > 0) im.fld32.reset(new float[ntot]);
        else im.fld.reset(new double[ntot]);
        if (s.icomp) {
            if (h.ntot_enc > 0) {
                im.data_enc.allocate(h.ntot_enc);
                finput.read(reinterpret_cast<char*>(im.data_enc.data()), (std::streamsize)h.ntot_enc);
                if (finput.fail()) { cout << "Cannot read from " << in_name << endl; throw std::runtime_error("short .wrb"); }
            } else
                for (size_t j = 0; j < ntot; j++) im.fld[j] = h.midval;  // gen_dec.cpp:201: a trivial field is its mid value
        } else {
            wrio::read_raw_field(finput, s.nbytes, im.fld.get(), ntot);
        }
        clock.add(wrcli::PhaseClock::kRead, t_read);
        im.decoded = s.icomp && h.ntot_enc > 0;
        if (im.decoded) os << "  decoding fld_1d_rec, field number " << it << endl;
        Item* ip = &im;
        const bool pipelined = depth > 0;
        auto work = [ip, it, pipelined, &tail, &clock, &contexts]() {
            if (ip->decoded) {
                const double t_codec = wrcli::PhaseClock::now();
                wrio::FieldHeader& hh = ip->h;
                const wrio::FieldSpec& sp = hh.spec;
                unsigned char wlev = (unsigned char)hh.wlev, nlay = (unsigned char)hh.nlay;
                if (wrcli::is_segmented(ip->data_enc.data(), hh.ntot_enc)) {
                    const string who = "field " + std::to_string(it) + ": ";
                    if (!(wr_decode_host_seg && wr_decode_host_seg_f32 && wr_ctx_create && wr_ctx_destroy && wr_last_error))
                        throw std::runtime_error(who + "a segmented stream is " + wrcli::kNotSupported);
                    wr_enc_info info;
                    memset(&info, 0, sizeof info);
                    info.tolabs = hh.tolabs; info.midval = hh.midval; info.halfspanval = hh.halfspanval;
                    info.wlev = wlev; info.nlay = nlay; info.ntot_enc = hh.ntot_enc;
                    for (unsigned l = 0; l < hh.nlay; l++) { info.deps_vec[l] = hh.deps_vec[l]; info.minval_vec[l] = hh.minval_vec[l]; info.len_enc_vec[l] = hh.len_enc_vec[l]; }
                    wr_ctx* c = contexts.borrow();
                    if (!c) throw std::runtime_error(who + wr_last_error());
                    const int rc = ip->fld32 ? wr_decode_host_seg_f32(c, ip->fld32.get(), sp.nx, sp.ny, sp.nz * sp.nh, &info, ip->data_enc.data(), hh.ntot_enc, nullptr)
                                             : wr_decode_host_seg(c, ip->fld.get(), sp.nx, sp.ny, sp.nz * sp.nh, &info, ip->data_enc.data(), hh.ntot_enc, nullptr);
                    const string why = rc ? who + wr_last_error() : string();  // (this thread's message)
                    contexts.give(c);
                    if (rc) throw std::runtime_error(why);
                } else if (ip->fld32)
                    wr_decoding_wrap_f32(sp.nx, sp.ny, sp.nz * sp.nh, ip->fld32.get(), &hh.tolabs, &hh.midval, &hh.halfspanval, &wlev,
                                         &nlay, &hh.ntot_enc, hh.deps_vec, hh.minval_vec, hh.len_enc_vec, ip->data_enc.data());
                else
                    decoding_wrap(sp.nx, sp.ny, sp.nz * sp.nh, ip->fld.get(), &hh.tolabs, &hh.midval, &hh.halfspanval, &wlev, &nlay,
                                  &hh.ntot_enc, hh.deps_vec, hh.minval_vec, hh.len_enc_vec, ip->data_enc.data());
                clock.add(wrcli::PhaseClock::kCodec, t_codec);
            }
            tail(*ip, pipelined ? static_cast<std::ostream&>(ip->log) : cout);
        };
        if (depth > 0) { im.done = std::async(std::launch::async, work); gate->launched(it); }
        else { work(); finish(it); }
    }
    } catch (...) {
        const std::exception_ptr e = std::current_exception();
        if (gate) gate->abort();
        if (writer.joinable()) writer.join();
        report(writer_error ? writer_error : e);
        return 1;
    }
    if (writer.joinable()) writer.join();
    if (writer_error) { report(writer_error); return 1; }
    cout << "=== End of decompression ===\n";
    return 0;
}
