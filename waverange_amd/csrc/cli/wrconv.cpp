// wrconv -- converts a .wrh/.wrb container from one stream format to another, on top of libwaverange_amd.
//
//   wrconv --format=TEXT IN.wrh OUT.wrh OUT.wrb          TEXT: ref | wrs1 | wrs2 | wrs3 [:seg=N] [:brick=B] [:strands=K]
//
// Every coded field goes through wr_transcode_host on a context of the tool's (waverange_amd.h): its planes are decoded by the
// decoder of whatever format the field's bytes say and coded by the target's coder.  No field is reconstructed, no tolerance
// is needed and nothing is quantized again: OUT.wrh / OUT.wrb are what wrenc --format=TEXT writes for the original input, and
// wrdec gives the same bytes from either container.  A file may mix formats field by field; fields stored uncompressed
// (icomp = 0) are copied.  The input .wrb is the one IN.wrh names (as it is named there, else beside IN.wrh; --wrb=PATH
// overrides) and is mapped read-only, not read.
// Options are judged before any output file is created: a bad --format gives exit status 2 and writes nothing.  A field that
// is refused gives "Error: field K: ..." and exit status 1; the output files then end with the field before it.
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../../include/waverange_amd.h"
#include "batch.h"
#include "gen_io.h"
#include "segfmt.h"

extern "C" {
size_t wr_transcode_bound(size_t n, int nlay, int format, unsigned seg, unsigned brick, unsigned strands) __attribute__((weak));
int wr_transcode_host(wr_ctx* ctx, int nx, int ny, int nz, const wr_enc_info* info_in, const unsigned char* data_in, size_t len_in, int format, unsigned seg,
                      unsigned brick, unsigned strands, wr_enc_info* info_out, unsigned char* data_out, size_t cap, wr_timings* tm) __attribute__((weak));
}

using std::cout;
using std::endl;
using std::string;

namespace {

void usage()
{
    cout << "usage: ./wrconv --format=TEXT IN_HEADER_FILE OUT_HEADER_FILE OUT_ENCODED_FILE\n";
    cout << "where TEXT = ref | wrs1 | wrs2 | wrs3 [:seg=N] [:brick=B] [:strands=K]; option: --wrb=IN_ENCODED_FILE (default: the file IN_HEADER_FILE names)\n";
}

// what the six lines in front of the field records say (gen_io.cpp: write_header_preamble)
struct Preamble {
    string wrb_name;
    int file_type = 0, nf = 0;
    bool flip = false;
};

bool read_preamble(std::istream& in, Preamble* p)
{
    string line[6];
    for (string& l : line) if (!std::getline(in, l)) return false;
    const size_t name = line[2].find(": "), type = line[3].rfind(": "), nf = line[5].rfind(": ");
    if (name == string::npos || type == string::npos || nf == string::npos) return false;
    p->wrb_name = line[2].substr(name + 2);
    p->file_type = atoi(line[3].c_str() + type + 2);
    p->flip = line[4].find("No endian conversion") == string::npos;
    p->nf = atoi(line[5].c_str() + nf + 2);
    return p->nf >= 0;
}

}  // namespace

int main(int argc, char** argv)
{
    std::vector<string> options;
    argc = wrcli::take_options(argc, argv, options);
    string format_text, wrb_override;
    bool have_format = false;
    for (const string& o : options) {
        string v;
        if (wrcli::option_value(o, "format", &v)) { format_text = v; have_format = true; }
        else if (wrcli::option_value(o, "wrb", &v) && !v.empty()) wrb_override = v;
        else { usage(); cout << "Error: unknown option " << o << endl; return 2; }
    }
    if (!have_format || argc != 4) { usage(); cout << "Error: --format and three file names are required" << endl; return 2; }
    if (!(wr_transcode_host && wr_transcode_bound && wr_stream_format_parse && wr_ctx_create && wr_ctx_destroy && wr_last_error)) {
        usage();
        cout << "Error: a conversion is " << wrcli::kNotSupported << endl;
        return 2;
    }
    int format = 0;
    unsigned seg = 0, brick = 0, strands = 0;
    if (wr_stream_format_parse(format_text.c_str(), &format, &seg, &brick, &strands) != 0) {
        usage();
        cout << "Error: --format: " << wr_last_error() << endl;
        return 2;
    }
    const string header_in = argv[1], header_out = argv[2], wrb_out = argv[3];
    wrcli::PhaseClock clock("wrconv");

    std::ifstream fheader(header_in);
    if (!fheader.is_open()) { cout << "Cannot open " << header_in << endl; return 1; }
    Preamble pre;
    if (!read_preamble(fheader, &pre)) { cout << "Error: " << header_in << " is not an encoding header file" << endl; return 1; }
    wrcli::MappedFile named, beside;
    wrcli::MappedFile* found = &named;
    string wrb_in = wrb_override.empty() ? pre.wrb_name : wrb_override;
    if (!named.open(wrb_in)) {
        if (!wrb_override.empty()) { cout << "Cannot open " << wrb_in << endl; return 1; }
        // a container that was moved: the .wrb lies beside its header
        const size_t dir = header_in.rfind('/'), base = pre.wrb_name.rfind('/');
        wrb_in = (dir == string::npos ? string() : header_in.substr(0, dir + 1)) + (base == string::npos ? pre.wrb_name : pre.wrb_name.substr(base + 1));
        if (!beside.open(wrb_in)) { cout << "Cannot open " << pre.wrb_name << " (nor " << wrb_in << ")" << endl; return 1; }
        found = &beside;
    }
    const wrcli::MappedFile& wrb = *found;
    // an output that is one of the inputs would be truncated under the mapping
    auto same_file = [](const string& a, const string& b) {
        struct stat sa, sb;
        return stat(a.c_str(), &sa) == 0 && stat(b.c_str(), &sb) == 0 && sa.st_dev == sb.st_dev && sa.st_ino == sb.st_ino;
    };
    if (same_file(wrb_out, wrb_in) || same_file(header_out, header_in) || same_file(wrb_out, header_in) || same_file(header_out, wrb_in)) {
        usage();
        cout << "Error: the output files must not be the input files" << endl;
        return 2;
    }
    cout << "=== Conversion parameters ===" << endl;
    cout << "Input header file name: " << header_in << endl;
    cout << "Input encoded data file name: " << wrb_in << endl;
    cout << "Output header file name: " << header_out << endl;
    cout << "Output encoded data file name: " << wrb_out << endl;
    cout << "Stream format: " << format_text << endl;
    cout << "Number of fields in the file, nf: " << pre.nf << endl;

    wrio::write_header_preamble(header_out, wrb_out, pre.file_type, pre.flip, pre.nf, format != 0);
    { std::ofstream trunc(wrb_out, std::ios::binary | std::ios::out | std::ios::trunc); }

    wrcli::ContextPool contexts;
    wr_ctx* ctx = nullptr;
    int status = 0;
    size_t at = 0;                    // of the field's bytes in the input .wrb
    unsigned long prev_ntot_enc = 0;  // quirk Q2 of the header text, as wrenc keeps it
    for (int it = 0; it < pre.nf && status == 0; it++) {
        wrio::FieldHeader h;
        try { wrio::read_field_header(fheader, it, h); } catch (const std::exception& e) { cout << "Error: field " << it << ": " << e.what() << endl; status = 1; break; }
        const wrio::FieldSpec& s = h.spec;
        const size_t here = at, len = s.icomp ? (size_t)h.ntot_enc : s.count() * (size_t)s.nbytes;
        at += len;
        auto refuse = [&](const string& why) { cout << "Error: field " << it << ": " << why << endl; status = 1; };
        if (here + len > wrb.size()) { refuse(wrb_in + " is shorter than its header says"); break; }
        if (!s.icomp) {  // stored as it was read: copied
            const double t_write = wrcli::PhaseClock::now();
            wrio::append_field_header(header_out, it, h, prev_ntot_enc);
            if (len) wrio::append_bytes(wrb_out, wrb.data() + here, len);
            clock.add(wrcli::PhaseClock::kWrite, t_write);
            cout << "  field " << it << ": stored uncompressed, copied" << endl;
            continue;
        }
        wr_enc_info info, out;
        memset(&info, 0, sizeof info);
        info.tolabs = h.tolabs; info.midval = h.midval; info.halfspanval = h.halfspanval;
        info.wlev = (unsigned char)h.wlev; info.nlay = (unsigned char)h.nlay; info.ntot_enc = h.ntot_enc;
        for (unsigned l = 0; l < h.nlay; l++) { info.deps_vec[l] = h.deps_vec[l]; info.minval_vec[l] = h.minval_vec[l]; info.len_enc_vec[l] = h.len_enc_vec[l]; }
        const int nx = s.nx, ny = s.ny, nz = s.nz * s.nh;  // nh > 1 folds into z, as it was coded
        const size_t cap = len ? wr_transcode_bound(s.count(), (int)h.nlay, format, seg, brick, strands) : 0;
        if (len && !cap) { refuse("nlay out of range"); break; }
        wrcli::RawBuffer data;  // the target's worst case, untouched beyond the coded bytes
        data.allocate(cap);
        if (!ctx && !(ctx = contexts.borrow())) { cout << "Error: " << wr_last_error() << endl; return 1; }
        static const unsigned char kNoBytes[4] = {0, 0, 0, 0};
        const double t_codec = wrcli::PhaseClock::now();
        const int rc = wr_transcode_host(ctx, nx, ny, nz, &info, len ? wrb.data() + here : kNoBytes, len, format, seg, brick, strands, &out, data.data(), cap, nullptr);
        clock.add(wrcli::PhaseClock::kCodec, t_codec);
        if (rc != 0) { refuse(wr_last_error()); break; }
        const int from = len ? wr_stream_sniff(wrb.data() + here, len) : -1;
        static const char* const names[4] = {"ref", "wrs1", "wrs2", "wrs3"};
        cout << "  field " << it << ": " << (from >= 0 ? names[from] : "constant") << " -> " << names[format] << ", " << h.ntot_enc << " -> " << out.ntot_enc << " bytes" << endl;
        h.ntot_enc = out.ntot_enc;
        for (unsigned l = 0; l < h.nlay; l++) h.len_enc_vec[l] = out.len_enc_vec[l];
        const double t_write = wrcli::PhaseClock::now();
        wrio::append_field_header(header_out, it, h, h.ntot_enc);
        if (h.ntot_enc > 0) wrio::append_bytes(wrb_out, data.data(), h.ntot_enc);
        prev_ntot_enc = h.ntot_enc;
        clock.add(wrcli::PhaseClock::kWrite, t_write);
    }
    if (ctx) contexts.give(ctx);
    cout << (status ? "=== conversion failed ===\n" : "=== End of conversion ===\n");
    return status;
}
