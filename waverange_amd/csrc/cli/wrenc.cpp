// wrenc -- generic encoder command-line tool on top of libwaverange_amd.
//
// Same command line, `inmeta` control file (new key=value and old line formats), interactive
// prompts and .wrh/.wrb output as the reference's generic encoder (src/generic/gen_enc.cpp):
//   wrenc INPUT_FILE ENCODED_FILE HEADER_FILE TYPE ENDIANFLIP NF PRECISION NX NY NZ TOLERANCE
// Parameter sources in the reference's priority order (gen_enc.cpp:112-486): a file named
// `inmeta` in the working directory, then 11 arguments, then interactive prompts.
// Arguments that start with "--" are options of this tool and are taken out before any of that:
//   --format=ref|wrs1|wrs2|wrs3[:seg=N][:brick=B][:strands=K]   the stream format of the coded fields (waverange_amd.h,
//       wr_stream_format_parse); without it the library's setting decides (WR_STREAM_FORMAT, else the reference's stream)
//   --maxerr=E  encode every compressed field to a pointwise error bound (wr_encode_host_seg_bounded): E is absolute, in the
//               field's units; TOLERANCE is the finest tolerance allowed; needs --format=wrs1, wrs2 or wrs3, excludes --ratio
//   --rmse=E    encode every compressed field to an RMS error target (wr_encode_host_seg_quality, WR_NORM_RMS): E is absolute, in
//               the field's units.  --psnr=DB: to a PSNR target in dB over the field's range (WR_NORM_PSNR).  TOLERANCE, the
//               formats and the exclusions are those of --maxerr; --rmse, --psnr, --maxerr and --ratio exclude one another
//   --ratio=R   encode every compressed field to a byte budget (wr_encode_host_seg_budget): the field's bytes on disk divided
//       by R.  TOLERANCE is then the finest tolerance the search may choose; the tool prints the one it chose.  Needs
//       --format=wrs1.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <future>
#include <thread>
#include <iostream>
#include <memory>
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

struct Job {
    string in_name = "data.bin", out_name = "data.wrb", header_name = "data.wrh";
    int file_type = 0, flip = 0, nf = 1;
    std::vector<wrio::FieldSpec> fields;
    // the value the reference leaves in its scalar `tol_base` when parsing ends; it alone
    // feeds cutoffvec[0] for EVERY field (quirk Q1, gen_enc.cpp:499-503)
    double effective_tol = 1e-16;
};

string trim(const string& s)
{
    const char* ws = " \t\v\r\n";
    size_t a = s.find_first_not_of(ws);
    if (a == string::npos) return "";
    return s.substr(a, s.find_last_not_of(ws) - a + 1);
}

string lower(string s) { std::transform(s.begin(), s.end(), s.begin(), ::tolower); return s; }

template <class T> void parse_into(const string& s, T& v) { if (!s.empty()) std::stringstream(s) >> v; }

// "key = value" with exactly one '='; returns false otherwise
bool key_value(const string& line, string& key, string& val, bool& malformed)
{
    size_t n = std::count(line.begin(), line.end(), '=');
    malformed = n != 1;
    if (malformed) return false;
    size_t p = line.find('=');
    key = lower(trim(line.substr(0, p)));
    val = trim(line.substr(p + 1));
    if (val.empty()) { malformed = true; return false; }
    return true;
}

// running per-field defaults: a field inherits whatever the previous one set (gen_enc.cpp:61-101)
struct Running {
    int intype = 2;
    wrio::FieldSpec s;
    void set(const string k[8])
    {
        parse_into(k[0], intype); parse_into(k[1], s.nx); parse_into(k[2], s.ny); parse_into(k[3], s.nz);
        parse_into(k[4], s.nh); parse_into(k[5], s.idinv); parse_into(k[6], s.icomp); parse_into(k[7], s.tol_base);
        s.nbytes = intype == 1 ? 4 : 8;
    }
};

void echo_field(const string k[8])
{
    static const char* names[8] = {"input_data_type", "nx", "ny", "nz", "nh", "order", "compress", "tolerance"};
    for (int i = 0; i < 8; i++) cout << names[i] << " = " << k[i] << endl;
    cout << "" << endl;
}

void echo_common(const Job& j, const string& ft, const string& ec, const string& nf)
{
    cout << "in_name = " << j.in_name << endl << "out_name = " << j.out_name << endl;
    cout << "header_name = " << j.header_name << endl << "file_type = " << ft << endl;
    cout << "endian_conversion = " << ec << endl << "number_of_field = " << nf << endl << "" << endl;
}

// `inmeta`, new format: "&key = value" lines, "%field = k" blocks closed by "/"  (gen_enc.cpp:119-279)
// returns 1 parsed, 0 not this format, -1 error
int parse_inmeta_new(const std::vector<string>& lines, Job& job)
{
    string ft, ec, nf;
    bool any = false;
    for (const string& raw : lines) {
        string l = trim(raw);
        if (l.empty() || l[0] != '&') continue;
        string k, v; bool bad;
        if (!key_value(l, k, v, bad)) {
            if (std::count(l.begin(), l.end(), '=') > 1) cout << "==== Error : '=' exists twice in a sentence :" << l << " ====" << endl;
            else cout << "==== Error : 'value' is missing in a sentence :" << l << " ====" << endl;
            return -1;
        }
        any = true;
        if (k == "&in_name") job.in_name = v;
        if (k == "&out_name") job.out_name = v;
        if (k == "&header_name") job.header_name = v;
        if (k == "&file_type") ft = v;
        if (k == "&endian_conversion") ec = v;
        if (k == "&number_of_field") nf = v;
    }
    if (!any) return 0;
    echo_common(job, ft, ec, nf);
    parse_into(ft, job.file_type); parse_into(ec, job.flip); parse_into(nf, job.nf);
    job.fields.assign(job.nf, wrio::FieldSpec());
    Running run;
    string k8[8];
    int blocks = 0, field_id = -1;
    for (const string& raw : lines) {
        string l = trim(raw);
        if (l.empty()) continue;
        string k, v; bool bad;
        if (l[0] == '%' && key_value(l, k, v, bad) && k == "%field") {
            std::stringstream(v) >> field_id;
            cout << "==== read parameters for field " << field_id << " ====" << endl;
            blocks++;
        }
        if (l[0] == '&' && key_value(l, k, v, bad)) {
            static const char* keys[8] = {"&input_data_type", "&nx", "&ny", "&nz", "&nh", "&order", "&compress", "&tolerance"};
            for (int i = 0; i < 8; i++) if (k == keys[i]) k8[i] = v;
        }
        if (l[0] == '/') {
            echo_field(k8);
            run.set(k8);
            if (field_id >= 0 && field_id < job.nf) job.fields[field_id] = run.s;
        }
    }
    if (blocks != job.nf) {
        cout << "==== Number of fields is " << job.nf << " ====" << endl;
        cout << "==== Number of blocks for field parameters are not sufficient. ====" << endl;
        cout << "==== Numbef of block = " << blocks << " ====" << endl;
        return -1;
    }
    job.effective_tol = run.s.tol_base;
    return 1;
}

// `inmeta`, old format: one value per line in prompt order (gen_enc.cpp:282-349)
void parse_inmeta_old(const std::vector<string>& lines, Job& job)
{
    cout << "==== read parameters from inmeta as old format. ====" << endl;
    size_t p = 0;
    auto next = [&]() { return p < lines.size() ? lines[p++] : string(); };
    job.in_name = next(); job.out_name = next(); job.header_name = next();
    string ft = next(), ec = next(), nf = next();
    echo_common(job, ft, ec, nf);
    if (job.in_name.empty()) job.in_name = "data.bin";
    if (job.out_name.empty()) job.out_name = "data.wrb";
    if (job.header_name.empty()) job.header_name = "data.wrh";
    parse_into(ft, job.file_type); parse_into(ec, job.flip); parse_into(nf, job.nf);
    Running run;
    for (int it = 0; it < job.nf; it++) {
        string k8[8];
        for (auto& s : k8) s = next();
        echo_field(k8);
        run.set(k8);
        job.fields.push_back(run.s);
    }
    job.effective_tol = run.s.tol_base;
}

void usage()
{
    cout << "usage: ./wrenc INPUT_FILE ENCODED_FILE HEADER_FILE TYPE ENDIANFLIP NF PRECISION NX NY NZ TOLERANCE\n";
    cout << "where TYPE=(0: Fortran sequential w 4-byte recl; 1: Fortran sequential w 8-byte recl; 2: C/C++),\n";
    cout << "      ENDIANFLIP=(0:no; 1:yes), NF=(how many fields, e.g. 1), PRECISION=(1:single; 2:double),\n";
    cout << "      NX=(e.g. 16), NY=(e.g. 16), NZ=(e.g. 16) and TOLERANCE=(e.g. 1.0e-16)\n";
    cout << "interactive mode if not enough arguments are passed.\n";
    cout << "option: --format=ref|wrs1|wrs2|wrs3[:seg=N][:brick=B][:strands=K] (stream format of the coded fields; default: WR_STREAM_FORMAT, else ref)\n";
    cout << "option: --ratio=R (with --format=wrs1: every field coded into its bytes on disk / R, at the finest tolerance not below TOLERANCE that fits)\n";
    cout << "option: --rmse=E | --psnr=DB (with --format=wrs1|wrs2|wrs3: every field coded at the coarsest tolerance not below TOLERANCE whose RMS error stays within E, in the field's units, or whose PSNR over the field's range reaches DB)\n";
    cout << "option: --maxerr=E (with --format=wrs1|wrs2|wrs3: every field coded at the coarsest tolerance not below TOLERANCE that keeps every sample within E, in the field's units)\n";
}

void parse_argv(char** argv, Job& job)  // gen_enc.cpp:365-412
{
    cout << "automatic mode.";
    job.in_name = argv[1]; job.out_name = argv[2]; job.header_name = argv[3];
    Running run;
    parse_into(string(argv[4]), job.file_type); parse_into(string(argv[5]), job.flip);
    parse_into(string(argv[6]), job.nf); parse_into(string(argv[7]), run.intype);
    parse_into(string(argv[8]), run.s.nx); parse_into(string(argv[9]), run.s.ny);
    parse_into(string(argv[10]), run.s.nz); parse_into(string(argv[11]), run.s.tol_base);
    run.s.nbytes = run.intype == 1 ? 4 : 8;
    job.fields.assign(job.nf > 0 ? job.nf : 0, run.s);
    job.effective_tol = run.s.tol_base;
}

void parse_interactive(Job& job)  // gen_enc.cpp:413-486
{
    auto ask = [](const char* prompt) { cout << prompt; string s; std::getline(std::cin, s); return s; };
    string s;
    s = ask("Enter input data file name [data.bin]: "); if (!s.empty()) job.in_name = s;
    s = ask("Enter encoded data file name [data.wrb]: "); if (!s.empty()) job.out_name = s;
    s = ask("Enter encoding header file name [data.wrh]: "); if (!s.empty()) job.header_name = s;
    parse_into(ask("Enter file type (0: Fortran sequential w 4-byte recl; 1: Fortran sequential w 8-byte recl; 2: C/C++) [0]: "), job.file_type);
    parse_into(ask("Enter endian conversion (0: do not perform; 1: inversion) [0]: "), job.flip);
    parse_into(ask("Enter the number of fields in the file, nf [1]: "), job.nf);
    Running run;
    for (int it = 0; it < job.nf; it++) {
        cout << "Field number " << it << endl;
        parse_into(ask("Enter input data type (1: float; 2: double) [2]: "), run.intype);
        run.s.nbytes = run.intype == 1 ? 4 : 8;
        parse_into(ask("Enter the number of data points in the first dimension, nx [16]: "), run.s.nx);
        parse_into(ask("Enter the number of data points in the second dimension, ny [16]: "), run.s.ny);
        parse_into(ask("Enter the number of data points in the third dimension, nz [16]: "), run.s.nz);
        parse_into(ask("Enter the number of data points in the higher (slowest) dimensions, nh [1]: "), run.s.nh);
        parse_into(ask("Invert the order of the dimensions? (0: no; 1: yes) [0]: "), run.s.idinv);
        parse_into(ask("Enter compression flag (0: do not compress; 1: compress) [1]: "), run.s.icomp);
        wrio::FieldSpec f = run.s;
        if (run.s.icomp) { parse_into(ask("Enter base cutoff relative tolerance [1e-16]: "), run.s.tol_base); f.tol_base = run.s.tol_base; }
        else f.tol_base = 0;
        job.fields.push_back(f);
    }
    job.effective_tol = run.s.tol_base;
}

}  // namespace

int main(int argc, char** argv)
{
    // options first: nothing is read, created or truncated before they are known to be good
    std::vector<string> options;
    argc = wrcli::take_options(argc, argv, options);
    string format_text;
    bool have_format = false;
    string ratio_text;
    double ratio = 0;
    string maxerr_text;
    double maxerr = 0;
    string quality_text;
    const char* quality_opt = nullptr;  // "rmse" or "psnr" once one of them is given
    int quality_norm = 0;
    double quality = 0;
    for (const string& o : options) {
        if (wrcli::option_value(o, "format", &format_text)) { have_format = true; continue; }
        if (wrcli::option_value(o, "ratio", &ratio_text)) {
            char* end = nullptr;
            ratio = strtod(ratio_text.c_str(), &end);
            if (ratio_text.empty() || *end || !(ratio >= 1.0) || !(ratio < 1e12)) {
                usage();
                cout << "Error: --ratio=" << ratio_text << ": a number of at least 1 is required" << endl;
                return 2;
            }
            continue;
        }
        if (wrcli::option_value(o, "maxerr", &maxerr_text)) {
            char* end = nullptr;
            maxerr = strtod(maxerr_text.c_str(), &end);
            if (maxerr_text.empty() || *end || !(maxerr > 0) || !(maxerr < 1e308)) {
                usage();
                cout << "Error: --maxerr=" << maxerr_text << ": a positive number is required" << endl;
                return 2;
            }
            continue;
        }
        {
            const bool rmse = wrcli::option_value(o, "rmse", &quality_text);
            if (rmse || wrcli::option_value(o, "psnr", &quality_text)) {
                const char* name = rmse ? "rmse" : "psnr";
                if (quality_opt && strcmp(quality_opt, name)) {
                    usage();
                    cout << "Error: --rmse and --psnr exclude one another" << endl;
                    return 2;
                }
                char* end = nullptr;
                quality = strtod(quality_text.c_str(), &end);
                if (quality_text.empty() || *end || !(quality > 0) || !(quality < 1e308)) {
                    usage();
                    cout << "Error: --" << name << "=" << quality_text << ": a positive number is required" << endl;
                    return 2;
                }
                quality_opt = name;
                quality_norm = rmse ? WR_NORM_RMS : WR_NORM_PSNR;
                continue;
            }
        }
        usage();
        cout << "Error: unknown option " << o << endl;
        return 2;
    }
    int stream_format = 0;
    {
        string why;
        if (!wrcli::choose_stream_format(have_format ? &format_text : nullptr, &stream_format, &why)) {
            usage();
            cout << "Error: " << why << endl;
            return 2;
        }
    }
    unsigned budget_seg = 0;
    if (ratio > 0) {
        if (stream_format != WR_FORMAT_WRS1) {
            usage();
            cout << "Error: --ratio needs --format=wrs1" << endl;
            return 2;
        }
        if (!wr_encode_host_seg_budget || !wr_encode_host_seg_budget_f32 || !wr_get_stream_format || !wr_ctx_create) {
            usage();
            cout << "Error: --ratio: " << wrcli::kNotSupported << endl;
            return 2;
        }
        wr_get_stream_format(nullptr, &budget_seg, nullptr, nullptr);
    }
    unsigned bounded_fmt[3] = {0, 0, 0};  // --maxerr, --rmse, --psnr: seg, brick, strands of the bounded / quality calls
    if (quality_opt) {
        if (maxerr > 0 || ratio > 0) {
            usage();
            cout << "Error: --" << quality_opt << " and --" << (maxerr > 0 ? "maxerr" : "ratio") << " exclude one another" << endl;
            return 2;
        }
        if (stream_format != WR_FORMAT_WRS1 && stream_format != WR_FORMAT_WRS2 && stream_format != WR_FORMAT_WRS3) {
            usage();
            cout << "Error: --" << quality_opt << " needs --format=wrs1, wrs2 or wrs3" << endl;
            return 2;
        }
        if (!wr_encode_host_seg_quality || !wr_encode_host_seg_quality_f32 || !wr_get_stream_format || !wr_ctx_create) {
            usage();
            cout << "Error: --" << quality_opt << ": " << wrcli::kNotSupported << endl;
            return 2;
        }
    }
    if (maxerr > 0) {
        if (ratio > 0) {
            usage();
            cout << "Error: --maxerr and --ratio exclude one another" << endl;
            return 2;
        }
        if (stream_format != WR_FORMAT_WRS1 && stream_format != WR_FORMAT_WRS2 && stream_format != WR_FORMAT_WRS3) {
            usage();
            cout << "Error: --maxerr needs --format=wrs1, wrs2 or wrs3" << endl;
            return 2;
        }
        if (!wr_encode_host_seg_bounded || !wr_encode_host_seg_bounded_f32 || !wr_get_stream_format || !wr_ctx_create) {
            usage();
            cout << "Error: --maxerr: " << wrcli::kNotSupported << endl;
            return 2;
        }
    }
    if (maxerr > 0 || quality_opt) {
        wr_get_stream_format(nullptr, &bounded_fmt[0], &bounded_fmt[1], &bounded_fmt[2]);
        if (stream_format == WR_FORMAT_WRS1) bounded_fmt[1] = bounded_fmt[2] = 0;
        if (stream_format == WR_FORMAT_WRS2) { bounded_fmt[2] = 0; if (!bounded_fmt[1]) bounded_fmt[1] = WR_BRICK_DEFAULT; }
        if (stream_format == WR_FORMAT_WRS3 && !bounded_fmt[2]) bounded_fmt[2] = WR_STRANDS_DEFAULT;
    }
    const unsigned bseg = bounded_fmt[0], bbrick = bounded_fmt[1], bstrands = bounded_fmt[2];
    wrcli::ContextPool contexts;  // --ratio, --maxerr, --rmse, --psnr: one explicit context per field in flight
    wrcli::PhaseClock clock("wrenc");

    Job job;
    std::ifstream meta("inmeta");
    if (!meta.fail()) {
        cout << "==== inmeta exists. ====" << endl;
        std::vector<string> lines;
        for (string l; std::getline(meta, l);) lines.push_back(l);
        int rc = parse_inmeta_new(lines, job);
        if (rc < 0) return -1;
        if (rc == 0) parse_inmeta_old(lines, job);
    } else {
        cout << "==== inmeta doesn't exists. ====" << endl;
        usage();
        if (argc == 12) parse_argv(argv, job); else parse_interactive(job);
    }

    cout << endl << "=== Compression parameters ===" << endl;
    cout << "Input data file name: " << job.in_name << endl;
    cout << "Encoded data file name: " << job.out_name << endl;
    cout << "Encoding header file name: " << job.header_name << endl;
    cout << "File type (0: Fortran sequential w 4-byte recl; 1: Fortran sequential w 8-byte recl; 2: C/C++): " << job.file_type << endl;
    if (job.flip) cout << "Convert big endian to little endian or vice versa" << endl;
    cout << "Number of fields in the file, nf: " << job.nf << endl;

    // (a segmented file says so in the first line of its header, which every reader skips: for the person who feeds it to
    // the reference's wrdec)
    wrio::write_header_preamble(job.header_name, job.out_name, job.file_type, job.flip != 0, job.nf, stream_format != 0);
    { std::ofstream trunc(job.out_name, std::ios::binary | std::ios::out | std::ios::trunc); }
    if (job.file_type < 0 || job.file_type > 2) { cout << "Error: unknown file type" << endl; return 0; }

    // Field pipeline.  The reference codes one field after the other (gen_enc.cpp:538-605); here up to `depth` fields
    // are in flight: the main thread reads field k from the input file and hands it to a worker thread (min/max for the
    // log, encoding_wrap: upload, GPU kernels, host range coder), a writer thread appends the header records and coded
    // bytes of finished fields in field order.  With more than one field the library's coder pool codes the plane
    // streams of all fields in flight on one worker per CPU, and says how many fields fit (wr_autotune_batch;
    // WR_CLI_PIPELINE overrides; 0 = strictly one after the other with the reference's order of log lines).
    size_t max_elems = 0;
    for (const wrio::FieldSpec& s : job.fields) max_elems = std::max(max_elems, s.count());
    int depth = wrcli::fields_in_flight(max_elems, job.nf);
    if (depth > 0) setenv("WR_QUIET", "1", 0);  // the library's progress lines of concurrent fields would interleave
    setenv("WR_WRITEBACK_RESIDUAL", "0", 0);    // the residual encoding_wrap leaves in the field array is not used here

    // fp32 records that are compressed go to the codec as fp32 (batch.h): read with no conversion, coded by wr_encoding_wrap_f32
    const char* widen_env = getenv("WR_CLI_WIDEN_ON_HOST");
    const bool f32_codec = wr_encoding_wrap_f32 != nullptr && !(widen_env && atoi(widen_env));
    const double cutoff = job.effective_tol;  // quirk Q1: one cutoff for all fields
    long pos = 0;
    unsigned long prev_ntot_enc = 0;  // quirk Q2: stale value reused for uncompressed fields
    struct Item {
        wrio::FieldHeader h;
        std::vector<double> fld;
        std::unique_ptr<float[]> fld32;  // instead of fld: an fp32 record for wr_encoding_wrap_f32 (not zero-filled)
        wrcli::RawBuffer data_enc;   // setup_wr's worst case, untouched beyond the coded bytes
        size_t cap = 0;              // its size
        std::future<void> done;
        std::ostringstream log;      // this field's lines, printed when it is written (pipelined mode)
    };
    std::vector<Item> items(job.nf);
    auto scan = [](const Item& im, std::ostream& os) {
        const size_t ntot = im.h.spec.count();
        double lo, hi;
        if (im.fld32) {
            os << "  read: fld_1d[0]=" << (double)im.fld32[0] << " fld_1d[last]=" << (double)im.fld32[ntot - 1] << endl;
            wrcli::minmax(im.fld32.get(), ntot, &lo, &hi);
        } else {
            os << "  read: fld_1d[0]=" << im.fld[0] << " fld_1d[last]=" << im.fld[ntot - 1] << endl;
            wrcli::minmax(im.fld.data(), ntot, &lo, &hi);
        }
        os << "        min=" << lo << " max=" << hi << endl;
    };
    auto finish = [&](int it) {  // in field order: wait for the codec, then append to .wrh / .wrb
        Item& im = items[it];
        const wrio::FieldSpec& s = im.h.spec;
        if (im.done.valid()) im.done.get();
        cout << im.log.str();
        const double t_write = wrcli::PhaseClock::now();
        if (s.icomp) {
            cout << "        tolabs=" << im.h.tolabs << endl;
            wrio::append_field_header(job.header_name, it, im.h, im.h.ntot_enc);
            if (im.h.ntot_enc > 0) wrio::append_bytes(job.out_name, im.data_enc.data(), im.h.ntot_enc);
            prev_ntot_enc = im.h.ntot_enc;
        } else {
            wrio::append_field_header(job.header_name, it, im.h, prev_ntot_enc);
            wrio::append_raw_field(job.out_name, s.nbytes, im.fld.data(), s.count());
        }
        clock.add(wrcli::PhaseClock::kWrite, t_write);
        std::vector<double>().swap(im.fld);
        im.fld32.reset();
        im.data_enc.release();
    };
    wrcli::InFlight gate(depth);      // fields between "read" and "written"
    std::thread writer;
    std::exception_ptr writer_error;
    if (depth > 0)
        writer = std::thread([&]() {
            try {
                for (int it = 0; it < job.nf; it++) { gate.wait_launched(it); finish(it); gate.leave(); }
            } catch (...) { writer_error = std::current_exception(); gate.abort(); }
        });
    unsigned char recl[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    try {
    for (int it = 0; it < job.nf; it++) {
        if (depth > 0 && !gate.enter()) break;  // waits while `depth` fields are in flight
        Item& im = items[it];
        const wrio::FieldSpec& s = job.fields[it];
        std::ostream& os = depth > 0 ? static_cast<std::ostream&>(im.log) : cout;
        os << "Field number " << it << endl;
        os << "  contains " << s.nbytes << "-byte floating point data" << endl;
        os << "  nx=" << s.nx << "  ny=" << s.ny << "  nz=" << s.nz << "  nh=" << s.nh;
        if (s.idinv) os << " and reordering" << endl; else os << endl;
        const double t_read = wrcli::PhaseClock::now();
        if (f32_codec && s.nbytes == 4 && s.icomp) {
            im.fld32.reset(new float[s.count()]);
            wrio::read_field(job.in_name, job.file_type, job.flip != 0, s, recl, &pos, im.fld32.get());
        } else {
            wrio::read_field(job.in_name, job.file_type, job.flip != 0, s, recl, &pos, im.fld);
        }
        clock.add(wrcli::PhaseClock::kRead, t_read);
        if (depth == 0) scan(im, cout);

        im.h.spec = s;
        for (int j = 0; j < 8; j++) im.h.recl[j] = recl[j];
        if (s.icomp) {
            unsigned char nlaymax; unsigned long cap;
            setup_wr(s.nx, s.ny, s.nz * s.nh, &nlaymax, &cap);
            im.data_enc.allocate(cap);
            im.cap = cap;
        }
        Item* ip = &im;
        const bool pipelined = depth > 0;
        auto work = [ip, cutoff, pipelined, ratio, budget_seg, maxerr, quality_opt, quality_norm, quality, bseg, bbrick, bstrands, &contexts, &scan, &clock]() {
            const wrio::FieldSpec& sp = ip->h.spec;
            if (pipelined) scan(*ip, ip->log);
            if (!sp.icomp) { (pipelined ? static_cast<std::ostream&>(ip->log) : cout) << "  Compression disabled" << endl; return; }
            (pipelined ? static_cast<std::ostream&>(ip->log) : cout) << "  Compression enabled with base relative tolerance " << sp.tol_base << endl;
            unsigned char wlev = 0, nlay = 0;
            double cut = cutoff;
            const double t_codec = wrcli::PhaseClock::now();
            // nh > 1 folds into z (gen_enc.cpp:559,596)
            if (ratio > 0) {  // to a byte budget: the field's bytes on disk / R, no tolerance finer than the command line's
                const size_t budget = (size_t)((double)(sp.count() * (size_t)sp.nbytes) / ratio);
                wr_ctx* ctx = contexts.borrow();
                wr_enc_info info;
                wr_budget_result res;
                int rc = ctx ? 0 : -1;
                if (ctx)
                    rc = ip->fld32 ? wr_encode_host_seg_budget_f32(ctx, ip->fld32.get(), sp.nx, sp.ny, sp.nz * sp.nh, 1, 1, 1, 1, budget, cut, budget_seg,
                                                                   &info, ip->data_enc.data(), ip->cap, nullptr, &res)
                                   : wr_encode_host_seg_budget(ctx, ip->fld.data(), sp.nx, sp.ny, sp.nz * sp.nh, 1, 1, 1, 1, budget, cut, budget_seg, &info,
                                                               ip->data_enc.data(), ip->cap, nullptr, &res);
                if (ctx) contexts.give(ctx);
                if (rc != 0) {  // (as the codec's own failures: the tool ends here, whatever other fields are in flight)
                    cout.flush();
                    fprintf(stderr, "Error: field with a budget of %zu bytes: %s\n", budget, wr_last_error());
                    std::_Exit(1);
                }
                char line[200];
                snprintf(line, sizeof line, "  Budget %zu bytes: relative tolerance %.17g (grid point %d), bound %zu bytes, coded %lu bytes\n", budget, res.tolrel,
                         res.g, res.bound, info.ntot_enc);
                (pipelined ? static_cast<std::ostream&>(ip->log) : cout) << line;
                ip->h.tolabs = info.tolabs; ip->h.midval = info.midval; ip->h.halfspanval = info.halfspanval;
                wlev = info.wlev; nlay = info.nlay;
                ip->h.ntot_enc = info.ntot_enc;
                for (int l = 0; l < WR_NLAYMAX; l++) {
                    ip->h.deps_vec[l] = info.deps_vec[l]; ip->h.minval_vec[l] = info.minval_vec[l]; ip->h.len_enc_vec[l] = info.len_enc_vec[l];
                }
            } else if (maxerr > 0) {  // to an error bound: no sample further than E from its reconstruction, no tolerance finer than the command line's
                wr_ctx* ctx = contexts.borrow();
                wr_enc_info info;
                wr_bounded_result res;
                int rc = ctx ? 0 : -1;
                if (ctx)
                    rc = ip->fld32 ? wr_encode_host_seg_bounded_f32(ctx, ip->fld32.get(), sp.nx, sp.ny, sp.nz * sp.nh, 1, 1, 1, 1, maxerr, cut, bseg, bbrick,
                                                                    bstrands, &info, ip->data_enc.data(), ip->cap, nullptr, &res)
                                   : wr_encode_host_seg_bounded(ctx, ip->fld.data(), sp.nx, sp.ny, sp.nz * sp.nh, 1, 1, 1, 1, maxerr, cut, bseg, bbrick, bstrands,
                                                                &info, ip->data_enc.data(), ip->cap, nullptr, &res);
                if (ctx) contexts.give(ctx);
                if (rc != 0) {  // (as the codec's own failures: the tool ends here, whatever other fields are in flight)
                    cout.flush();
                    fprintf(stderr, "Error: field with an error bound of %.17g: %s\n", maxerr, wr_last_error());
                    std::_Exit(1);
                }
                char line[240];
                snprintf(line, sizeof line, "  Error bound %.17g: relative tolerance %.17g (grid point %d), error %.17g, %d trials, coded %lu bytes\n", maxerr,
                         res.tolrel, res.g, res.err, res.trials, info.ntot_enc);
                (pipelined ? static_cast<std::ostream&>(ip->log) : cout) << line;
                ip->h.tolabs = info.tolabs; ip->h.midval = info.midval; ip->h.halfspanval = info.halfspanval;
                wlev = info.wlev; nlay = info.nlay;
                ip->h.ntot_enc = info.ntot_enc;
                for (int l = 0; l < WR_NLAYMAX; l++) {
                    ip->h.deps_vec[l] = info.deps_vec[l]; ip->h.minval_vec[l] = info.minval_vec[l]; ip->h.len_enc_vec[l] = info.len_enc_vec[l];
                }
            } else if (quality_opt) {  // to an RMS error or PSNR target, no tolerance finer than the command line's
                wr_ctx* ctx = contexts.borrow();
                wr_enc_info info;
                wr_quality_result res;
                int rc = ctx ? 0 : -1;
                if (ctx)
                    rc = ip->fld32 ? wr_encode_host_seg_quality_f32(ctx, ip->fld32.get(), sp.nx, sp.ny, sp.nz * sp.nh, 1, 1, 1, 1, quality_norm, quality, cut,
                                                                    bseg, bbrick, bstrands, &info, ip->data_enc.data(), ip->cap, nullptr, &res)
                                   : wr_encode_host_seg_quality(ctx, ip->fld.data(), sp.nx, sp.ny, sp.nz * sp.nh, 1, 1, 1, 1, quality_norm, quality, cut, bseg,
                                                                bbrick, bstrands, &info, ip->data_enc.data(), ip->cap, nullptr, &res);
                if (ctx) contexts.give(ctx);
                if (rc != 0) {  // (as the codec's own failures: the tool ends here, whatever other fields are in flight)
                    cout.flush();
                    fprintf(stderr, "Error: field with a %s target of %.17g: %s\n", quality_norm == WR_NORM_RMS ? "RMS error" : "PSNR", quality, wr_last_error());
                    std::_Exit(1);
                }
                char line[400];
                snprintf(line, sizeof line,
                         "  %s target %.17g: relative tolerance %.17g (grid point %d), rms %.17g (allowed %.17g), psnr %.17g dB, max error %.17g, %d trials, coded %lu bytes\n",
                         quality_norm == WR_NORM_RMS ? "RMS error" : "PSNR", quality, res.tolrel, res.g, res.rms, res.max_rms, res.psnr, res.max_abs, res.trials,
                         info.ntot_enc);
                (pipelined ? static_cast<std::ostream&>(ip->log) : cout) << line;
                ip->h.tolabs = info.tolabs; ip->h.midval = info.midval; ip->h.halfspanval = info.halfspanval;
                wlev = info.wlev; nlay = info.nlay;
                ip->h.ntot_enc = info.ntot_enc;
                for (int l = 0; l < WR_NLAYMAX; l++) {
                    ip->h.deps_vec[l] = info.deps_vec[l]; ip->h.minval_vec[l] = info.minval_vec[l]; ip->h.len_enc_vec[l] = info.len_enc_vec[l];
                }
            } else if (ip->fld32)
                wr_encoding_wrap_f32(sp.nx, sp.ny, sp.nz * sp.nh, ip->fld32.get(), 1, 1, 1, 1, &cut, &ip->h.tolabs, &ip->h.midval,
                                     &ip->h.halfspanval, &wlev, &nlay, &ip->h.ntot_enc, ip->h.deps_vec, ip->h.minval_vec,
                                     ip->h.len_enc_vec, ip->data_enc.data());
            else
                encoding_wrap(sp.nx, sp.ny, sp.nz * sp.nh, ip->fld.data(), 1, 1, 1, 1, &cut, &ip->h.tolabs, &ip->h.midval,
                              &ip->h.halfspanval, &wlev, &nlay, &ip->h.ntot_enc, ip->h.deps_vec, ip->h.minval_vec,
                              ip->h.len_enc_vec, ip->data_enc.data());
            clock.add(wrcli::PhaseClock::kCodec, t_codec);
            ip->h.wlev = wlev; ip->h.nlay = nlay;
        };
        if (depth > 0) { im.done = std::async(std::launch::async, work); gate.launched(it); }
        else { work(); finish(it); }
    }
    } catch (...) {
        gate.abort();
        if (writer.joinable()) writer.join();
        throw;
    }
    if (writer.joinable()) writer.join();
    if (writer_error) std::rethrow_exception(writer_error);
    cout << "=== End of compression ===\n";
    return 0;
}
