// mcq_annotate_cli -- the reference's `metacache annotate taxid` (src/mode_annotate.cpp): taxid|N written into the headers of a genome
// file from *.accession2taxid files, so that the unchanged mcq_build_cli finds a parent for every target.
//   mcq_annotate_cli taxid INFILE MAPPING... [-out FILE | -outdir DIR] [-field-sep S] [-value-sep S] [-id=accver | -id=acc | -id=gi]
// The reference reads every line of every mapping file into one std::map and then looks up the ids of INFILE.  Here the join is turned
// round: the ids of INFILE are few, the mapping text is GBs, so the ids are collected first and the text is streamed against them.
//   pass 1  (host) every line of INFILE that begins with '>' or '@' is a header: its id (mcq_annotate_id) is collected; the distinct
//           ids, sorted, are the names of an mcq_accmap handle with the rule of the chosen column (mcq_accmap_create_rule)
//   pass 2  every mapping file is streamed through two pinned buffers: a thread reads the next chunk while the GPU joins this one
//           (mcq_accmap_chunk: the file's ordinal, the chunk's byte offset as line number).  From a chunk that is not strict on, the
//           rest of that file goes through the host parser (mcq_accmap_host_rule), record by record as the reference reads it
//   pass 3  (host) INFILE is copied, every header line rewritten (mcq_annotate_rewrite) with the taxid of its id, or 0
// Host memory: the buffers and the ids, whatever the size of the mapping files.  DESIGN.md section 34.
#include <sys/stat.h>
#include <sys/types.h>

#include <algorithm>
#include <cctype>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/mcq.h"
#include "../../../include/mcq_host.h"
#include "mcq_cli_buffers.hpp"

namespace {

const char* const kUsage =
    "usage: mcq_annotate_cli taxid INFILE MAPPING... [options]\n"
    "  writes INFILE (FASTA or FASTQ) with `taxid|N` put into every header line: N is the taxid that the first line of the MAPPING\n"
    "  files (NCBI's *.accession2taxid: accession, accession.version, taxid, gi; the first line of a file is passed over) gives the\n"
    "  header's id, or 0.  MAPPING is every argument up to the first option; a directory stands for the files in it, in name order.\n"
    "  An old taxid in a header is cut out.  The output ends at the first empty line of INFILE, as the reference's does.\n"
    "  -out FILE                 the annotated text goes to FILE (default: stdout, and the progress lines go to stderr)\n"
    "  -outdir DIR               INFILE may be a directory; every file F in it is written to DIR/<basename of F>; the mapping files\n"
    "                            are joined once against the ids of all files   [not in the reference]\n"
    "  -field-sep S              what separates the fields of a header (default \" \"; alias -field-separator)\n"
    "  -value-sep S              what separates `taxid` from its number (default \"|\"; alias -value-separator)\n"
    "  -id=accver | -id=acc | -id=gi\n"
    "                            the id of a header and the column of the mapping files it is looked up in (default -id=accver)\n"
    "  -mapper gpu|host          gpu (default): strict text is joined on the GPU, the rest on the host; host: everything on the host\n"
    "  -map-chunk BYTES          bytes of mapping text per chunk (default 67108864; 64 .. 2^32 - 1)\n"
    "  -io-bytes BYTES           the buffer INFILE is read through (default 1048576); a header line must fit into it\n"
    "  -device D                 the GPU to use (default 0)\n"
    "  -timing                   the milliseconds of the three passes on stderr\n"
    "  -help                     this text\n"
    "mcq_build_cli does not read mapping files itself (DESIGN.md sections 29 and 34): annotate the genomes first,\n"
    "  mcq_annotate_cli taxid GENOMES TAXDIR/nucl_gb.accession2taxid -outdir G2   and then   mcq_build_cli DB P G2 -taxonomy TAXDIR\n";

struct Opts {
    std::string infile, out, outdir, fs = " ", vs = "|";
    std::vector<std::string> mappings;
    uint32_t id_type = MCQ_ACCMAP_RULE_ACCVER;
    bool host_only = false, timing = false;
    uint64_t chunk = 64ull << 20, io = 1ull << 20;
    int device = 0;
};

int abort_with(const std::string& msg) { std::fprintf(stderr, "ABORT: %s\n", msg.c_str()); return 1; }
double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

struct File {
    FILE* f = nullptr;
    File() = default;
    File(const File&) = delete;
    File& operator=(const File&) = delete;
    ~File() { if (f) std::fclose(f); }
    bool open(const std::string& path, const char* mode) {
        f = std::fopen(path.c_str(), mode);
        if (!f) return false;
        struct stat st;
        if (mode[0] == 'r' && (fstat(fileno(f), &st) != 0 || S_ISDIR(st.st_mode))) { std::fclose(f); f = nullptr; return false; }
        return true;
    }
};

bool list_files(const std::string& arg, std::vector<std::string>& out) {
    const char* a = arg.c_str();
    mcq_file_list* l = nullptr;
    if (mcq_genome_files(&a, 1, &l)) return false;
    for (uint32_t i = 0; i < mcq_file_list_count(l); ++i) out.push_back(mcq_file_list_get(l, i));
    mcq_file_list_free(l);
    return true;
}

// ---- INFILE line by line through one buffer: getline's lines (the last one need not end in '\n'; nothing behind a last '\n').
// A line that begins with '>' or '@' comes in one piece (it must fit the buffer), any other in as many pieces as it takes.
struct Lines {
    struct Piece { const char* p; size_t n; bool begins_line; bool header; uint64_t off; };
    File in;
    std::vector<char> buf;
    size_t b = 0, e = 0;
    uint64_t base = 0;                          // file offset of buf[0]
    bool at_line_start = true, eof = false, too_long = false;
    bool open(const std::string& path, uint64_t io) { buf.resize((size_t)io); return in.open(path, "rb"); }
    void refill() {                             // keeps [b, e), moved to the front
        if (b) { std::memmove(buf.data(), buf.data() + b, e - b); base += b; e -= b; b = 0; }
        while (!eof && e < buf.size()) {
            const size_t got = std::fread(buf.data() + e, 1, buf.size() - e, in.f);
            if (!got) eof = true;
            e += got;
        }
        if (!eof && e == buf.size()) { const int c = std::fgetc(in.f); if (c == EOF) eof = true; else std::ungetc(c, in.f); }   // (a full buffer at the file's end)
    }
    bool next(Piece& pc) {
        if (b == e) { refill(); if (b == e) return false; }
        const bool header = at_line_start && (buf[b] == '>' || buf[b] == '@');
        const char* q = (const char*)std::memchr(buf.data() + b, '\n', e - b);
        if (!q && header && !eof) {
            refill();
            q = (const char*)std::memchr(buf.data() + b, '\n', e - b);
            if (!q && !eof) { too_long = true; return false; }
        }
        pc.p = buf.data() + b; pc.begins_line = at_line_start; pc.header = header; pc.off = base + b;
        if (q) { pc.n = (size_t)(q - pc.p); b += pc.n + 1; at_line_start = true; }
        else { pc.n = e - b; b = e; at_line_start = false; }
        return true;
    }
    bool more() { if (b == e) refill(); return b < e; }
};

struct Ids {
    std::vector<std::string> names;             // sorted as std::string compares (unsigned bytes, then length), distinct
    std::vector<uint8_t> unranked;
    std::vector<int64_t> parent;
    void seal() {
        std::sort(names.begin(), names.end());
        names.erase(std::unique(names.begin(), names.end()), names.end());
        unranked.assign(names.size(), 1); parent.assign(names.size(), 0);
    }
    uint64_t taxid_of(const std::string& id) const {
        auto it = std::lower_bound(names.begin(), names.end(), id);
        if (it == names.end() || *it != id) return 0;
        const size_t k = (size_t)(it - names.begin());
        return unranked[k] ? 0 : (uint64_t)parent[k];
    }
};

// one walk over a file: pass 1 (out == nullptr: the ids are collected) or pass 3 (the text is written).  0, or 1 after a message
int walk(const Opts& o, const std::string& path, Ids& ids, FILE* out) {
    Lines L;
    if (!L.open(path, o.io)) { std::fprintf(stderr, "Input file %s could not be opened.\n", path.c_str()); return 1; }
    std::vector<char> id((size_t)o.io + 1), line;
    Lines::Piece pc;
    bool first = true;
    while (L.next(pc)) {
        if (pc.begins_line && pc.n == 0) {      // the reference's loop ends at the first empty line (src/mode_annotate.cpp:302-309)
            if (out && L.more())
                std::fprintf(stderr, "%s: the output ends at the empty line at byte %llu; the text behind it is not copied\n", path.c_str(), (unsigned long long)pc.off);
            break;
        }
        if (!pc.header) {
            if (out) { if (pc.begins_line && !first) std::fputc('\n', out); std::fwrite(pc.p, 1, pc.n, out); }
        } else {
            const int64_t n = mcq_annotate_id(pc.p, pc.n, o.id_type, id.data(), id.size());
            if (n < 0) return abort_with(mcq_host_last_error());
            if (!out) { if (n) ids.names.emplace_back(id.data(), (size_t)n); }
            else {
                line.resize(pc.n + 32 + 2 * o.fs.size() + o.vs.size());
                const int64_t m = mcq_annotate_rewrite(pc.p, pc.n, n > 0, n ? ids.taxid_of(std::string(id.data(), (size_t)n)) : 0, o.fs.c_str(), o.vs.c_str(),
                                                       line.data(), line.size());
                if (m < 0 || (size_t)m >= line.size()) return abort_with(m < 0 ? mcq_host_last_error() : "a rewritten header outgrew its buffer");
                if (!first) std::fputc('\n', out);
                std::fwrite(line.data(), 1, (size_t)m, out);
            }
        }
        first = false;
    }
    if (L.too_long) return abort_with(path + ": a header line at byte " + std::to_string(L.base + L.b) + " is longer than the buffer (-io-bytes " + std::to_string(o.io) + ")");
    if (out && std::ferror(out)) return abort_with("writing the output failed");
    return 0;
}

// ---- pass 2 ----------------------------------------------------------------------------------------------------------------
struct TextBuf {                                // pinned for the GPU route, plain for -mapper host (which never touches the GPU)
    char* p = nullptr; bool pinned = false;
    TextBuf() = default;
    TextBuf(const TextBuf&) = delete;
    TextBuf& operator=(const TextBuf&) = delete;
    ~TextBuf() { if (p) { if (pinned) (void)hipHostFree(p); else std::free(p); } }
    bool alloc(uint64_t n, bool pin) {
        pinned = pin;
        if (pin) { MCQ_HIP(hipHostMalloc((void**)&p, n, hipHostMallocDefault), return false); return true; }
        p = (char*)std::malloc(n);
        return p != nullptr;
    }
};

struct Join {
    const Opts& o;
    Ids& ids;
    std::string blob; std::vector<uint64_t> off; std::vector<uint32_t> tgt;
    TextBuf slot[2];
    DeviceBuf<char> dev;
    Stream st;
    mcq_accmap* h = nullptr;
    double ms_gpu = 0, ms_host = 0;
    uint64_t gpu_chunks = 0, host_files = 0;
    Join(const Opts& o_, Ids& ids_) : o(o_), ids(ids_) {}
    ~Join() { if (h) mcq_accmap_free(h); }
    bool start() {
        off.push_back(0);
        for (size_t k = 0; k < ids.names.size(); ++k) { blob += ids.names[k]; off.push_back(blob.size()); tgt.push_back((uint32_t)k); }
        if (!slot[0].alloc(o.chunk, !o.host_only)) return false;
        if (o.host_only) return true;
        MCQ_HIP(hipSetDevice(o.device), return false);
        if (!slot[1].alloc(o.chunk, true) || !dev.grow(o.chunk) || !st.create()) return false;
        if (mcq_accmap_create_rule(blob.data(), off.data(), ids.names.size(), tgt.data(), ids.unranked.data(), (uint32_t)ids.names.size(), o.id_type,
                                   o.device, &h)) { abort_with(mcq_last_error()); return false; }
        return true;
    }
    // what the handle has found so far goes to the ids the host has not ranked: every chunk so far lies before what the host reads next
    bool absorb() {
        if (!h || ids.names.empty()) return true;
        std::vector<int64_t> parent(ids.names.size()); std::vector<uint8_t> found(ids.names.size());
        if (mcq_accmap_finish(h, parent.data(), found.data())) { abort_with(mcq_last_error()); return false; }
        for (size_t k = 0; k < found.size(); ++k) if (found[k] && ids.unranked[k]) { ids.unranked[k] = 0; ids.parent[k] = parent[k]; }
        return true;
    }
    // carry bytes from `carry`, then the file, into buf: the number of bytes there; *eof when the file gave no more
    static uint64_t fill(FILE* f, char* buf, uint64_t cap, const char* carry, uint64_t n_carry, bool* eof) {
        if (n_carry) std::memmove(buf, carry, (size_t)n_carry);
        uint64_t n = n_carry;
        *eof = false;
        while (n < cap) {
            const size_t got = std::fread(buf + n, 1, (size_t)(cap - n), f);
            if (!got) { *eof = true; break; }
            n += got;
        }
        return n;
    }
    // the rest of a file from byte `from` on through the host parser, as one stream of records: a buffer is cut behind its last white
    // space (every word in front of it is whole), parsed, and what lies behind the last whole record is carried into the next
    bool host_rest(FILE* f, const std::string& path, uint64_t from) {
        const auto t0 = std::chrono::steady_clock::now();
        ++host_files;
        if (fseeko(f, (off_t)from, SEEK_SET) != 0) { abort_with(path + " cannot be positioned"); return false; }
        char* buf = slot[0].p;
        uint64_t n_carry = 0, carry_at = 0;
        for (;;) {
            bool eof = false;
            const uint64_t n = fill(f, buf, o.chunk, buf + carry_at, n_carry, &eof);
            uint64_t cut = n;
            if (!eof) while (cut && !std::isspace((unsigned char)buf[cut - 1])) --cut;
            uint64_t consumed = 0; int32_t stopped = 0;
            if (mcq_accmap_host_rule(buf, cut, 0, blob.data(), off.data(), ids.names.size(), tgt.data(), ids.unranked.data(), ids.parent.data(),
                                     (uint32_t)ids.names.size(), o.id_type, nullptr, &consumed, &stopped)) { abort_with(mcq_host_last_error()); return false; }
            if (stopped || eof) break;
            if (consumed == 0 && n == o.chunk) { abort_with(path + ": a record of the mapping text is longer than -map-chunk " + std::to_string(o.chunk)); return false; }
            carry_at = consumed; n_carry = n - consumed;
        }
        ms_host += ms_since(t0);
        return true;
    }
    // one mapping file: its first line passed over, then chunks of whole lines to the GPU until one is not strict
    bool file(const std::string& path, uint32_t ordinal, FILE* msg) {
        File in;
        if (!in.open(path, "rb")) { std::fprintf(stderr, "File '%s' could not be read.\n", path.c_str()); return true; }
        std::fprintf(msg, "Processing mappings in file '%s'\n", path.c_str()); std::fflush(msg);
        if (ids.names.empty()) return true;
        uint64_t at = 0;                                                   // (getline: through the first '\n')
        for (int c; (c = std::fgetc(in.f)) != EOF;) { ++at; if (c == '\n') break; }
        if (o.host_only) return host_rest(in.f, path, at);
        if (ordinal >= (1u << 23)) return abort_with("more than 2^23 mapping files"), false;
        bool eof = false;
        int cur = 0;
        uint64_t n = fill(in.f, slot[0].p, o.chunk, nullptr, 0, &eof);
        while (n) {
            uint64_t cut = n;
            if (!eof) while (cut && slot[cur].p[cut - 1] != '\n') --cut;
            if (!cut) return absorb() && host_rest(in.f, path, at);       // (a line longer than a chunk)
            uint64_t n_next = 0; bool eof_next = true;
            std::thread reader;
            if (!eof) reader = std::thread([&, cur, cut, n]() { n_next = fill(in.f, slot[cur ^ 1].p, o.chunk, slot[cur].p + cut, n - cut, &eof_next); });
            struct Joiner { std::thread& t; ~Joiner() { if (t.joinable()) t.join(); } } joiner{reader};
            const auto t0 = std::chrono::steady_clock::now();
            uint32_t strict = 0;
            MCQ_HIP(hipMemcpyAsync(dev.p, slot[cur].p, cut, hipMemcpyHostToDevice, st), return false);
            if (mcq_accmap_chunk(h, dev.p, cut, ordinal, at, &strict, st.h)) { abort_with(mcq_last_error()); return false; }
            ms_gpu += ms_since(t0); ++gpu_chunks;
            if (reader.joinable()) reader.join();
            if (!strict) return absorb() && host_rest(in.f, path, at);
            at += cut; cur ^= 1; n = n_next; eof = eof_next;
        }
        return true;
    }
};

bool parse(int argc, char** argv, Opts& o) {
    std::vector<std::string> pos;
    bool accver = false, acc = false, gi = false, seen_option = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto next = [&]() -> const char* { return (i + 1 < argc) ? argv[++i] : ""; };
        if (a == "-help" || a == "--help" || a == "-h") { std::fputs(kUsage, stdout); return false; }
        if (a.size() < 2 || a[0] != '-') {
            if (seen_option) { abort_with("argument " + a + " behind the options: the mapping files stand in front of the first option"); return false; }
            pos.push_back(a);
            continue;
        }
        seen_option = true;
        if (a == "-out") o.out = next();
        else if (a == "-outdir") o.outdir = next();
        else if (a == "-field-sep" || a == "-field-separator") o.fs = next();
        else if (a == "-value-sep" || a == "-value-separator") o.vs = next();
        else if (a == "-id=accver") accver = true;
        else if (a == "-id=acc") acc = true;
        else if (a == "-id=gi") gi = true;
        else if (a == "-mapper") {
            const std::string m = next();
            if (m != "gpu" && m != "host") { abort_with("-mapper takes gpu or host"); return false; }
            o.host_only = m == "host";
        }
        else if (a == "-map-chunk") o.chunk = std::strtoull(next(), nullptr, 10);
        else if (a == "-io-bytes") o.io = std::strtoull(next(), nullptr, 10);
        else if (a == "-device") o.device = std::atoi(next());
        else if (a == "-timing") o.timing = true;
        else { abort_with("option " + a + " is not supported by mcq_annotate_cli"); return false; }
    }
    if (pos.empty()) { std::fputs(kUsage, stderr); abort_with("No annotation mode provided."); return false; }
    if (pos[0] != "taxid") { abort_with("Annotation mode '" + pos[0] + "' not recognized."); return false; }
    if (pos.size() < 2) { abort_with("No input filename provided."); return false; }
    if (pos.size() < 3) { abort_with("No taxonomic mapping filenames provided"); return false; }
    o.infile = pos[1];
    for (size_t k = 2; k < pos.size(); ++k) if (!list_files(pos[k], o.mappings)) { abort_with(mcq_host_last_error()); return false; }
    o.id_type = accver ? MCQ_ACCMAP_RULE_ACCVER : (acc ? MCQ_ACCMAP_RULE_ACC : (gi ? MCQ_ACCMAP_RULE_GI : MCQ_ACCMAP_RULE_ACCVER));   // (the reference's order)
    if (o.fs.empty() || o.vs.empty()) { abort_with("the separators must not be empty"); return false; }
    if (o.chunk < 64 || o.chunk >= (1ull << 32)) { abort_with("-map-chunk takes 64 .. 4294967295 bytes"); return false; }
    if (o.io < 64 || o.io >= (1ull << 32)) { abort_with("-io-bytes takes 64 .. 4294967295 bytes"); return false; }
    if (!o.out.empty() && !o.outdir.empty()) { abort_with("-out and -outdir exclude each other"); return false; }
    return true;
}

std::string basename_of(const std::string& f) { const size_t i = f.find_last_of('/'); return i == std::string::npos ? f : f.substr(i + 1); }

}  // namespace

int main(int argc, char** argv) {
    Opts o;
    if (!parse(argc, argv, o)) return 1;
    FILE* msg = (o.out.empty() && o.outdir.empty()) ? stderr : stdout;       // DIVERGENCE: the text alone on stdout when it goes there
    std::vector<std::string> inputs, outputs;
    if (o.outdir.empty()) { inputs.push_back(o.infile); outputs.push_back(o.out); }
    else {
        if (!list_files(o.infile, inputs)) return abort_with(mcq_host_last_error());
        std::string dir = o.outdir;
        if (dir.back() != '/') dir += '/';
        for (const std::string& f : inputs) outputs.push_back(dir + basename_of(f));
        std::vector<std::string> sorted = outputs;
        std::sort(sorted.begin(), sorted.end());
        const auto dup = std::adjacent_find(sorted.begin(), sorted.end());
        if (dup != sorted.end()) return abort_with("two input files would be written to " + *dup);
    }
    std::fprintf(msg, "Annotating sequences in '%s' with taxonomic ids.\nOutput will be written to '%s'\n", o.infile.c_str(),
                 !o.outdir.empty() ? o.outdir.c_str() : (o.out.empty() ? "stdout" : o.out.c_str()));
    std::fflush(msg);
    // pass 1: the ids
    auto t0 = std::chrono::steady_clock::now();
    Ids ids;
    for (const std::string& f : inputs) if (int rc = walk(o, f, ids, nullptr)) return rc;
    ids.seal();
    const double ms1 = ms_since(t0);
    // pass 2: the join
    t0 = std::chrono::steady_clock::now();
    Join join(o, ids);
    if (!join.start()) return 1;
    for (size_t k = 0; k < o.mappings.size(); ++k) if (!join.file(o.mappings[k], (uint32_t)k, msg)) return 1;
    if (!join.absorb()) return 1;
    const double ms2 = ms_since(t0);
    // pass 3: the text
    t0 = std::chrono::steady_clock::now();
    if (!o.outdir.empty()) (void)mkdir(o.outdir.c_str(), 0777);
    if (msg == stdout) { std::fputs("Mapping ... ", msg); std::fflush(msg); }
    for (size_t k = 0; k < inputs.size(); ++k) {
        File out;
        FILE* to = stdout;
        if (!outputs[k].empty()) {
            if (!out.open(outputs[k], "wb")) { std::fprintf(stderr, "Output file %s could not be opened.\n", outputs[k].c_str()); return 1; }
            to = out.f;
        }
        if (int rc = walk(o, inputs[k], ids, to)) return rc;
        if (std::fflush(to) != 0) return abort_with("writing " + (outputs[k].empty() ? std::string("stdout") : outputs[k]) + " failed");
    }
    if (msg == stdout) std::fputs("complete.\n", msg);
    if (o.timing)
        std::fprintf(stderr, "phases ms: ids %.3f, join %.3f (gpu chunks %.3f in %llu calls, host parser %.3f in %llu files), text %.3f; ids %llu\n", ms1, ms2,
                     join.ms_gpu, (unsigned long long)join.gpu_chunks, join.ms_host, (unsigned long long)join.host_files, ms_since(t0),
                     (unsigned long long)ids.names.size());
    return 0;
}
