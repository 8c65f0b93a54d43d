// mcq_host_build.cpp -- the build side of the host library (include/mcq_host.h): the NCBI taxonomy dump, the genome files
// and what the reference makes of their headers.  Plain C++14, no GPU.  Each part names the reference code it restates.
#include "../../../include/mcq_host.h"
#include "mcq_host_internal.hpp"

#include <algorithm>
#include <cctype>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <dirent.h>
#include <fcntl.h>
#include <map>
#include <set>
#include <string>
#include <unistd.h>
#include <vector>

namespace {
int fail(const std::string& m) { return mcq_host_set_error(m.c_str()); }

bool slurp(const std::string& path, std::string& out) {
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    char buf[1 << 16]; size_t n;
    out.clear();
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) out.append(buf, n);
    std::fclose(f);
    return true;
}

// formatted extraction as the reference's parsers use it on an std::ifstream (operator>> of an integer / a string,
// ignore(max, c)): leading white space is skipped, a word ends at white space, a failed extraction ends the parse
struct Cursor {
    const char* p; const char* e; bool ok = true;
    Cursor(const std::string& s) : p(s.data()), e(s.data() + s.size()) {}
    bool good() const { return ok && p < e; }
    void ws() { while (p < e && std::isspace((unsigned char)*p)) ++p; }
    bool integer(int64_t& v) {
        ws();
        const char* q = p; bool neg = false;
        if (q < e && (*q == '-' || *q == '+')) { neg = *q == '-'; ++q; }
        if (q >= e || !std::isdigit((unsigned char)*q)) { ok = false; return false; }
        int64_t x = 0;
        while (q < e && std::isdigit((unsigned char)*q)) { x = x * 10 + (*q - '0'); ++q; }
        v = neg ? -x : x; p = q;
        return true;
    }
    bool word(std::string& w) {
        ws();
        if (p >= e) { ok = false; return false; }
        const char* q = p;
        while (q < e && !std::isspace((unsigned char)*q)) ++q;
        w.assign(p, q); p = q;
        return true;
    }
    void past(char c) {
        const void* q = std::memchr(p, c, (size_t)(e - p));
        p = q ? (const char*)q + 1 : e;
    }
};

struct TaxNode { int64_t parent; uint8_t rank; std::string name; };
}  // namespace

// ---- make_taxonomic_hierarchy (src/taxonomy_io.cpp:56-185): names.dmp (scientific names only, :73-102), merged.dmp (:111-130:
// every old id becomes a taxon of rank none whose parent is the new id, and ids of nodes.dmp are replaced by their new ones),
// nodes.dmp (:134-171; rank names through taxonomy::rank_from_name, src/taxonomy.h:173-213 = mcq_rank_from_name; a rank of two
// words such as "species group" is joined), rank of taxon 1 set to root (:179).  The taxa live in a std::set ordered by id
// (src/taxonomy.h:290-294, :348) into which emplace does not overwrite (:414): the first record of an id wins, and the order
// written (src/taxonomy.h:660-676) is ascending id.
struct mcq_taxdump {
    std::map<int64_t, TaxNode> taxa;
    std::vector<mcq_taxon_rec> recs;
};

extern "C" int mcq_taxdump_read(const char* dir, mcq_taxdump** out) {
    if (!dir || !out) return fail("null argument");
    std::string path = dir;
    if (!path.empty() && path.back() != '/') path += '/';                  // src/args_handling.cpp:112-118
    std::string text;
    std::map<int64_t, std::string> names;
    if (slurp(path + "names.dmp", text)) {
        Cursor c(text);
        int64_t last = 0, id = 0;
        std::string name, w, category;
        while (c.good()) {
            if (!c.integer(id)) break;
            if (id != last) {
                c.past('|');
                name.clear();
                c.word(name);
                while (c.good()) {
                    if (!c.word(w) || w.find('|') != std::string::npos) break;
                    name += " " + w;
                }
                c.past('|');
                if (c.word(category) && category.find("scientific") != std::string::npos) { last = id; names.insert({id, name}); }
            }
            c.past('\n');
        }
    } else std::fprintf(stderr, "Could not read taxon names file %snames.dmp; continuing with ids only.\n", path.c_str());

    mcq_taxdump* T = new mcq_taxdump();
    auto emplace = [&](int64_t id, int64_t parent, const std::string& name, uint8_t rank) {
        if (id != 0) T->taxa.insert({id, TaxNode{parent, rank, name}});
    };
    std::map<int64_t, int64_t> merged;
    if (slurp(path + "merged.dmp", text)) {
        Cursor c(text);
        int64_t oldid = 0, newid = 0;
        while (c.good()) {
            if (!c.integer(oldid)) break;
            c.past('|');
            if (!c.integer(newid)) break;
            c.past('\n');
            merged.insert({oldid, newid});
            emplace(oldid, newid, "", (uint8_t)MCQ_RANK_NONE);
        }
    }
    if (!slurp(path + "nodes.dmp", text)) { delete T; return fail("Could not read taxonomic nodes file " + path + "nodes.dmp"); }
    {
        Cursor c(text);
        int64_t id = 0, parent = 0;
        std::string rank, ext;
        while (c.good()) {
            if (!c.integer(id)) break;
            c.past('|');
            if (!c.integer(parent)) break;
            c.past('|');
            if (!c.word(rank)) break;
            if (c.word(ext) && ext != "|") rank += ' ' + ext;
            c.past('\n');
            auto it = names.find(id);
            std::string name = it != names.end() ? it->second : std::string("--");
            if (name.empty()) name = "<" + std::to_string(id) + ">";
            auto mi = merged.find(id);
            if (mi != merged.end()) id = mi->second;
            mi = merged.find(parent);
            if (mi != merged.end()) parent = mi->second;
            emplace(id, parent, name, (uint8_t)mcq_rank_from_name(rank.c_str()));
        }
    }
    auto root = T->taxa.find(1);
    if (root != T->taxa.end()) root->second.rank = (uint8_t)MCQ_RANK_ROOT;
    for (const auto& t : T->taxa) {
        mcq_taxon_rec r; r.id = t.first; r.parent = t.second.parent; r.rank = t.second.rank; r.name = t.second.name.c_str();
        r.file = ""; r.index = 0; r.windows = 0;
        T->recs.push_back(r);
    }
    *out = T;
    return 0;
}
extern "C" uint64_t mcq_taxdump_count(const mcq_taxdump* t) { return t ? t->recs.size() : 0; }
extern "C" const mcq_taxon_rec* mcq_taxdump_taxa(const mcq_taxdump* t) { return t && !t->recs.empty() ? t->recs.data() : nullptr; }
extern "C" int mcq_taxdump_free(mcq_taxdump* t) { delete t; return 0; }

// ---- what a sequence header gives: extract_accession_string (src/sequence_io.cpp:705-719) and extract_taxon_id (:724-748) ----
namespace {
const char* const kAccessionPrefix[] = {"GCF_", "AC_", "NC_", "NG_", "NS_", "NT_", "NW_", "NZ_", "MKHE", "AE", "AJ", "AL", "AM", "AP",
                                        "AY", "BA", "BK", "BX", "CC", "CM", "CP", "CR", "CT", "CU", "FM", "FN", "FO", "FP", "FQ", "FR",
                                        "HE", "JH"};                       // src/sequence_io.cpp:43-58
const size_t npos = std::string::npos;

std::string trimmed(const std::string& s) {
    size_t b = 0, e = s.size();
    while (b < e && std::isspace((unsigned char)s[b])) ++b;
    while (e > b && std::isspace((unsigned char)s[e - 1])) --e;
    return s.substr(b, e - b);
}
// the first of '|', ' ', '-', '_', ',' that occurs at all from `start` on -- in this order of preference, not the nearest (:576-598)
size_t accession_end(const std::string& t, size_t start) {
    if (start >= t.size()) return t.size();
    for (char c : {'|', ' ', '-', '_', ','}) { const size_t k = t.find(c, start); if (k != npos) return k; }
    return t.size();
}
std::string accession_version(const std::string& t) {                      // :602-642
    if (t.size() < 2) return "";
    for (const char* prefix : kAccessionPrefix) {
        const size_t i = t.find(prefix);
        if (i == npos) continue;
        const size_t s = t.find('.', i + std::strlen(prefix));
        if (s == npos || s - i > 25) continue;
        const std::string num = trimmed(t.substr(i, accession_end(t, s + 1) - i));
        if (!num.empty()) return num;
    }
    const size_t s = t.find('.', 1);
    if (s < 25) return trimmed(t.substr(0, accession_end(t, s + 1)));
    return "";
}
std::string accession_plain(const std::string& t) {                        // :647-677
    for (const char* prefix : kAccessionPrefix) {
        const size_t i = t.find(prefix);
        if (i == npos) continue;
        const size_t j = i + std::strlen(prefix);
        size_t k = accession_end(t, j);
        const size_t l = t.find('.', j);
        if (l < k) k = l;
        const std::string num = trimmed(t.substr(i, k - i));
        if (!num.empty()) return num;
    }
    return "";
}
std::string genbank_id(const std::string& t) {                             // :682-700
    size_t i = t.find("gi|");
    if (i == npos) return "";
    i += 3;
    size_t j = t.find('|', i);
    if (j == npos) { j = t.find(' ', i); if (j == npos) j = t.size(); }
    return trimmed(t.substr(i, j - i));
}
// the sequence id of a target (src/mode_build.cpp:591-596): the accession string, else the whole header
std::string target_name(const std::string& header) {
    if (header.empty()) return header;
    std::string s = accession_version(header);
    if (s.empty()) s = accession_plain(header);
    if (s.empty()) s = genbank_id(header);
    return s.empty() ? header : s;
}
int64_t header_taxid(const std::string& t) {
    size_t i = t.find("taxid");
    if (i == npos) return 0;
    i += 6;                                                                // "taxid" and one separator character
    if (i > t.size()) return 0;                                            // (substr would throw: caught, 0)
    size_t j = t.find('|', i);
    if (j == npos) { j = t.find(' ', i); if (j == npos) j = t.size(); }
    const std::string num = t.substr(i, j - i);
    const char* p = num.c_str();                                           // std::stoull: white space, sign, digits
    while (std::isspace((unsigned char)*p)) ++p;
    const char* d = p;
    if (*d == '+' || *d == '-') ++d;
    if (!std::isdigit((unsigned char)*d)) return 0;
    errno = 0;
    const unsigned long long v = std::strtoull(p, nullptr, 10);
    if (errno == ERANGE) return 0;
    return (int64_t)v;
}
}  // namespace

std::string mcq_header_accession_version(const std::string& header) { return accession_version(header); }
std::string mcq_header_accession(const std::string& header) { return accession_plain(header); }
int64_t mcq_header_taxid(const std::string& header) { return header_taxid(header); }

extern "C" int64_t mcq_target_name(const char* header, uint64_t len, char* buf, size_t cap) {
    if ((len && !header) || (cap && !buf)) return fail("null argument");
    const std::string s = target_name(std::string(header ? header : "", (size_t)len));
    if (cap) { const size_t n = std::min(cap - 1, s.size()); std::memcpy(buf, s.data(), n); buf[n] = 0; }
    return (int64_t)s.size();
}
extern "C" int64_t mcq_target_parent_taxid(const char* header, uint64_t len) {
    const int64_t v = header_taxid(std::string(header ? header : "", header ? (size_t)len : 0));
    return v < 1 ? 0 : v;                                                  // src/sketch_database.h:545
}

// ---- the genome files of a command line: sequence_filenames (src/args_handling.cpp:50-90) expands every argument that is a
// directory (files_in_directory, src/filesys_utility.cpp:32-73: recursive, 10 levels) and add_targets_to_database sorts the names
// (src/mode_build.cpp:570-575).  Target ids follow this order.
namespace {
std::vector<std::string> files_in(std::string dir, int recurse) {
    if (!dir.empty() && (dir.back() == '/' || dir.back() == '\\')) dir.pop_back();
    std::vector<std::string> files;
    DIR* d = opendir(dir.c_str());
    if (!d) return files;
    while (dirent* e = readdir(d)) {
        if (!std::strcmp(e->d_name, ".") || !std::strcmp(e->d_name, "..")) continue;
        const std::string path = dir + "/" + e->d_name;
        std::vector<std::string> below;
        if (recurse > 0) below = files_in(path, recurse - 1);
        if (below.empty()) files.push_back(path);
        else files.insert(files.end(), below.begin(), below.end());
    }
    closedir(d);
    return files;
}
}  // namespace
struct mcq_file_list { std::vector<std::string> files; };
extern "C" int mcq_genome_files(const char* const* args, uint32_t n_args, mcq_file_list** out) {
    if ((n_args && !args) || !out) return fail("null argument");
    mcq_file_list* L = new mcq_file_list();
    for (uint32_t i = 0; i < n_args; ++i) {
        std::vector<std::string> f = files_in(args[i], 10);
        if (f.empty()) L->files.push_back(args[i]);
        else L->files.insert(L->files.end(), f.begin(), f.end());
    }
    std::sort(L->files.begin(), L->files.end());
    *out = L;
    return 0;
}
extern "C" uint32_t mcq_file_list_count(const mcq_file_list* l) { return l ? (uint32_t)l->files.size() : 0; }
extern "C" const char* mcq_file_list_get(const mcq_file_list* l, uint32_t i) { return l && i < l->files.size() ? l->files[i].c_str() : ""; }
extern "C" int mcq_file_list_free(mcq_file_list* l) { delete l; return 0; }

// ---- the genome reader: fasta_reader (src/sequence_io.cpp:121-170) over the files in order, as add_targets_to_database
// (src/mode_build.cpp:578-646) and add_target_distributed (src/sketch_database.h:519-563) use it.  A record is a '>' line and
// the lines up to the next line that starts with '>', joined without their '\n' (a '\r' stays, an empty line adds nothing).
// A file whose first line does not start with '>', and a record without any sequence text, end the reading of THAT file (the
// reader throws, the loop over the file is left: :139, :161, :639); a file that cannot be opened is passed over (:585-586,
// :639).  A record whose sequence id is already taken is not added and gets no target id (:534); the index of a record
// counts every record of its file from 1 (src/sequence_io.cpp:66-77).  Host memory: the io buffer and one header line,
// plus name, file and length per target.
namespace {
// 1 = FASTA by its extension, 2 = FASTQ by its extension, 0 = by its first character.  The comparisons are the reference's, in
// its unsigned arithmetic: the FIRST ".fa" must be the last three characters, and for a name shorter than the extension n - 6
// wraps to npos (a 5-character name such as "a1.fa" is taken for FASTQ).
int file_kind(const std::string& f) {
    const size_t n = f.size();
    if (f.find(".fq") == n - 3 || f.find(".fnq") == n - 4 || f.find(".fastq") == n - 6) return 2;
    if (f.find(".fa") == n - 3 || f.find(".fna") == n - 4 || f.find(".fasta") == n - 6) return 1;
    return 0;
}
}  // namespace
struct mcq_genome_reader {
    std::vector<std::string> files; size_t next_file = 0;
    int fd = -1; std::vector<char> io; size_t pos = 0, end = 0; bool file_eof = false;
    bool at_line_start = true, in_header = false, first_line = true;
    enum { NONE, PENDING, ACCEPTED, SKIPPED } rec = NONE;
    std::string header; uint64_t index = 0;
    struct Target { std::string name; int64_t parent; uint32_t file; uint64_t index, length; };
    std::vector<Target> targets;
    std::set<std::string> names;
    uint32_t first_target = 0;         // mcq_genome_reader_open_after: the targets of the database come before this reader's
    uint64_t n_skipped = 0;
    std::map<std::string, int64_t> seq2tax;    // mcq_genome_reader_open_mapped: the pre-mapping (empty: the header's taxid|N alone)
    int64_t parent_of(const std::string& name, const std::string& file) const;
    ~mcq_genome_reader() { if (fd >= 0) ::close(fd); }
    void leave_file() { if (fd >= 0) ::close(fd); fd = -1; }
    bool open_next() {                 // false: no file left
        while (next_file < files.size()) {
            const std::string& f = files[next_file++];
            fd = ::open(f.c_str(), O_RDONLY);
            if (fd < 0) { std::fprintf(stderr, "mcq: can't open file %s (passed over)\n", f.c_str()); continue; }
            pos = end = 0; file_eof = false; at_line_start = true; in_header = false; first_line = true; rec = NONE; index = 0;
            return true;
        }
        return false;
    }
};

extern "C" int mcq_genome_reader_open(const char* const* files, uint32_t n_files, uint64_t io_bytes, mcq_genome_reader** out) {
    if ((n_files && !files) || !out) return fail("null argument");
    mcq_genome_reader* r = new mcq_genome_reader();
    for (uint32_t i = 0; i < n_files; ++i) r->files.push_back(files[i]);
    r->io.resize((size_t)std::max<uint64_t>(1, io_bytes));
    *out = r;
    return 0;
}

extern "C" int mcq_genome_reader_open_after(const char* const* files, uint32_t n_files, uint64_t io_bytes, const mcq_refdb* existing,
                                            mcq_genome_reader** out) {
    mcq_refdb_info info;
    if (!existing || mcq_refdb_get_info(existing, &info)) return fail("null argument");
    mcq_genome_reader* r = nullptr;
    if (mcq_genome_reader_open(files, n_files, io_bytes, &r)) return -1;
    for (uint32_t i = 0; i < info.n_taxa; ++i)                                 // name2tax_ of a database that was read (src/sketch_database.h:938-943)
        if (mcq_refdb_taxon_rank(existing, i) == MCQ_RANK_SEQUENCE) r->names.insert(mcq_refdb_taxon_name(existing, i));
    r->first_target = info.n_targets;
    *out = r;
    return 0;
}
extern "C" uint64_t mcq_genome_reader_n_skipped(const mcq_genome_reader* r) { return r ? r->n_skipped : 0; }

extern "C" int mcq_genome_reader_next(mcq_genome_reader* r, char* bases, uint64_t cap, uint64_t* n_bases, int32_t* done) {
    if (!r || (cap && !bases) || !n_bases || !done) return fail("null argument");
    if (cap < 1) return fail("the buffer holds at least one base");
    uint64_t n = 0;
    *done = 0;
    for (;;) {
        if (r->fd < 0 && !r->open_next()) { *done = 1; break; }
        if (r->pos == r->end) {
            if (r->file_eof) { r->leave_file(); continue; }
            ssize_t got;
            do got = ::read(r->fd, r->io.data(), r->io.size()); while (got < 0 && errno == EINTR);
            if (got < 0) {                                                 // (a directory among the names: the reference's reader gives nothing, the file is left)
                std::fprintf(stderr, "mcq: can't read %s: %s (passed over)\n", r->files[r->next_file - 1].c_str(), std::strerror(errno));
                r->leave_file(); continue;
            }
            if (got == 0) { r->file_eof = true; continue; }
            r->pos = 0; r->end = (size_t)got;
        }
        const char* b = r->io.data();
        if (r->at_line_start) {
            const char c = b[r->pos];
            if (r->first_line) {
                r->first_line = false;
                // make_sequence_reader (src/sequence_io.cpp:534-571): the extension decides, the first character only without one.
                // A FASTA reader on a file that does not begin with '>' and a FASTQ reader on one that does not begin with '@' throw:
                // the file is left.  What the reference would read as FASTQ is the one thing not restated: an error.
                const std::string& f = r->files[r->next_file - 1];
                const int kind = file_kind(f);
                if (c == '@' && kind != 1) { r->leave_file(); return fail("FASTQ genome files are not supported: " + f); }
                if (c != '>' || kind == 2) { r->leave_file(); continue; }
            }
            r->at_line_start = false;
            if (c == '>') {
                if (r->rec == mcq_genome_reader::PENDING) { r->leave_file(); continue; }      // the record before had no sequence text
                r->header.clear(); r->in_header = true; ++r->pos;
                continue;
            }
        }
        const char* nl = (const char*)std::memchr(b + r->pos, '\n', r->end - r->pos);
        const size_t stop = nl ? (size_t)(nl - b) : r->end;
        if (r->in_header) {
            r->header.append(b + r->pos, stop - r->pos);
            r->pos = stop;
            if (nl) { ++r->pos; r->in_header = false; r->at_line_start = true; r->rec = mcq_genome_reader::PENDING; ++r->index; }
            continue;
        }
        if (stop > r->pos) {
            if (r->rec == mcq_genome_reader::PENDING) {
                std::string name = target_name(r->header);
                if (r->names.count(name)) { r->rec = mcq_genome_reader::SKIPPED; ++r->n_skipped; }
                else {
                    if ((uint64_t)r->first_target + r->targets.size() >= 0xFFFFFFFFull) return fail("more targets than a 32-bit target id holds");
                    r->names.insert(name);
                    const int64_t parent = r->parent_of(name, r->files[r->next_file - 1]);
                    r->targets.push_back({std::move(name), parent < 1 ? 0 : parent, (uint32_t)(r->next_file - 1), r->index, 0});
                    r->rec = mcq_genome_reader::ACCEPTED;
                }
            }
            if (r->rec == mcq_genome_reader::ACCEPTED) {
                const size_t take = (size_t)std::min<uint64_t>(stop - r->pos, cap - n);
                std::memcpy(bases + n, b + r->pos, take);
                n += take; r->pos += take; r->targets.back().length += take;
                if (r->pos < stop) break;                                  // the buffer is full
            } else r->pos = stop;
        }
        if (nl && r->pos == stop) { ++r->pos; r->at_line_start = true; }
        if (n == cap) break;
    }
    *n_bases = n;
    return 0;
}
extern "C" uint32_t mcq_genome_reader_n_targets(const mcq_genome_reader* r) { return r ? (uint32_t)r->targets.size() : 0; }
extern "C" int mcq_genome_reader_target(const mcq_genome_reader* r, uint32_t t, mcq_taxon_rec* rec, uint64_t* length) {
    if (!r || t >= r->targets.size()) return fail("no such target");
    const mcq_genome_reader::Target& x = r->targets[t];
    if (rec) {
        rec->id = -((int64_t)r->first_target + t) - 1; rec->parent = x.parent; rec->rank = (uint8_t)MCQ_RANK_SEQUENCE; rec->name = x.name.c_str();
        rec->file = r->files[x.file].c_str(); rec->index = x.index; rec->windows = 0;
    }
    if (length) *length = x.length;
    return 0;
}
extern "C" int mcq_genome_reader_close(mcq_genome_reader* r) { delete r; return 0; }

// ---- pre-mapping: read_sequence_to_taxon_id_mapping and make_sequence_to_taxon_id_map (src/taxonomy_io.cpp:190-310), find_taxon_id
// (src/mode_build.cpp:531-550).  The reader with its quirks: up to 10 leading '#' lines, the LAST of them is the header row (without
// one: the first line); the header's first word is dropped and the others are numbered from 0: `taxid` gives taxcol,
// `accession.version` / `assembly_accession` keycol; a data line is read as keycol TABs passed, a word, taxcol TABs passed, an
// integer, the rest of the line passed -- so the taxid is taken from column keycol + taxcol, and both passes run across lines.
// Without a taxid column (taxcol < 1) the file is read again from its first byte as `key TAB taxid` (keycol stays).  A taxid that
// does not parse is entered as 0 and ends the file; at the end of the text the taxid of the line before is entered; map.insert
// keeps the first entry of a key.  Not restated: the entry {"", undefined} the reference makes for a file without any data line
// (no lookup can find it).
struct mcq_seq2tax {
    std::map<std::string, int64_t> map;
    std::vector<std::map<std::string, int64_t>::const_iterator> order;     // for mcq_seq2tax_entry
};
namespace {
struct LineIn {                        // std::getline on an ifstream: good() until a read has hit the end of the text
    const char* p; const char* e; bool eof = false, failed = false;
    bool good() const { return !eof && !failed; }
    void getline(std::string& line) {
        if (!good()) { failed = true; return; }                            // (the line keeps its text)
        const char* q = p < e ? (const char*)std::memchr(p, '\n', (size_t)(e - p)) : nullptr;
        if (q) { line.assign(p, q); p = q + 1; return; }
        line.assign(p, e); p = e; eof = true;
        if (line.empty()) failed = true;
    }
};
void read_seq2tax_text(const std::string& text, std::map<std::string, int64_t>& map) {
    const char* const b = text.data(); const char* const e = b + text.size();
    int header_row = 0;
    {
        LineIn is{b, e};
        std::string line;
        for (int i = 0; i < 10; ++i, ++header_row) { is.getline(line); if (line.empty() || line[0] != '#') break; }
        if (header_row > 0) --header_row;
    }
    LineIn is{b, e};
    std::string line;
    for (int i = 0; i < header_row; ++i) is.getline(line);
    if (!is.good()) return;
    int keycol = 0, taxcol = 0;
    {
        std::string header;
        is.getline(header);
        Cursor hs(header);
        std::string w;
        int col = 0;
        hs.word(w);                                                        // "get rid of comment chars"
        while (hs.ok && hs.word(w)) {
            if (w == "taxid") taxcol = col;
            else if (w == "accession.version" || w == "assembly_accession") keycol = col;
            ++col;
        }
    }
    if (taxcol < 1) { is = LineIn{b, e}; taxcol = 1; }
    if (!is.good()) return;
    const std::string rest(is.p, e);
    Cursor c(rest);
    std::string key; int64_t taxid = 0; bool have = false;                 // have: taxonId holds a value that was read
    while (c.good()) {
        for (int i = 0; i < keycol; ++i) c.past('\t');
        if (!c.word(key)) break;                                           // (the pair of the line before once more: nothing)
        for (int i = 0; i < taxcol; ++i) c.past('\t');
        c.ws();
        if (c.p >= c.e) { if (have) map.insert({key, taxid}); break; }     // nothing extracted: taxonId keeps the line before's
        int64_t v = 0;
        if (!c.integer(v)) { map.insert({key, 0}); break; }                // a failed extraction stores 0; the stream is done
        taxid = v; have = true;
        c.past('\n');
        map.insert({key, taxid});
    }
}
int64_t find_taxon_id(const std::map<std::string, int64_t>& m, const std::string& name) {
    if (m.empty() || name.empty()) return 0;
    auto i = m.find(name);
    if (i != m.end()) return i->second;
    i = m.upper_bound(name);
    if (i == m.end()) return 0;
    if (i->first.compare(0, name.size(), name) != 0) return 0;
    return i->second;
}
}  // namespace

extern "C" int mcq_seq2tax_create(mcq_seq2tax** out) {
    if (!out) return fail("null argument");
    *out = new mcq_seq2tax();
    return 0;
}
extern "C" int mcq_seq2tax_add_file(mcq_seq2tax* m, const char* path, int32_t* opened) {
    if (!m || !path) return fail("null argument");
    std::string text;
    const bool ok = slurp(path, text);
    if (opened) *opened = ok ? 1 : 0;
    if (ok) { read_seq2tax_text(text, m->map); m->order.clear(); }
    return 0;
}
extern "C" int mcq_seq2tax_read(const char* const* genome_files, uint32_t n_files, mcq_seq2tax** out) {
    if ((n_files && !genome_files) || !out) return fail("null argument");
    std::set<std::string> dirs;                                            // unique_directories (src/filesys_utility.cpp:79-89)
    for (uint32_t i = 0; i < n_files; ++i) {
        const std::string f = genome_files[i];
        dirs.insert(f.substr(0, f.find_last_of("/\\")));                   // (a name without a separator stands for itself)
    }
    mcq_seq2tax* m = new mcq_seq2tax();
    for (const std::string& d : dirs) mcq_seq2tax_add_file(m, (d + "/assembly_summary.txt").c_str(), nullptr);
    *out = m;
    return 0;
}
extern "C" uint64_t mcq_seq2tax_count(const mcq_seq2tax* m) { return m ? m->map.size() : 0; }
extern "C" int mcq_seq2tax_entry(mcq_seq2tax* m, uint64_t i, const char** key, int64_t* taxid) {
    if (!m || i >= m->map.size()) return fail("no such entry");
    if (m->order.size() != m->map.size()) { m->order.clear(); for (auto it = m->map.cbegin(); it != m->map.cend(); ++it) m->order.push_back(it); }
    if (key) *key = m->order[(size_t)i]->first.c_str();
    if (taxid) *taxid = m->order[(size_t)i]->second;
    return 0;
}
extern "C" int64_t mcq_seq2tax_find(const mcq_seq2tax* m, const char* name, uint64_t len) {
    return (m && name) ? find_taxon_id(m->map, std::string(name, (size_t)len)) : 0;
}
extern "C" int mcq_seq2tax_free(mcq_seq2tax* m) { delete m; return 0; }

extern "C" int mcq_genome_reader_open_mapped(const char* const* files, uint32_t n_files, uint64_t io_bytes, const mcq_refdb* existing,
                                             const mcq_seq2tax* seq2tax, mcq_genome_reader** out) {
    mcq_genome_reader* r = nullptr;
    if (existing ? mcq_genome_reader_open_after(files, n_files, io_bytes, existing, &r) : mcq_genome_reader_open(files, n_files, io_bytes, &r)) return -1;
    if (seq2tax) r->seq2tax = seq2tax->map;
    *out = r;
    return 0;
}
// a target's parent (src/mode_build.cpp:591-604): the map's entry for the sequence id, else for the accession string of the file
// name, else the header's taxid|N
int64_t mcq_genome_reader::parent_of(const std::string& name, const std::string& file) const {
    int64_t parent = find_taxon_id(seq2tax, name);
    if (parent == 0) {
        std::string id;
        if (!file.empty()) { id = accession_version(file); if (id.empty()) id = accession_plain(file); if (id.empty()) id = genbank_id(file); }
        parent = find_taxon_id(seq2tax, id);
    }
    if (parent == 0) parent = header_taxid(header);
    return parent;
}

// ---- post-mapping: the files (get_taxonomy_options, src/args_handling.cpp:122-145) and the reference's parser of one of them
// (rank_targets_with_mapping_file, src/mode_build.cpp:248-312).  The files: -taxpostmap FILE, then nucl_gb / nucl_wgs / nucl_est /
// nucl_gss .accession2taxid of the taxonomy directory (named whether they exist or not), then every other file below it whose path
// contains ".accession2taxid".  DIVERGENCE: those come in name order here, in readdir's order in the reference.  Without a
// taxonomy directory only FILE is named (the reference would look in the working directory).
extern "C" int mcq_taxmap_files(const char* taxdir, const char* postmap, mcq_file_list** out) {
    if (!out) return fail("null argument");
    mcq_file_list* L = new mcq_file_list();
    if (postmap && *postmap) L->files.push_back(postmap);
    std::string path = taxdir ? taxdir : "";
    if (!path.empty()) {
        if (path.back() != '/') path += '/';
        for (const char* n : {"nucl_gb", "nucl_wgs", "nucl_est", "nucl_gss"}) L->files.push_back(path + n + ".accession2taxid");
        std::vector<std::string> more = files_in(path, 10);
        std::sort(more.begin(), more.end());
        for (const std::string& f : more)
            if (f.find(".accession2taxid") != npos && std::find(L->files.begin(), L->files.end(), f) == L->files.end()) L->files.push_back(f);
    }
    *out = L;
    return 0;
}

namespace {
struct NameSet {
    const char* blob; const uint64_t* off; uint64_t n; const uint32_t* target;
    int cmp(uint64_t k, const std::string& s) const {                      // name k against s, as std::string::compare
        const uint64_t b = off[k], nl = off[k + 1] - b;
        const int d = std::memcmp(blob + b, s.data(), (size_t)std::min<uint64_t>(nl, s.size()));
        return d ? d : (nl < s.size() ? -1 : (nl > s.size() ? 1 : 0));
    }
    uint64_t find(const std::string& s) const {                            // taxon_with_name
        if (s.empty()) return n;
        uint64_t lo = 0, hi = n;
        while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (cmp(mid, s) < 0) lo = mid + 1; else hi = mid; }
        return (lo < n && cmp(lo, s) == 0) ? lo : n;
    }
    uint64_t similar(const std::string& s) const {                         // taxon_with_similar_name (src/sketch_database.h:631-639)
        if (s.empty()) return n;
        uint64_t lo = 0, hi = n;
        while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (cmp(mid, s) <= 0) lo = mid + 1; else hi = mid; }
        if (lo >= n) return n;
        const uint64_t b = off[lo], nl = off[lo + 1] - b;
        return (nl >= s.size() && std::memcmp(blob + b, s.data(), s.size()) == 0) ? lo : n;
    }
};
}  // namespace

// `is >> acc >> accver >> taxid >> gi` until an extraction fails: words are separated by any white space and run across lines; taxid
// is a uint64 as num_get reads it (an optional sign -- '-' negates in 64 bits --, then digits up to the first other character, which
// stays in the stream; no digit, or a value beyond 64 bits, fails).
// rule 0: the record's target is the one named accver, else similar to acc, else named gi; rules 1 to 3 (annotate's map,
// src/mode_annotate.cpp:210-217): the name equal to the record's acc / accver / gi word and nothing else.
namespace {
int accmap_host(const char* text, uint64_t n_bytes, int32_t skip_first_line, const char* names_blob, const uint64_t* name_off,
                uint64_t n_names, const uint32_t* name_target, uint8_t* unranked, int64_t* parent, uint32_t n_targets, uint32_t rule,
                uint64_t* n_records, uint64_t* n_consumed, int32_t* stopped) {
    if (rule > 3) return fail("the rule is 0 (targets), 1 (acc), 2 (accver) or 3 (gi)");
    if ((n_bytes && !text) || !name_off || (n_names && (!names_blob || !name_target)) || (n_targets && (!unranked || !parent))) return fail("null argument");
    for (uint64_t k = 0; k < n_names; ++k) if (name_target[k] >= n_targets) return fail("a name's target is outside the targets");
    const NameSet N{names_blob, name_off, n_names, name_target};
    uint64_t left = 0, records = 0;
    for (uint32_t t = 0; t < n_targets; ++t) left += unranked[t] != 0;
    const char* p = text; const char* const e = text + n_bytes;
    if (skip_first_line && p < e) { const char* q = (const char*)std::memchr(p, '\n', (size_t)(e - p)); p = q ? q + 1 : e; }
    auto word = [&](std::string& w) {
        while (p < e && std::isspace((unsigned char)*p)) ++p;
        if (p >= e) return false;
        const char* q = p;
        while (q < e && !std::isspace((unsigned char)*q)) ++q;
        w.assign(p, q); p = q;
        return true;
    };
    std::string acc, accver, gi;
    const char* whole = p;                                                 // behind the last whole record
    bool ran_out = false;                                                  // the text ended inside a record or between two
    while (left) {                                                         // (`if(targetTaxa.empty()) break`)
        if (!word(acc) || !word(accver)) { ran_out = true; break; }
        while (p < e && std::isspace((unsigned char)*p)) ++p;
        if (p >= e) { ran_out = true; break; }
        const char* q = p; bool neg = false;
        if (q < e && (*q == '-' || *q == '+')) { neg = *q == '-'; ++q; }
        if (q >= e || *q < '0' || *q > '9') break;
        uint64_t v = 0; bool over = false;
        for (; q < e && *q >= '0' && *q <= '9'; ++q) {
            const uint64_t d = (uint64_t)(*q - '0');
            if (v > (0xFFFFFFFFFFFFFFFFull - d) / 10) over = true;
            v = v * 10 + d;
        }
        if (over) break;
        if (neg) v = 0 - v;
        p = q;
        if (!word(gi)) { ran_out = true; break; }
        ++records; whole = p;
        uint64_t k;
        if (rule == 0) { k = N.find(accver); if (k == N.n) { k = N.similar(acc); if (k == N.n) k = N.find(gi); } }
        else k = N.find(rule == 1 ? acc : (rule == 2 ? accver : gi));
        if (k != N.n && unranked[name_target[k]]) { unranked[name_target[k]] = 0; parent[name_target[k]] = (int64_t)v; --left; }
    }
    if (n_records) *n_records = records;
    if (n_consumed) *n_consumed = (uint64_t)(whole - text);
    if (stopped) *stopped = ran_out ? 0 : 1;
    return 0;
}
}  // namespace

extern "C" int mcq_accmap_host(const char* text, uint64_t n_bytes, int32_t skip_first_line, const char* names_blob, const uint64_t* name_off,
                               uint64_t n_names, const uint32_t* name_target, uint8_t* unranked, int64_t* parent, uint32_t n_targets,
                               uint64_t* n_records) {
    return accmap_host(text, n_bytes, skip_first_line, names_blob, name_off, n_names, name_target, unranked, parent, n_targets, 0, n_records, nullptr, nullptr);
}
extern "C" int mcq_accmap_host_rule(const char* text, uint64_t n_bytes, int32_t skip_first_line, const char* names_blob, const uint64_t* name_off,
                                    uint64_t n_names, const uint32_t* name_target, uint8_t* unranked, int64_t* parent, uint32_t n_targets,
                                    uint32_t rule, uint64_t* n_records, uint64_t* n_consumed, int32_t* stopped) {
    return accmap_host(text, n_bytes, skip_first_line, names_blob, name_off, n_names, name_target, unranked, parent, n_targets, rule, n_records,
                       n_consumed, stopped);
}

// ---- annotate (src/mode_annotate.cpp:238-311): the id of a header line and the line with its taxid put in ------------------
// The extractors get the WHOLE line, its '>' or '@' included, as annotate_with_taxid calls them: a header without a known prefix
// whose first '.' stands before byte 25 gives an id that begins with that character, which no mapping line names.
extern "C" int64_t mcq_annotate_id(const char* line, uint64_t len, uint32_t id_type, char* buf, size_t cap) {
    if ((len && !line) || (cap && !buf)) return fail("null argument");
    if (id_type < 1 || id_type > 3) return fail("the id type is 1 (acc), 2 (accver) or 3 (gi)");
    const std::string t(line ? line : "", (size_t)len);
    const std::string s = id_type == 1 ? accession_plain(t) : (id_type == 2 ? accession_version(t) : genbank_id(t));
    if (cap) { const size_t n = std::min(cap - 1, s.size()); std::memcpy(buf, s.data(), n); buf[n] = 0; }
    return (int64_t)s.size();
}
// :265-298.  The old taxid: from "taxid" through the field separator found behind the value separator (which is looked for 4 bytes
// into "taxid"), else through the next value separator, else to the end of the line; without a value separator nothing is cut.
// The new one goes ONE byte behind the first field separator's first byte, however long the separator is.
extern "C" int64_t mcq_annotate_rewrite(const char* line, uint64_t len, int32_t has_id, uint64_t taxid, const char* field_sep,
                                        const char* value_sep, char* buf, size_t cap) {
    if ((len && !line) || (cap && !buf) || !field_sep || !value_sep) return fail("null argument");
    if (!*field_sep || !*value_sep) return fail("the separators must not be empty");
    std::string t(line ? line : "", (size_t)len);
    const std::string fs = field_sep, vs = value_sep;
    const size_t j = t.find("taxid");
    if (j != npos) {
        const size_t k = t.find(vs, j + 4);
        if (k != npos) {
            size_t l = t.find(fs, k + 1);
            if (l == npos) l = t.find(vs, k + 1);
            t.erase(j, l - j + 1);                                         // (l == npos: npos - j + 1 wraps to "the rest", j >= 1 in a header)
        }
    }
    if (has_id) {
        const std::string ins = "taxid" + vs + std::to_string((unsigned long long)taxid) + fs;
        const size_t ipos = t.find(fs);
        if (ipos == npos) t += fs + ins; else t.insert(ipos + 1, ins);
    }
    if (cap) { const size_t n = std::min(cap - 1, t.size()); std::memcpy(buf, t.data(), n); buf[n] = 0; }
    return (int64_t)t.size();
}
