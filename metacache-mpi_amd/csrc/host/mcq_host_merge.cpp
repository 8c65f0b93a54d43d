// mcq_host_merge.cpp -- the host side of merging query result files (include/mcq_host.h): the header scan of a results file
// (get_results_file_properties, src/mode_merge.cpp:131-200) and the reference's token-stream parser of its mapping lines
// (read_results, src/mode_merge.cpp:209-264) restated over a buffer -- the fall-back of mcq_merge_chunk (include/mcq.h) for text
// that is not strict, and the CPU yardstick.  Plain C++14, no GPU.
#include "../../../include/mcq_host.h"
#include "mcq_host_internal.hpp"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <limits>
#include <sstream>
#include <string>

namespace {

int fail(const std::string& m) { return mcq_host_set_error(m.c_str()); }
inline bool blank(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\v' || c == '\f' || c == '\r'; }

// operator>> of an unsigned / a signed 64-bit integer as num_get reads it: white space skipped, an optional sign ('-' negates,
// for an unsigned one in 64 bits), digits up to the first other character; no digit or a value out of range fails
bool number(const char*& p, const char* e, bool is_signed, uint64_t& out) {
    while (p < e && blank(*p)) ++p;
    const char* q = p;
    bool neg = false;
    if (q < e && (*q == '-' || *q == '+')) { neg = *q == '-'; ++q; }
    if (q >= e || *q < '0' || *q > '9') return false;
    uint64_t v = 0;
    bool over = false;
    for (; q < e && *q >= '0' && *q <= '9'; ++q) {
        const uint64_t d = (uint64_t)(*q - '0');
        if (v > (0xFFFFFFFFFFFFFFFFull - d) / 10) over = true;
        v = v * 10 + d;
    }
    if (over) return false;
    if (is_signed && v > (neg ? 0x8000000000000000ull : 0x7FFFFFFFFFFFFFFFull)) return false;
    out = neg ? 0 - v : v;
    p = q;
    return true;
}
// ignore(max, c): behind the next c; false (the stream is at its end) if there is none
bool past(const char*& p, const char* e, char c) {
    const void* q = p < e ? std::memchr(p, c, (size_t)(e - p)) : nullptr;
    p = q ? (const char*)q + 1 : e;
    return q != nullptr;
}

}  // namespace

extern "C" int mcq_results_properties(const char* path, uint32_t* tophits_column, uint64_t* results_begin, uint64_t* n_lines) {
    if (!path || !tophits_column || !results_begin || !n_lines) return fail("null argument");
    const std::string name(path);
    std::ifstream ifs(name, std::ios::binary);
    if (!ifs.good()) return fail("could not open file " + name);
    std::string line;
    for (;;) {                                                   // the classification ranks
        if (!std::getline(ifs, line) || line.empty() || line[0] != '#') return fail("classification ranks not found in file " + name);
        if (line.compare(0, 16, "# Classification") == 0) {
            if (line.find("sequence") != std::string::npos) return fail("cannot merge results on sequence level: file " + name);
            break;
        }
    }
    uint32_t column = 0;
    for (;;) {                                                   // the layout
        if (!std::getline(ifs, line) || line.empty() || line[0] != '#') return fail("TABLE_LAYOUT not found in file " + name);
        if (line.compare(0, 15, "# TABLE_LAYOUT:") == 0) {
            std::stringstream ls(line.substr(15));
            std::string col;
            ls >> col;
            if (col != "query_id") return fail("no query_id in file " + name);
            uint32_t c = 0;
            while (ls.good()) {
                ls.ignore(std::numeric_limits<std::streamsize>::max(), '|');
                col.clear();
                ls >> col;
                ++c;
                if (col == "top_hits") { column = c; break; }
            }
            break;
        }
    }
    if (column < 1) return fail("no top_hits in file " + name);
    if (column < 2) return fail("top_hits in front of the query header in file " + name);
    // the results begin at the first line that is no comment; every such line from there on counts
    uint64_t pos = ifs.eof() ? 0 : (uint64_t)ifs.tellg(), begin = 0, count = 0;
    bool at_line_start = true, begun = false;
    if (ifs.eof()) { ifs.clear(); ifs.seekg(0, std::ios::end); pos = (uint64_t)ifs.tellg(); }
    std::string buf(1 << 20, '\0');
    while (ifs.good()) {
        ifs.read(&buf[0], (std::streamsize)buf.size());
        const size_t got = (size_t)ifs.gcount();
        for (size_t i = 0; i < got; ++i) {
            if (at_line_start && buf[i] != '#') {
                if (!begun) { begun = true; begin = pos + i; }
                ++count;
            }
            at_line_start = buf[i] == '\n';
        }
        pos += got;
    }
    *tophits_column = column;
    *results_begin = begun ? begin : pos;
    *n_lines = count;
    return 0;
}

extern "C" int mcq_merge_host(const char* text, uint64_t n_bytes, uint32_t tophits_column, uint64_t n_queries, const char* file_name,
                              uint64_t first_line_no, uint64_t text_offset, uint32_t* line_query, uint64_t* item_off, int64_t* taxid,
                              uint32_t* hits, uint64_t* header_off, uint32_t* header_len, uint64_t line_cap, uint64_t item_cap,
                              uint64_t* n_lines, uint64_t* n_items) {
    if ((n_bytes && !text) || !item_off || !n_lines || !n_items || (line_cap && (!line_query || !header_off || !header_len)) ||
        (item_cap && (!taxid || !hits))) return fail("null argument");
    if (tophits_column < 2) return fail("top_hits is column 2 or later");
    const std::string file = file_name ? file_name : "";
    const char* p = text;
    const char* const e = text + n_bytes;
    uint64_t lines = 0, items = 0;
    auto stop = [&](const char* at, const std::string& why) {          // (once per call: the line of `at` is counted from the start)
        uint64_t line_no = first_line_no;
        for (const char* q = text; q < at && q < e; ++q) line_no += *q == '\n';
        return fail(file + ": line " + std::to_string(line_no) + ": " + why);
    };
    item_off[0] = 0;
    while (p < e) {
        const char* const rec = p;
        if (*p != '#') {
            uint64_t id = 0;
            if (!number(p, e, false, id)) return stop(rec, "no query id (the reference does not return from this line)");
            const char* const at = p;                            // (behind white space the id may stand in a later line)
            if (id == 0) return stop(at, "query id 0");
            if (id > n_queries) return stop(at, "query id " + std::to_string(id) + " beyond the " + std::to_string(n_queries) + " queries of the file");
            if (!past(p, e, '|')) return stop(at, "no column separator behind the query id");
            while (p < e && blank(*p)) ++p;
            const char* const hb = p;
            while (p < e && !blank(*p)) ++p;
            if (p == hb || p >= e) return stop(at, "the line ends in the query header");
            if (std::memchr(hb, '|', (size_t)(p - hb))) return stop(at, "a '|' in the query header (the reference reads such a line differently once it knows the header)");
            for (uint32_t c = 1; c < tophits_column; ++c)
                if (!past(p, e, '|')) return stop(at, "fewer columns than the layout names");
            if (!past(p, e, '\t') || p >= e) return stop(at, "no top_hits column");
            if (lines >= line_cap) return fail("mcq_merge_host: more lines than line_cap");
            char next = *p;
            while (next != '\t') {
                uint64_t t = 0, h = 0;
                if (!number(p, e, true, t) || p >= e) return stop(at, "a top_hits item that is not taxid:hits (the reference does not return from this line)");
                if (!past(p, e, ':')) return stop(at, "a top_hits item without ':'");
                if (!number(p, e, false, h) || p >= e) return stop(at, "a top_hits item without hits, with hits beyond 64 bits, or at the end of the text (the reference does not return from this line)");
                if (h > 0xFFFFFFFFull) return stop(at, "hits of 2^32 or more");
                if (items >= item_cap) return fail("mcq_merge_host: more items than item_cap");
                taxid[items] = (int64_t)t; hits[items] = (uint32_t)h; ++items;
                next = *p++;
            }
            line_query[lines] = (uint32_t)(id - 1);
            header_off[lines] = text_offset + (uint64_t)(hb - text);
            const char* he = hb;
            while (he < e && !blank(*he)) ++he;
            header_len[lines] = (uint32_t)(he - hb);
            ++lines;
            item_off[lines] = items;
        }
        past(p, e, '\n');
    }
    *n_lines = lines; *n_items = items;
    return 0;
}
