// mcq_host.cpp -- host companions of the engine: reference shard reader, taxonomy keys,
// classification (include/mcq_host.h).  Plain C++14, no GPU, no MPI.
#include "../../../include/mcq_host.h"
#include "mcq_host_internal.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>

namespace {

thread_local std::string g_err;
int fail(const std::string& m) { g_err = m; return -1; }

const uint64_t kDbVersion = 20181001;      // MC_DB_VERSION
const int kNumRanks = 21;                  // taxonomy::num_ranks; rank::root == 20, rank::none == 21

struct Taxon { int64_t id, parent; uint8_t rank; std::string name, file; uint64_t index, windows; };

struct Reader {
    std::vector<unsigned char> buf; size_t pos = 0; bool ok = true;
    template <class T> T get() {
        T v{};
        if (pos + sizeof(T) > buf.size()) { ok = false; return v; }
        std::memcpy(&v, buf.data() + pos, sizeof(T)); pos += sizeof(T);
        return v;
    }
    std::string str() {                     // u64 length + bytes (src/io_serialize.h:48-55)
        uint64_t n = get<uint64_t>();
        if (!ok || pos + n > buf.size()) { ok = false; return ""; }
        std::string s((const char*)buf.data() + pos, n); pos += n;
        return s;
    }
};

}  // namespace

struct mcq_refdb {
    mcq_refdb_info info{};
    std::vector<Taxon> taxa;
    std::unordered_map<int64_t, uint32_t> by_id;
    std::vector<uint32_t> lineage;          // n_taxa x 21, taxon indices or MCQ_NO_TAXON
    std::map<std::string, uint32_t> seq_names;   // name2tax_ (src/sketch_database.h:938-943): names of the sequence-level taxa, the first of a name stays
    std::vector<uint32_t> keys; std::vector<uint64_t> off, locs;
    // mcq_refdb_open_meta: no table in host memory; per shard file where its key records begin, how many there are
    std::string prefix;
    std::vector<uint64_t> table_pos, table_keys, table_locs, file_bytes;
    std::vector<uint32_t> tgt_windows;      // windows of every target, from the rank that owns it
    std::vector<uint64_t> seq_windows;      // the same, kept by both openers: windows_in_sequence of the -hits-per-seq table
};

namespace {
// sequential reader of one file through a fixed buffer (the streaming route never holds a shard file in memory)
struct FileReader {
    FILE* f = nullptr; std::vector<unsigned char> buf; size_t pos = 0, end = 0; bool ok = true; uint64_t consumed = 0;
    explicit FileReader(size_t cap = 1u << 22) : buf(cap) {}
    ~FileReader() { if (f) std::fclose(f); }
    bool open(const std::string& path) { f = std::fopen(path.c_str(), "rb"); return f != nullptr; }
    bool seek(uint64_t at) { pos = end = 0; consumed = at; return std::fseek(f, (long)at, SEEK_SET) == 0; }
    bool fill(size_t need) {                 // makes `need` bytes available at buf[pos..)
        if (end - pos >= need) return true;
        if (need > buf.size()) buf.resize(need);
        std::memmove(buf.data(), buf.data() + pos, end - pos); end -= pos; pos = 0;
        while (end < need) {
            const size_t n = std::fread(buf.data() + end, 1, buf.size() - end, f);
            if (n == 0) return false;
            end += n;
        }
        return true;
    }
    template <class T> T get() {
        T v{};
        if (!ok || !fill(sizeof(T))) { ok = false; return v; }
        std::memcpy(&v, buf.data() + pos, sizeof(T)); pos += sizeof(T); consumed += sizeof(T);
        return v;
    }
    const unsigned char* bytes(size_t n) {   // n bytes in place (valid until the next call)
        if (!ok || !fill(n)) { ok = false; return nullptr; }
        const unsigned char* p = buf.data() + pos; pos += n; consumed += n;
        return p;
    }
    std::string str() {
        const uint64_t n = get<uint64_t>();
        if (!ok || n > (1u << 24)) { ok = false; return ""; }
        const unsigned char* p = bytes((size_t)n);
        return p ? std::string((const char*)p, (size_t)n) : std::string();
    }
};
void build_lineages(mcq_refdb* db) {
    // ranked lineages: walk the parents, record every ranked ancestor (incl. the taxon itself)
    // at lineage[rank] (taxonomy::ranks, src/taxonomy.h:576-597)
    for (uint32_t i = 0; i < db->taxa.size(); ++i) db->by_id[db->taxa[i].id] = i;
    db->lineage.assign((size_t)db->taxa.size() * kNumRanks, MCQ_NO_TAXON);
    for (uint32_t i = 0; i < db->taxa.size(); ++i) {
        int64_t cur = db->taxa[i].id;
        while (cur != 0) {
            auto it = db->by_id.find(cur);
            if (it == db->by_id.end()) break;
            const Taxon& t = db->taxa[it->second];
            if (t.rank < kNumRanks) db->lineage[(size_t)i * kNumRanks + t.rank] = it->second;
            cur = (t.parent != cur) ? t.parent : 0;
        }
    }
    for (uint32_t i = 0; i < db->taxa.size(); ++i)
        if (db->taxa[i].rank == MCQ_RANK_SEQUENCE) db->seq_names.insert({db->taxa[i].name, i});
}
}  // namespace

static bool read_file(const std::string& path, std::vector<unsigned char>& out) {
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END); long n = std::ftell(f); std::fseek(f, 0, SEEK_SET);
    out.resize((size_t)n);
    bool ok = n == 0 || std::fread(out.data(), 1, (size_t)n, f) == (size_t)n;
    std::fclose(f);
    return ok;
}

extern "C" const char* mcq_host_last_error(void) { return g_err.c_str(); }
int mcq_host_set_error(const char* text) { return fail(text ? text : ""); }

extern "C" int mcq_refdb_open(const char* prefix, uint32_t n_ranks, mcq_refdb** out) {
    if (!prefix || !out || n_ranks < 1) return fail("bad argument");
    mcq_refdb* db = new mcq_refdb();
    // (key, location) pairs of all shards; the union list of a key is the multiset union of
    // the per-rank lists, each target living on exactly one rank (src/sketch_database.h:540)
    std::vector<std::pair<uint32_t, uint64_t>> all;
    for (uint32_t r = 0; r < n_ranks; ++r) {
        Reader rd;
        const std::string path = std::string(prefix) + ".db_" + std::to_string(r);
        if (!read_file(path, rd.buf)) { delete db; return fail("can't open file " + path); }
        if (rd.get<uint64_t>() != kDbVersion) { delete db; return fail("Database " + path + " is incompatible (version)"); }
        uint8_t w[6]; for (auto& x : w) x = rd.get<uint8_t>();
        if (w[0] != 4 || w[1] != 4 || w[2] != 4 || w[3] != 1 || w[4] != 8 || w[5] != kNumRanks) {
            delete db; return fail("Database " + path + " is incompatible due to different data type sizes");
        }
        uint64_t p[9]; for (auto& x : p) x = rd.get<uint64_t>();
        const uint64_t ntaxa = rd.get<uint64_t>();
        std::vector<Taxon> taxa; taxa.reserve(ntaxa);
        for (uint64_t i = 0; i < ntaxa && rd.ok; ++i) {
            Taxon t; t.id = rd.get<int64_t>(); t.parent = rd.get<int64_t>(); t.rank = rd.get<uint8_t>();
            t.name = rd.str(); t.file = rd.str(); t.index = rd.get<uint64_t>(); t.windows = rd.get<uint64_t>();
            taxa.push_back(std::move(t));
        }
        const uint32_t ntargets = rd.get<uint32_t>();
        if (r == 0) db->seq_windows.assign(ntargets, 0);
        for (const Taxon& t : taxa)          // (`windows` is non-zero only on the rank that owns the target, src/taxonomy.h:326-335)
            if (t.id < 0 && (uint64_t)(-t.id - 1) < db->seq_windows.size() && t.windows) db->seq_windows[(size_t)(-t.id - 1)] = t.windows;
        if (r == 0) {
            db->info.k = (uint32_t)p[0]; db->info.sketch_size = (uint32_t)p[1]; db->info.winlen = (uint32_t)p[2];
            db->info.winstride = (uint32_t)p[3]; db->info.q_sketch_size = (uint32_t)p[5]; db->info.q_winlen = (uint32_t)p[6];
            db->info.q_winstride = (uint32_t)p[7]; db->info.max_locs_per_feature = (uint32_t)p[8];
            db->info.n_targets = ntargets; db->info.n_taxa = (uint32_t)ntaxa; db->info.n_ranks = n_ranks;
            db->taxa = std::move(taxa);
        } else if (ntargets != db->info.n_targets || ntaxa != db->info.n_taxa) {
            delete db; return fail("shard " + path + " does not belong to the same database");
        }
        if (ntargets >= 1) {
            const uint64_t nkeys = rd.get<uint64_t>(); rd.get<uint64_t>();
            for (uint64_t i = 0; i < nkeys && rd.ok; ++i) {
                const uint32_t key = rd.get<uint32_t>(); const uint8_t n = rd.get<uint8_t>();
                if (n == 0) continue;
                const uint64_t n1 = rd.get<uint64_t>(); const size_t tpos = rd.pos; rd.pos += 4 * n1;
                const uint64_t n2 = rd.get<uint64_t>(); const size_t wpos = rd.pos; rd.pos += 4 * n2;
                if (n1 != n || n2 != n || rd.pos > rd.buf.size()) { rd.ok = false; break; }
                for (uint32_t j = 0; j < n; ++j) {
                    uint32_t t, wi; std::memcpy(&t, rd.buf.data() + tpos + 4 * j, 4); std::memcpy(&wi, rd.buf.data() + wpos + 4 * j, 4);
                    all.emplace_back(key, ((uint64_t)t << 32) | wi);
                }
            }
        }
        if (!rd.ok) { delete db; return fail("Database " + path + " is truncated or corrupt"); }
    }
    std::sort(all.begin(), all.end());
    db->off.push_back(0);
    for (size_t i = 0; i < all.size(); ++i) {
        if (i == 0 || all[i].first != all[i - 1].first) { if (i) db->off.push_back(i); db->keys.push_back(all[i].first); }
        db->locs.push_back(all[i].second);
    }
    if (!all.empty()) db->off.push_back(all.size());
    db->info.n_keys = db->keys.size(); db->info.n_locs = db->locs.size();
    build_lineages(db);
    *out = db;
    return 0;
}

extern "C" int mcq_refdb_close(mcq_refdb* db) { delete db; return 0; }

// ---- the streaming route (r04): shard files of any size without a host-side union ------------------------------------------
// mcq_refdb_open (above) materialises every (key, location) of all P shards in one host vector and sorts it: 16 B per location,
// 240 GB and minutes for a RefSeq-scale database.  The streaming route reads only the head of every file here (parameters,
// taxa, target count: what classify and the taxon keys need), and hands the key records out in chunks of (feature, target,
// window) triples in file order; the consumer (mcq_parts_builder_*, include/mcq.h) turns them into global-window words on the
// GPU, merges the ranks per feature-hash range there and makes the table parts.  Host memory: one read buffer + one chunk.
extern "C" int mcq_refdb_open_meta(const char* prefix, uint32_t n_ranks, mcq_refdb** out) {
    if (!prefix || !out || n_ranks < 1) return fail("bad argument");
    mcq_refdb* db = new mcq_refdb();
    db->prefix = prefix;
    for (uint32_t r = 0; r < n_ranks; ++r) {
        const std::string path = std::string(prefix) + ".db_" + std::to_string(r);
        FileReader rd;
        if (!rd.open(path)) { delete db; return fail("can't open file " + path); }
        if (rd.get<uint64_t>() != kDbVersion) { delete db; return fail("Database " + path + " is incompatible (version)"); }
        uint8_t w[6]; for (auto& x : w) x = rd.get<uint8_t>();
        if (w[0] != 4 || w[1] != 4 || w[2] != 4 || w[3] != 1 || w[4] != 8 || w[5] != kNumRanks) {
            delete db; return fail("Database " + path + " is incompatible due to different data type sizes");
        }
        uint64_t p[9]; for (auto& x : p) x = rd.get<uint64_t>();
        const uint64_t ntaxa = rd.get<uint64_t>();
        std::vector<Taxon> taxa;
        for (uint64_t i = 0; i < ntaxa && rd.ok; ++i) {
            Taxon t; t.id = rd.get<int64_t>(); t.parent = rd.get<int64_t>(); t.rank = rd.get<uint8_t>();
            t.name = rd.str(); t.file = rd.str(); t.index = rd.get<uint64_t>(); t.windows = rd.get<uint64_t>();
            taxa.push_back(std::move(t));
        }
        const uint32_t ntargets = rd.get<uint32_t>();
        if (!rd.ok) { delete db; return fail("Database " + path + " is truncated or corrupt"); }
        if (r == 0) {
            db->info.k = (uint32_t)p[0]; db->info.sketch_size = (uint32_t)p[1]; db->info.winlen = (uint32_t)p[2];
            db->info.winstride = (uint32_t)p[3]; db->info.q_sketch_size = (uint32_t)p[5]; db->info.q_winlen = (uint32_t)p[6];
            db->info.q_winstride = (uint32_t)p[7]; db->info.max_locs_per_feature = (uint32_t)p[8];
            db->info.n_targets = ntargets; db->info.n_taxa = (uint32_t)ntaxa; db->info.n_ranks = n_ranks;
            db->tgt_windows.assign(ntargets, 0); db->seq_windows.assign(ntargets, 0);
        } else if (ntargets != db->info.n_targets || ntaxa != db->info.n_taxa) {
            delete db; return fail("shard " + path + " does not belong to the same database");
        }
        // windows of the targets this rank owns (`windows` is non-zero only there, src/taxonomy.h:326-335)
        for (const Taxon& t : taxa)
            if (t.id < 0 && (uint64_t)(-t.id - 1) < ntargets && t.windows) {
                if (t.windows >= (1ull << 32)) { delete db; return fail("a target with 2^32 windows or more"); }
                db->tgt_windows[(size_t)(-t.id - 1)] = (uint32_t)t.windows;
                db->seq_windows[(size_t)(-t.id - 1)] = t.windows;
            }
        if (r == 0) db->taxa = std::move(taxa);
        uint64_t nkeys = 0, nlocs = 0;
        if (ntargets >= 1) { nkeys = rd.get<uint64_t>(); nlocs = rd.get<uint64_t>(); }
        if (!rd.ok) { delete db; return fail("Database " + path + " is truncated or corrupt"); }
        db->table_pos.push_back(rd.consumed); db->table_keys.push_back(nkeys); db->table_locs.push_back(nlocs);
        std::fseek(rd.f, 0, SEEK_END);
        db->file_bytes.push_back((uint64_t)std::ftell(rd.f));
        db->info.n_locs += nlocs;            // (n_keys of the union is not known without reading the tables: left 0)
    }
    build_lineages(db);
    *out = db;
    return 0;
}
extern "C" int mcq_refdb_tgt_windows(const mcq_refdb* db, uint32_t* out) {
    if (!db || !out) return fail("bad argument");
    if (db->tgt_windows.size() != db->info.n_targets) return fail("the handle was not opened with mcq_refdb_open_meta");
    std::memcpy(out, db->tgt_windows.data(), db->tgt_windows.size() * 4);
    return 0;
}
extern "C" int mcq_refdb_file_stats(const mcq_refdb* db, uint32_t rank, uint64_t* bytes, uint64_t* n_keys, uint64_t* n_locs) {
    if (!db || rank >= db->table_pos.size()) return fail("bad argument");
    if (bytes) *bytes = db->file_bytes[rank];
    if (n_keys) *n_keys = db->table_keys[rank];
    if (n_locs) *n_locs = db->table_locs[rank];
    return 0;
}

struct mcq_shard_stream {
    FileReader rd{1u << 24};
    uint64_t keys_left = 0;
};
extern "C" int mcq_shard_stream_open(const mcq_refdb* db, uint32_t rank, mcq_shard_stream** out) {
    if (!db || !out || rank >= db->table_pos.size()) return fail("bad argument (the handle must come from mcq_refdb_open_meta)");
    mcq_shard_stream* s = new mcq_shard_stream();
    const std::string path = db->prefix + ".db_" + std::to_string(rank);
    if (!s->rd.open(path) || !s->rd.seek(db->table_pos[rank])) { delete s; return fail("can't open file " + path); }
    s->keys_left = db->table_keys[rank];
    *out = s;
    return 0;
}
extern "C" int mcq_shard_stream_next(mcq_shard_stream* s, uint32_t* feat, uint32_t* tgt, uint32_t* win, uint64_t cap, uint64_t* n_out) {
    if (!s || !feat || !tgt || !win || !n_out || cap < 255) return fail("bad argument (a chunk holds at least 255 locations)");
    uint64_t n = 0;
    while (s->keys_left && n + 255 <= cap) {                     // (whole key records only: a list has at most 255 entries)
        const uint32_t key = s->rd.get<uint32_t>(); const uint8_t cnt = s->rd.get<uint8_t>();
        --s->keys_left;
        if (!s->rd.ok) return fail("shard file is truncated or corrupt");
        if (cnt == 0) continue;                                  // (an empty bucket is written without its columns)
        const uint64_t n1 = s->rd.get<uint64_t>();
        if (!s->rd.ok || n1 != cnt) return fail("shard file is truncated or corrupt");
        const unsigned char* tp = s->rd.bytes(4 * (size_t)cnt);
        if (!tp) return fail("shard file is truncated or corrupt");
        std::memcpy(tgt + n, tp, 4 * (size_t)cnt);
        const uint64_t n2 = s->rd.get<uint64_t>();
        if (!s->rd.ok || n2 != cnt) return fail("shard file is truncated or corrupt");
        const unsigned char* wp = s->rd.bytes(4 * (size_t)cnt);
        if (!wp) return fail("shard file is truncated or corrupt");
        std::memcpy(win + n, wp, 4 * (size_t)cnt);
        for (uint32_t j = 0; j < cnt; ++j) feat[n + j] = key;
        n += cnt;
    }
    *n_out = n;
    return 0;
}
extern "C" int mcq_shard_stream_close(mcq_shard_stream* s) { delete s; return 0; }

// ---- shard writer: the exact inverse of the reader above
namespace {
struct Writer {
    FILE* f; bool ok = true;
    template <class T> void put(T v) { if (ok && std::fwrite(&v, sizeof(T), 1, f) != 1) ok = false; }
    void str(const char* s) {
        const uint64_t n = s ? std::strlen(s) : 0;
        put<uint64_t>(n);
        if (ok && n && std::fwrite(s, 1, n, f) != n) ok = false;
    }
};
// what a shard file holds in front of its table: version, type widths, sketch parameters, taxon list, target count
void write_head(Writer& w, const mcq_shard_params* p, const mcq_taxon_rec* taxa, uint64_t n_taxa, uint32_t n_targets) {
    w.put<uint64_t>(kDbVersion);
    const uint8_t widths[6] = {4, 4, 4, 1, 8, (uint8_t)kNumRanks};
    for (uint8_t x : widths) w.put<uint8_t>(x);
    const uint64_t pv[9] = {p->k, p->sketch_size, p->winlen, p->winstride, p->q_k, p->q_sketch_size, p->q_winlen, p->q_winstride,
                            p->max_locs_per_feature};
    for (uint64_t x : pv) w.put<uint64_t>(x);
    w.put<uint64_t>(n_taxa);
    for (uint64_t i = 0; i < n_taxa; ++i) {
        w.put<int64_t>(taxa[i].id); w.put<int64_t>(taxa[i].parent); w.put<uint8_t>(taxa[i].rank);
        w.str(taxa[i].name); w.str(taxa[i].file);
        w.put<uint64_t>(taxa[i].index); w.put<uint64_t>(taxa[i].windows);
    }
    w.put<uint32_t>(n_targets);
}
}  // namespace

// ---- the same file written in blocks: the head and two zero counts, key records as the caller has them (mcq_table_shard_records of
// include/mcq.h makes them on the GPU), the counts patched in at the end
struct mcq_shard_writer {
    Writer w; std::string path;
    long counts_pos = -1;                // where the two counts stand; -1: a file without targets has none
    uint64_t n_keys = 0, n_locs = 0;
};
extern "C" int mcq_shard_writer_open(const char* path, const mcq_shard_params* p, const mcq_taxon_rec* taxa, uint64_t n_taxa,
                                     uint32_t n_targets, mcq_shard_writer** out) {
    if (!path || !p || (n_taxa && !taxa) || !out) return fail("bad argument");
    FILE* f = std::fopen(path, "wb");
    if (!f) return fail(std::string("can't open file ") + path);
    mcq_shard_writer* s = new mcq_shard_writer();
    s->w.f = f; s->path = path;
    write_head(s->w, p, taxa, n_taxa, n_targets);
    if (n_targets >= 1) {
        s->counts_pos = std::ftell(f);
        s->w.put<uint64_t>(0); s->w.put<uint64_t>(0);
    }
    if (!s->w.ok || (n_targets >= 1 && s->counts_pos < 0)) { std::fclose(f); delete s; return fail(std::string("write error on ") + path); }
    *out = s;
    return 0;
}
extern "C" int mcq_shard_writer_append(mcq_shard_writer* s, const void* records, uint64_t n_bytes, uint64_t n_keys, uint64_t n_locs) {
    if (!s || (n_bytes && !records)) return fail("bad argument");
    if (n_bytes != 21 * n_keys + 8 * n_locs) return fail("key records of n_keys keys and n_locs locations take 21 n_keys + 8 n_locs bytes");
    if (n_bytes && s->counts_pos < 0) return fail("a shard file without targets holds no key records");
    if (s->w.ok && n_bytes && std::fwrite(records, 1, n_bytes, s->w.f) != n_bytes) s->w.ok = false;
    if (!s->w.ok) return fail("write error on " + s->path);
    s->n_keys += n_keys; s->n_locs += n_locs;
    return 0;
}
extern "C" int mcq_shard_writer_close(mcq_shard_writer* s) {
    if (!s) return 0;
    if (s->w.ok && s->counts_pos >= 0) {
        if (std::fseek(s->w.f, s->counts_pos, SEEK_SET) != 0) s->w.ok = false;
        s->w.put<uint64_t>(s->n_keys); s->w.put<uint64_t>(s->n_locs);
    }
    const bool ok = (std::fclose(s->w.f) == 0) && s->w.ok;
    const std::string path = s->path;
    delete s;
    return ok ? 0 : fail("write error on " + path);
}

extern "C" int mcq_refdb_write_shard(const char* path, const mcq_shard_params* p, const mcq_taxon_rec* taxa, uint64_t n_taxa,
                                     uint32_t n_targets, const uint32_t* keys, const uint64_t* list_off, const uint64_t* locs,
                                     uint64_t n_keys) {
    if (!path || !p || (n_taxa && !taxa) || (n_keys && (!keys || !list_off || !locs))) return fail("bad argument");
    for (uint64_t i = 0; i < n_keys; ++i)
        if (list_off[i + 1] < list_off[i] || list_off[i + 1] - list_off[i] > 255)
            return fail("a list has more than 255 locations (bucket size type is uint8, src/config.h:77)");
    Writer w; w.f = std::fopen(path, "wb");
    if (!w.f) return fail(std::string("can't open file ") + path);
    write_head(w, p, taxa, n_taxa, n_targets);
    if (n_targets >= 1) {
        uint64_t nonempty = 0;
        for (uint64_t i = 0; i < n_keys; ++i) nonempty += list_off[i + 1] > list_off[i];
        w.put<uint64_t>(nonempty);
        w.put<uint64_t>(n_keys ? list_off[n_keys] - list_off[0] : 0);
        std::vector<uint32_t> col;
        for (uint64_t i = 0; i < n_keys; ++i) {
            const uint64_t b = list_off[i], n = list_off[i + 1] - b;
            if (n == 0) continue;
            w.put<uint32_t>(keys[i]); w.put<uint8_t>((uint8_t)n);
            col.resize(n);
            w.put<uint64_t>(n);
            for (uint64_t j = 0; j < n; ++j) col[j] = (uint32_t)(locs[b + j] >> 32);
            if (w.ok && std::fwrite(col.data(), 4, n, w.f) != n) w.ok = false;
            w.put<uint64_t>(n);
            for (uint64_t j = 0; j < n; ++j) col[j] = (uint32_t)locs[b + j];
            if (w.ok && std::fwrite(col.data(), 4, n, w.f) != n) w.ok = false;
        }
    }
    const bool ok = w.ok;
    if (std::fclose(w.f) != 0 || !ok) return fail(std::string("write error on ") + path);
    return 0;
}
extern "C" int mcq_refdb_get_info(const mcq_refdb* db, mcq_refdb_info* out) { if (!db || !out) return fail("bad argument"); *out = db->info; return 0; }
extern "C" const uint32_t* mcq_refdb_keys(const mcq_refdb* db) { return db->keys.data(); }
extern "C" const uint64_t* mcq_refdb_list_off(const mcq_refdb* db) { return db->off.empty() ? nullptr : db->off.data(); }
extern "C" const uint64_t* mcq_refdb_locs(const mcq_refdb* db) { return db->locs.data(); }

extern "C" int mcq_refdb_tgt2tax(const mcq_refdb* db, uint32_t merge_below_rank, uint32_t* out) {
    if (!db || !out) return fail("bad argument");
    for (uint32_t t = 0; t < db->info.n_targets; ++t) {
        auto it = db->by_id.find(-(int64_t)t - 1);              // taxon_id_of_target (src/sketch_database.h:149-150)
        if (it == db->by_id.end()) return fail("target " + std::to_string(t) + " has no sequence-level taxon");
        uint32_t a = (merge_below_rank > 0 && merge_below_rank < (uint32_t)kNumRanks)
                         ? db->lineage[(size_t)it->second * kNumRanks + merge_below_rank] : MCQ_NO_TAXON;
        out[t] = (a != MCQ_NO_TAXON) ? a : (0x80000000u | it->second);
    }
    return 0;
}

static inline bool valid_key(const mcq_refdb* db, uint32_t key) { return key != MCQ_NO_TAXON && (key & 0x7FFFFFFFu) < db->taxa.size(); }
extern "C" int64_t mcq_refdb_taxon_id(const mcq_refdb* db, uint32_t key) { return valid_key(db, key) ? db->taxa[key & 0x7FFFFFFFu].id : 0; }
extern "C" uint32_t mcq_refdb_taxon_rank(const mcq_refdb* db, uint32_t key) { return valid_key(db, key) ? db->taxa[key & 0x7FFFFFFFu].rank : MCQ_RANK_NONE; }
extern "C" const char* mcq_refdb_taxon_name(const mcq_refdb* db, uint32_t key) { return valid_key(db, key) ? db->taxa[key & 0x7FFFFFFFu].name.c_str() : "--"; }
extern "C" int64_t mcq_refdb_taxon_parent(const mcq_refdb* db, uint32_t key) { return valid_key(db, key) ? db->taxa[key & 0x7FFFFFFFu].parent : 0; }
extern "C" const char* mcq_refdb_taxon_file(const mcq_refdb* db, uint32_t key) { return valid_key(db, key) ? db->taxa[key & 0x7FFFFFFFu].file.c_str() : ""; }
extern "C" uint64_t mcq_refdb_taxon_index(const mcq_refdb* db, uint32_t key) { return valid_key(db, key) ? db->taxa[key & 0x7FFFFFFFu].index : 0; }
extern "C" uint64_t mcq_refdb_taxon_windows(const mcq_refdb* db, uint32_t key) { return valid_key(db, key) ? db->taxa[key & 0x7FFFFFFFu].windows : 0; }
extern "C" int mcq_refdb_taxa(const mcq_refdb* db, mcq_taxon_rec* out) {
    if (!db || (!out && !db->taxa.empty())) return fail("bad argument");
    for (size_t i = 0; i < db->taxa.size(); ++i) {
        const Taxon& t = db->taxa[i];
        out[i].id = t.id; out[i].parent = t.parent; out[i].rank = t.rank; out[i].name = t.name.c_str(); out[i].file = t.file.c_str();
        out[i].index = t.index; out[i].windows = t.windows;
    }
    return 0;
}
extern "C" uint32_t mcq_refdb_ancestor(const mcq_refdb* db, uint32_t key, uint32_t rank) {
    if (!valid_key(db, key) || rank >= (uint32_t)kNumRanks) return MCQ_NO_TAXON;
    return db->lineage[(size_t)(key & 0x7FFFFFFFu) * kNumRanks + rank];
}

// ---- ground truth of a read and clade keys: ground_truth (src/classification.cpp:111-131), next_ranked_ancestor
// (src/sketch_database.h:724-737, src/taxonomy.h:550-566), remove_hits_on_rank's db.ancestor(., rank) (src/classification.cpp:141-157)
namespace {
uint32_t next_ranked_ancestor(const mcq_refdb* db, uint32_t i) {
    const Taxon& t = db->taxa[i];
    if (t.rank == MCQ_RANK_SEQUENCE) {                           // the first entry of its ranked lineage above the sequence level
        for (int r = 1; r < kNumRanks; ++r) { const uint32_t a = db->lineage[(size_t)i * kNumRanks + r]; if (a != MCQ_NO_TAXON) return a; }
        return MCQ_NO_TAXON;
    }
    if (t.rank != MCQ_RANK_NONE) return i;
    int64_t id = t.id;
    while (id != 0) {
        auto it = db->by_id.find(id);
        if (it == db->by_id.end()) return MCQ_NO_TAXON;
        const Taxon& a = db->taxa[it->second];
        if (a.rank != MCQ_RANK_NONE) return it->second;
        if (a.parent == id) return MCQ_NO_TAXON;
        id = a.parent;
    }
    return MCQ_NO_TAXON;
}
uint32_t taxon_with_name(const mcq_refdb* db, const std::string& name) {           // src/sketch_database.h:620-626
    if (name.empty()) return MCQ_NO_TAXON;
    auto i = db->seq_names.find(name);
    return i == db->seq_names.end() ? MCQ_NO_TAXON : i->second;
}
uint32_t taxon_with_similar_name(const mcq_refdb* db, const std::string& name) {   // :631-639: the first name AFTER `name` that begins with it
    if (name.empty()) return MCQ_NO_TAXON;
    auto i = db->seq_names.upper_bound(name);
    if (i == db->seq_names.end()) return MCQ_NO_TAXON;
    if (0 != i->first.compare(0, name.size(), name)) return MCQ_NO_TAXON;
    return i->second;
}
}  // namespace

extern "C" uint32_t mcq_refdb_ground_truth(const mcq_refdb* db, const char* header, uint64_t len) {
    if (!db || (len && !header)) return MCQ_NO_TAXON;
    const std::string h(header ? header : "", (size_t)len);
    uint32_t t = taxon_with_name(db, mcq_header_accession_version(h));              // src/classification.cpp:116
    if (t == MCQ_NO_TAXON) t = taxon_with_similar_name(db, mcq_header_accession(h));   // :119
    if (t == MCQ_NO_TAXON) {                                                         // :123 (taxon id 0 is "none")
        const int64_t id = mcq_header_taxid(h);
        if (id != 0) { auto it = db->by_id.find(id); if (it != db->by_id.end()) t = it->second; }
    }
    if (t == MCQ_NO_TAXON) t = taxon_with_name(db, h);                               // :127
    return t == MCQ_NO_TAXON ? MCQ_NO_TAXON : next_ranked_ancestor(db, t);
}

extern "C" uint32_t mcq_refdb_taxon_clade(const mcq_refdb* db, uint32_t truth, uint32_t rank) {
    if (!db || !valid_key(db, truth)) return 0xFFFFFFFEu;                            // no ground truth: MCQ_CLADE_KEEP_ALL
    return mcq_refdb_ancestor(db, truth, rank);                                      // MCQ_NO_TAXON == MCQ_CLADE_NONE: no ancestor there
}

extern "C" int mcq_refdb_clade_keys(const mcq_refdb* db, uint32_t rank, uint32_t* out) {
    if (!db || !out) return fail("bad argument");
    if (rank >= (uint32_t)kNumRanks) return fail("clade keys need a rank from sequence to root");
    for (uint32_t t = 0; t < db->info.n_targets; ++t) {
        auto it = db->by_id.find(-(int64_t)t - 1);
        if (it == db->by_id.end()) return fail("target " + std::to_string(t) + " has no sequence-level taxon");
        out[t] = db->lineage[(size_t)it->second * kNumRanks + rank];
    }
    return 0;
}

// the same keys from a taxon list that has not been written yet (what mcq_build_cli is about to hand to mcq_refdb_write_shard):
// a handle without files around the list, the lineages of build_lineages, mcq_refdb_clade_keys
extern "C" int mcq_taxa_clade_keys(const mcq_taxon_rec* taxa, uint64_t n_taxa, uint32_t n_targets, uint32_t rank, uint32_t* out) {
    if ((n_taxa && !taxa) || (n_targets && !out)) return fail("bad argument");
    mcq_refdb db;
    db.taxa.reserve(n_taxa);
    for (uint64_t i = 0; i < n_taxa; ++i) {
        Taxon t; t.id = taxa[i].id; t.parent = taxa[i].parent; t.rank = taxa[i].rank; t.name = taxa[i].name ? taxa[i].name : "";
        t.index = taxa[i].index; t.windows = taxa[i].windows;
        db.taxa.push_back(std::move(t));
    }
    db.info.n_targets = n_targets; db.info.n_taxa = (uint32_t)n_taxa;
    build_lineages(&db);
    return mcq_refdb_clade_keys(&db, rank, out);
}

extern "C" uint32_t mcq_refdb_ranked_lca(const mcq_refdb* db, uint32_t a, uint32_t b) {
    if (!valid_key(db, a) || !valid_key(db, b)) return MCQ_NO_TAXON;
    const uint32_t* la = &db->lineage[(size_t)(a & 0x7FFFFFFFu) * kNumRanks];
    const uint32_t* lb = &db->lineage[(size_t)(b & 0x7FFFFFFFu) * kNumRanks];
    for (int r = 0; r <= (int)MCQ_RANK_ROOT; ++r) if (la[r] != MCQ_NO_TAXON && la[r] == lb[r]) return la[r];
    return MCQ_NO_TAXON;
}

// ---- evaluation statistics: classification_statistics (src/classification_statistics.h) and its summary (src/printing.cpp:522-600)
extern "C" void mcq_eval_stats_assign(mcq_eval_stats* s, uint32_t assigned) {               // :70-78
    if (assigned >= MCQ_RANK_NONE) ++s->assigned[MCQ_RANK_NONE];
    else for (uint32_t r = assigned; r <= MCQ_RANK_ROOT; ++r) ++s->assigned[r];
}
extern "C" void mcq_eval_stats_assign_known_correct(mcq_eval_stats* s, uint32_t assigned, uint32_t known, uint32_t correct) {   // :91-120
    assigned = std::min<uint32_t>(assigned, MCQ_RANK_NONE); known = std::min<uint32_t>(known, MCQ_RANK_NONE); correct = std::min<uint32_t>(correct, MCQ_RANK_NONE);
    mcq_eval_stats_assign(s, assigned);
    if (correct < assigned) correct = assigned;                  // plausibility check
    if (correct < known) correct = known;
    if (known == MCQ_RANK_NONE) { ++s->known[MCQ_RANK_NONE]; return; }
    for (uint32_t r = known; r <= MCQ_RANK_ROOT; ++r) ++s->known[r];
    if (correct == MCQ_RANK_NONE) ++s->correct[MCQ_RANK_NONE];
    else for (uint32_t r = correct; r <= MCQ_RANK_ROOT; ++r) ++s->correct[r];
    if (correct > known && correct > assigned)                   // all ranks below the correct one are wrong
        for (uint32_t r = MCQ_RANK_SEQUENCE; r < correct; ++r) ++s->wrong[r];
}
extern "C" void mcq_eval_stats_add(mcq_eval_stats* into, const mcq_eval_stats* from) {
    for (int r = 0; r <= (int)MCQ_RANK_NONE; ++r) {
        into->assigned[r] += from->assigned[r]; into->known[r] += from->known[r]; into->correct[r] += from->correct[r]; into->wrong[r] += from->wrong[r];
    }
}
static inline uint32_t stat_rank(uint32_t r) { return std::min<uint32_t>(r, MCQ_RANK_NONE); }
extern "C" uint64_t mcq_eval_stats_assigned(const mcq_eval_stats* s, uint32_t r) { return s->assigned[stat_rank(r)]; }
extern "C" uint64_t mcq_eval_stats_total(const mcq_eval_stats* s) { return s->assigned[MCQ_RANK_ROOT] + s->assigned[MCQ_RANK_NONE]; }
extern "C" uint64_t mcq_eval_stats_known(const mcq_eval_stats* s, uint32_t r) { return s->known[stat_rank(r)]; }
extern "C" uint64_t mcq_eval_stats_unknown(const mcq_eval_stats* s) { return s->known[MCQ_RANK_NONE]; }
extern "C" uint64_t mcq_eval_stats_correct(const mcq_eval_stats* s, uint32_t r) { return s->correct[stat_rank(r)]; }
extern "C" uint64_t mcq_eval_stats_wrong(const mcq_eval_stats* s, uint32_t r) { return s->wrong[stat_rank(r)]; }
static inline double over_total(const mcq_eval_stats* s, uint64_t n) { const uint64_t t = mcq_eval_stats_total(s); return t > 0 ? n / double(t) : 0; }   // :201-215
extern "C" double mcq_eval_stats_known_rate(const mcq_eval_stats* s, uint32_t r) { return over_total(s, mcq_eval_stats_known(s, r)); }
extern "C" double mcq_eval_stats_unknown_rate(const mcq_eval_stats* s) { return over_total(s, mcq_eval_stats_unknown(s)); }
extern "C" double mcq_eval_stats_classification_rate(const mcq_eval_stats* s, uint32_t r) { return over_total(s, mcq_eval_stats_assigned(s, r)); }
extern "C" double mcq_eval_stats_unclassified_rate(const mcq_eval_stats* s) { return over_total(s, s->assigned[MCQ_RANK_NONE]); }
extern "C" double mcq_eval_stats_sensitivity(const mcq_eval_stats* s, uint32_t r) {         // :217-219
    const uint64_t k = mcq_eval_stats_known(s, r);
    return k > 0 ? mcq_eval_stats_correct(s, r) / double(k) : 0;
}
extern "C" double mcq_eval_stats_precision(const mcq_eval_stats* s, uint32_t r) {           // :220-224
    const double tot = mcq_eval_stats_correct(s, r) + mcq_eval_stats_wrong(s, r);
    return tot > 0 ? mcq_eval_stats_correct(s, r) / tot : 0;
}
extern "C" int64_t mcq_eval_stats_text(const mcq_eval_stats* s, const char* prefix, char* buf, size_t cap) {   // src/printing.cpp:522-600
    if (!s || !prefix || (cap && !buf)) return fail("bad argument");
    static const uint32_t ranks[] = {0 /*sequence*/, 3 /*subspecies*/, 4 /*species*/, 6 /*genus*/, 10 /*family*/, 12 /*order*/,
                                     14 /*class*/, 16 /*phylum*/, 18 /*kingdom*/, 19 /*domain*/, 20 /*root*/};
    std::ostringstream os;
    auto per_rank = [&](auto&& value) {                          // one line per rank that has assignments
        for (uint32_t r : ranks) {
            if (s->assigned[r] == 0) continue;
            std::string rn = mcq_rank_name(r);
            rn.resize(11, ' ');
            os << prefix << "  " << rn; value(r); os << '\n';
        }
    };
    if (s->assigned[MCQ_RANK_ROOT] < 1) os << "None of the input sequences could be classified.\n";
    else {
        if (s->assigned[MCQ_RANK_NONE] > 0)
            os << prefix << "unclassified: " << (100 * mcq_eval_stats_unclassified_rate(s)) << "% (" << s->assigned[MCQ_RANK_NONE] << ")\n";
        os << prefix << "classified:\n";
        per_rank([&](uint32_t r) { os << (100 * mcq_eval_stats_classification_rate(s, r)) << "% (" << s->assigned[r] << ")"; });
        if (s->known[MCQ_RANK_ROOT] > 0) {
            if (s->known[MCQ_RANK_NONE] > 0)
                os << prefix << "ground truth unknown: " << (100 * mcq_eval_stats_unknown_rate(s)) << "% (" << s->known[MCQ_RANK_NONE] << ")\n";
            os << prefix << "ground truth known:\n";
            per_rank([&](uint32_t r) { os << (100 * mcq_eval_stats_known_rate(s, r)) << "% (" << s->known[r] << ")"; });
            os << prefix << "correctly classified:\n";
            per_rank([&](uint32_t r) { os << s->correct[r]; });
            os << prefix << "precision (correctly classified / classified) if ground truth known:\n";
            per_rank([&](uint32_t r) { os << (100 * mcq_eval_stats_precision(s, r)) << "%"; });
            os << prefix << "sensitivity (correctly classified / all) if ground truth known:\n";
            per_rank([&](uint32_t r) { os << (100 * mcq_eval_stats_sensitivity(s, r)) << "%"; });
        }
    }
    const std::string t = os.str();
    if (cap) { const size_t n = std::min(cap - 1, t.size()); std::memcpy(buf, t.data(), n); buf[n] = 0; }
    return (int64_t)t.size();
}

extern "C" uint32_t mcq_refdb_classify(const mcq_refdb* db, const uint32_t* c, uint32_t n,
                                       uint32_t hits_min, float hits_diff_fraction, uint32_t highest_rank) {
    if (n == 0 || !valid_key(db, c[0])) return MCQ_NO_TAXON;
    const uint64_t h0 = c[1];
    if (h0 < hits_min) return MCQ_NO_TAXON;                     // below threshold: not classifiable
    uint32_t lca = c[0] & 0x7FFFFFFFu;
    const float thr = h0 > hits_min ? (float)(h0 - hits_min) * hits_diff_fraction : 0.0f;
    for (uint32_t i = 1; i < n; ++i) {
        if (!((float)(uint64_t)c[4 * i + 1] > thr)) break;
        uint32_t r = MCQ_NO_TAXON;
        if (valid_key(db, c[4 * i])) {
            const uint32_t b = c[4 * i] & 0x7FFFFFFFu;
            for (int j = 0; j <= 20; ++j) {                      // ranked_lca: first shared non-null rank up to root
                uint32_t x = db->lineage[(size_t)lca * kNumRanks + j];
                if (x != MCQ_NO_TAXON && x == db->lineage[(size_t)b * kNumRanks + j]) { r = x; break; }
            }
        }
        lca = r;
        if (lca == MCQ_NO_TAXON || db->taxa[lca].rank > highest_rank) return MCQ_NO_TAXON;
    }
    return db->taxa[lca].rank <= highest_rank ? lca : MCQ_NO_TAXON;
}

extern "C" int mcq_refdb_lineages(const mcq_refdb* db, uint32_t* lineage, uint8_t* rank) {
    if (!db || !lineage || !rank) return fail("bad argument");
    std::memcpy(lineage, db->lineage.data(), db->lineage.size() * 4);
    for (size_t i = 0; i < db->taxa.size(); ++i) rank[i] = db->taxa[i].rank;
    return 0;
}

// ---- abundance tables: taxon_count_map (src/classification.h:107-115), estimate_abundance (src/classification.cpp:362-428),
// show_abundances / show_abundance_estimates / show_abundance_table (src/printing.cpp:474-517).  The arithmetic is the
// reference's, type for type and in its order: float counts, u64 (query_id) weights that float sums are truncated into, the
// share of a child computed as parent * (child + weight) / sum in float.  Built without FP contraction (build.py).
namespace {
struct ByRank {                                  // sortTaxaByRank: rank descending (root first), then id ascending
    const mcq_refdb* db;
    bool operator()(uint32_t a, uint32_t b) const {
        const Taxon& x = db->taxa[a]; const Taxon& y = db->taxa[b];
        if (x.rank != y.rank) return x.rank > y.rank;
        return x.id < y.id;
    }
};
using CountMap = std::map<uint32_t, float, ByRank>;

void estimate_abundance(const mcq_refdb* db, CountMap& counts, uint32_t rank) {
    const uint32_t* lin = db->lineage.data();
    if (rank != MCQ_RANK_SEQUENCE) {
        // prune below the rank: from lower_bound(taxon{id 0, rank - 1}) on, into the first ranked ancestor at or above it
        auto begin = counts.begin();
        while (begin != counts.end()) {
            const Taxon& t = db->taxa[begin->first];
            if (!(t.rank > rank - 1 || (t.rank == rank - 1 && t.id < 0))) break;
            ++begin;
        }
        for (auto it = begin; it != counts.end();) {
            uint32_t anc = MCQ_NO_TAXON;
            for (uint32_t r = rank; anc == MCQ_NO_TAXON && r < (uint32_t)kNumRanks; ++r) anc = lin[(size_t)it->first * kNumRanks + r];
            if (anc != MCQ_NO_TAXON) {
                counts[anc] += it->second;
                it = counts.erase(it);
            } else ++it;
        }
    }
    std::unordered_map<uint32_t, std::vector<uint32_t>> children;
    std::unordered_map<uint32_t, uint64_t> weight;   // query_id
    for (const auto& c : counts) weight[c.first] = 0;
    for (auto it = counts.rbegin(); it != counts.rend(); ++it) {          // leaves to root
        for (uint32_t r = (uint8_t)(db->taxa[it->first].rank + 1); r < (uint32_t)kNumRanks; ++r) {
            const uint32_t parent = lin[(size_t)it->first * kNumRanks + r];
            if (parent != MCQ_NO_TAXON && weight.count(parent)) {
                weight[parent] += weight[it->first] + it->second;
                children[parent].push_back(it->first);
                break;
            }
        }
    }
    for (auto it = counts.begin(); it != counts.end();) {                 // root to leaves: distribute, erase the parents
        auto ch = children.find(it->first);
        if (ch == children.end()) { ++it; continue; }
        const uint64_t sum = weight[it->first];
        for (uint32_t c : ch->second) counts[c] += it->second * (counts[c] + weight[c]) / sum;
        it = counts.erase(it);
    }
}
}  // namespace

extern "C" int64_t mcq_refdb_abundance_text(const mcq_refdb* db, const uint64_t* counts, uint64_t total, uint32_t est_rank,
                                            char* buf, size_t cap) {
    if (!db || !counts || (cap && !buf) || est_rank == MCQ_RANK_ROOT || est_rank > MCQ_RANK_NONE) return fail("bad argument");
    CountMap m(ByRank{db});
    for (uint32_t i = 0; i < db->taxa.size(); ++i)
        if (counts[i]) m.emplace(i, (float)counts[i]);       // exact u64 counts, one conversion (counts past 2^24)
    std::string s;
    if (est_rank == MCQ_RANK_NONE) s = "# query summary: number of queries mapped per taxon\n";
    else {
        estimate_abundance(db, m, est_rank);
        s = std::string("# estimated abundance (number of queries) per ") + mcq_rank_name(est_rank) + "\n";
    }
    char num[64];
    for (const auto& c : m) {                    // default ostream formatting of a float and of a double: %g
        const Taxon& t = db->taxa[c.first];
        s += mcq_rank_name(t.rank); s += ':'; s += t.name; s += "\t|\t";
        std::snprintf(num, sizeof num, "%g", (double)c.second); s += num; s += "\t|\t";
        std::snprintf(num, sizeof num, "%g", (double)c.second / double(total) * 100); s += num; s += "%\n";
    }
    if (cap) { const size_t n = std::min(cap - 1, s.size()); std::memcpy(buf, s.data(), n); buf[n] = 0; }
    return (int64_t)s.size();
}

// ---- the table of -hits-per-seq: matches_per_target (src/matches_per_target.h:43-188) and show_matches_per_targets
// (src/printing.cpp:437-469)
struct mcq_hits_table {
    struct Entry { uint64_t qid; std::vector<std::pair<uint32_t, uint32_t>> wins; };       // (window, hits), ascending windows
    std::map<uint32_t, std::vector<Entry>> per_target;                                    // ascending target id: the row order
    bool sorted = false;                                                                  // sort_match_lists has run since the last add / merge
};
extern "C" int mcq_hits_table_create(mcq_hits_table** out) {
    if (!out) return fail("bad argument");
    *out = new mcq_hits_table();
    return 0;
}
extern "C" int mcq_hits_table_free(mcq_hits_table* t) { delete t; return 0; }
extern "C" int mcq_hits_table_add(mcq_hits_table* t, uint64_t query_id, uint32_t target, uint32_t win_beg, uint32_t n_win, const uint32_t* counts) {
    if (!t || (n_win && !counts)) return fail("bad argument");
    mcq_hits_table::Entry e; e.qid = query_id;
    for (uint32_t i = 0; i < n_win; ++i) if (counts[i]) e.wins.emplace_back(win_beg + i, counts[i]);    // (the reference's vector holds only windows with a match)
    if (e.wins.empty()) return 0;                     // no match in the range: no candidate the reference could have had
    t->per_target[target].push_back(std::move(e));
    t->sorted = false;
    return 0;
}
extern "C" int mcq_hits_table_merge(mcq_hits_table* into, mcq_hits_table* from) {          // matches_per_target::merge: `from` is left empty
    if (!into || !from) return fail("bad argument");
    for (auto& m : from->per_target) {
        auto& dst = into->per_target[m.first];
        dst.insert(dst.end(), std::make_move_iterator(m.second.begin()), std::make_move_iterator(m.second.end()));
    }
    from->per_target.clear();
    into->sorted = false;
    return 0;
}
extern "C" uint64_t mcq_hits_table_targets(const mcq_hits_table* t) { return t ? t->per_target.size() : 0; }
extern "C" uint64_t mcq_hits_table_entries(const mcq_hits_table* t) {
    uint64_t n = 0;
    if (t) for (const auto& m : t->per_target) n += m.second.size();
    return n;
}
extern "C" uint32_t mcq_refdb_target_key(const mcq_refdb* db, uint32_t target) {
    if (!db) return MCQ_NO_TAXON;
    auto it = db->by_id.find(-(int64_t)target - 1);
    return it == db->by_id.end() ? MCQ_NO_TAXON : (0x80000000u | it->second);
}
extern "C" int mcq_refdb_tax2tgt(const mcq_refdb* db, uint32_t* out) {
    if (!db || !out) return fail("bad argument");
    for (size_t i = 0; i < db->taxa.size(); ++i) {
        const Taxon& t = db->taxa[i];
        out[i] = (t.rank == MCQ_RANK_SEQUENCE && t.id < 0 && (uint64_t)(-t.id - 1) < db->info.n_targets) ? (uint32_t)(-t.id - 1) : MCQ_NO_TAXON;
    }
    return 0;
}
namespace {
// show_taxon / show_no_taxon (src/printing.cpp:117-176) for one taxon index or, with MCQ_NO_TAXON, the blank of `rank`
void put_taxon(std::string& s, const mcq_refdb* db, uint32_t idx, uint32_t rank, const mcq_taxon_print& m) {
    const bool have = idx != MCQ_NO_TAXON;
    if (m.show_ranks) { s += mcq_rank_name(have ? db->taxa[idx].rank : rank); s += ':'; }
    const std::string id = std::to_string(have ? (long long)db->taxa[idx].id : 0ll);
    if (m.body != 1) s += have ? db->taxa[idx].name : std::string("--");
    if (m.body == 2) s += '(';
    if (m.body != 0) s += id;
    if (m.body == 2) s += ')';
}
// the sequence column of a per-target table: show_taxon(os, db, opt, tax) (src/printing.cpp:305-330) of target `tgt`'s sequence-level
// taxon, as Out::best of mcq_cli_common.hpp writes it (highest_rank beyond root is read as root: the lineage has no entry above it);
// *windows: its windows_in_sequence.  false: the target has no sequence-level taxon
bool put_sequence(std::string& s, const mcq_refdb* db, uint32_t tgt, const mcq_taxon_print& mode, uint64_t* windows) {
    const uint32_t key = mcq_refdb_target_key(db, tgt);
    if (key == MCQ_NO_TAXON) return false;
    const uint32_t idx = key & 0x7FFFFFFFu;
    const uint32_t highest = std::min<uint32_t>(mode.highest_rank, MCQ_RANK_ROOT);
    if (db->taxa[idx].rank > highest) s += (mode.body == 1 && !mode.show_ranks) ? "0" : "--";
    else {
        const uint32_t rmin = std::max<uint32_t>(mode.lowest_rank, db->taxa[idx].rank);
        const uint32_t rmax = mode.lineage ? highest : rmin;
        for (uint32_t r = rmin; r <= rmax; ++r) {
            put_taxon(s, db, db->lineage[(size_t)idx * kNumRanks + r], r, mode);
            if (r < rmax) s += ',';
        }
    }
    *windows = tgt < db->seq_windows.size() ? db->seq_windows[tgt] : db->taxa[idx].windows;
    return true;
}
}  // namespace
// the block of show_matches_per_targets, handed to `sink` piece by piece (the head, then one piece per row): nothing of the table's
// text is held beyond one row
extern "C" int mcq_hits_table_write(mcq_hits_table* t, const mcq_refdb* db, const char* comment, const char* column,
                                    const mcq_taxon_print* mode, mcq_text_sink sink, void* user) {
    if (!t || !db || !comment || !column || !mode || !sink || mode->body > 2) return fail("bad argument");
    // sort_match_lists (src/matches_per_target.h:172-184): first window, then last window, then query id
    if (!t->sorted) {
        for (auto& m : t->per_target)
            std::sort(m.second.begin(), m.second.end(), [](const mcq_hits_table::Entry& a, const mcq_hits_table::Entry& b) {
                if (a.wins.front().first != b.wins.front().first) return a.wins.front().first < b.wins.front().first;
                if (a.wins.back().first != b.wins.back().first) return a.wins.back().first < b.wins.back().first;
                return a.qid < b.qid;
            });
        t->sorted = true;
    }
    std::string s;
    s += comment; s += "--- list of hits for each reference sequence ---\n";
    s += comment; s += "window start position within sequence = window_index * window_stride(=" + std::to_string(db->info.q_winstride) + ")\n";
    s += comment; s += "TABLE_LAYOUT:  sequence "; s += column; s += " windows_in_sequence "; s += column;
    s += "queryid/window_index:hits/window_index:hits/...,queryid/...\n";
    if (sink(user, s.data(), s.size())) return fail("the sink refused the table's head");
    // (rows in ascending target id: the reference walks an unordered_map of taxon pointers, an order no two runs need share)
    for (const auto& m : t->per_target) {
        s.clear();
        uint64_t windows = 0;
        if (!put_sequence(s, db, m.first, *mode, &windows)) return fail("target " + std::to_string(m.first) + " has no sequence-level taxon");
        s += column; s += std::to_string(windows); s += column;
        bool first = true;
        for (const auto& e : m.second) {
            if (first) first = false; else s += ',';
            s += std::to_string(e.qid);
            for (const auto& w : e.wins) { s += '/'; s += std::to_string(w.first); s += ':'; s += std::to_string(w.second); }
        }
        s += '\n';
        if (sink(user, s.data(), s.size())) return fail("the sink refused a row of the table");
    }
    return 0;
}
namespace {
struct TextBuf { char* buf; size_t cap, len; };
int text_buf_sink(void* user, const char* data, size_t n) {
    TextBuf* b = static_cast<TextBuf*>(user);
    if (b->cap && b->len < b->cap - 1) std::memcpy(b->buf + b->len, data, std::min(n, b->cap - 1 - b->len));
    b->len += n;
    return 0;
}
}  // namespace
// the same into a caller's buffer (cut to cap - 1 bytes, NUL-terminated); returns the whole length.  For tests and small tables: a
// caller that asks for the length first formats the table twice -- mcq_hits_table_write formats it once
extern "C" int64_t mcq_hits_table_text(mcq_hits_table* t, const mcq_refdb* db, const char* comment, const char* column,
                                       const mcq_taxon_print* mode, char* buf, size_t cap) {
    if (cap && !buf) return fail("bad argument");
    TextBuf b{buf, cap, 0};
    if (mcq_hits_table_write(t, db, comment, column, mode, text_buf_sink, &b)) return -1;
    if (cap) buf[std::min(b.len, cap - 1)] = 0;
    return (int64_t)b.len;
}

// ---- coverage of reference sequences (-coverage, -cov-percentile): the cut and the report over what mcq_coverage_read returns
extern "C" int mcq_refdb_seq_windows(const mcq_refdb* db, uint32_t* out) {
    if (!db || !out) return fail("bad argument");
    for (uint32_t t = 0; t < db->info.n_targets; ++t) {
        const uint64_t w = t < db->seq_windows.size() ? db->seq_windows[t] : 0;
        if (w >= (1ull << 32)) return fail("a target with 2^32 windows or more");
        out[t] = (uint32_t)w;
    }
    return 0;
}
// THE CUT RULE (the project's own; tests/coverage_ref.py restates it):
//   * the hit targets are those with windows_covered > 0; H is their number;
//   * they are ordered by breadth windows_covered / windows ascending -- compared exactly, a before b iff
//     a.covered * b.windows < b.covered * a.windows in 64 bits (both factors are below 2^32), never as floats; ties go by ascending id;
//   * the first K = floor(H * percentile / 100) of them (in double arithmetic, at most H) are removed;
//   * so percentile 0 removes nothing, 100 removes every hit target, and a target without a covered window is never removed.
extern "C" int mcq_coverage_cut(const mcq_target_coverage* cov, const uint32_t* windows, uint32_t n_targets, double percentile, uint8_t* removed) {
    if ((n_targets && (!cov || !windows || !removed)) || !(percentile >= 0.0 && percentile <= 100.0)) return fail("mcq_coverage_cut: bad argument (percentile 0..100)");
    std::vector<uint32_t> hit;
    for (uint32_t t = 0; t < n_targets; ++t) { removed[t] = 0; if (cov[t].windows_covered > 0) hit.push_back(t); }
    std::sort(hit.begin(), hit.end(), [&](uint32_t a, uint32_t b) {
        const uint64_t l = (uint64_t)cov[a].windows_covered * windows[b], r = (uint64_t)cov[b].windows_covered * windows[a];
        return l != r ? l < r : a < b;
    });
    const uint64_t K = std::min<uint64_t>(hit.size(), (uint64_t)std::floor((double)hit.size() * percentile / 100.0));
    for (uint64_t i = 0; i < K; ++i) removed[hit[i]] = 1;
    return 0;
}
// the report block: two head lines behind `comment`, one more for each of reads_skipped / out_of_range that is not 0, then one row per
// target with queries > 0 in ascending target id -- sequence (as in the -hits-per-seq table), windows_in_sequence, windows_covered,
// coverage (the fraction, six decimals; 0 for a target without windows), queries, hits, kept | removed (removed == NULL: all kept)
extern "C" int mcq_coverage_write(const mcq_refdb* db, const mcq_target_coverage* cov, const uint32_t* windows, uint32_t n_targets,
                                  const uint8_t* removed, uint64_t reads_skipped, uint64_t out_of_range, const char* comment,
                                  const char* column, const mcq_taxon_print* mode, mcq_text_sink sink, void* user) {
    if (!db || (n_targets && (!cov || !windows)) || !comment || !column || !mode || !sink || mode->body > 2) return fail("bad argument");
    std::string s;
    s += comment; s += "--- coverage of reference sequences ---\n";
    if (reads_skipped) { s += comment; s += std::to_string(reads_skipped) + " queries beyond the capacity of mcq_target_hits added nothing\n"; }
    if (out_of_range) { s += comment; s += std::to_string(out_of_range) + " candidate ranges outside their sequence added nothing\n"; }
    s += comment; s += "TABLE_LAYOUT:  sequence ";
    for (const char* c : {"windows_in_sequence", "windows_covered", "coverage", "queries", "hits"}) { s += column; s += ' '; s += c; s += ' '; }
    s += column; s += " kept\n";
    if (sink(user, s.data(), s.size())) return fail("the sink refused the report's head");
    for (uint32_t t = 0; t < n_targets; ++t) {
        if (!cov[t].queries) continue;
        s.clear();
        uint64_t seq_windows = 0;
        if (!put_sequence(s, db, t, *mode, &seq_windows)) return fail("target " + std::to_string(t) + " has no sequence-level taxon");
        char frac[64];
        std::snprintf(frac, sizeof(frac), "%.6f", windows[t] ? (double)cov[t].windows_covered / (double)windows[t] : 0.0);
        s += column; s += std::to_string(windows[t]);
        s += column; s += std::to_string(cov[t].windows_covered);
        s += column; s += frac;
        s += column; s += std::to_string(cov[t].queries);
        s += column; s += std::to_string(cov[t].hits);
        s += column; s += (removed && removed[t]) ? "removed" : "kept";
        s += '\n';
        if (sink(user, s.data(), s.size())) return fail("the sink refused a row of the report");
    }
    return 0;
}
extern "C" int64_t mcq_coverage_text(const mcq_refdb* db, const mcq_target_coverage* cov, const uint32_t* windows, uint32_t n_targets,
                                     const uint8_t* removed, uint64_t reads_skipped, uint64_t out_of_range, const char* comment,
                                     const char* column, const mcq_taxon_print* mode, char* buf, size_t cap) {
    if (cap && !buf) return fail("bad argument");
    TextBuf b{buf, cap, 0};
    if (mcq_coverage_write(db, cov, windows, n_targets, removed, reads_skipped, out_of_range, comment, column, mode, text_buf_sink, &b)) return -1;
    if (cap) buf[std::min(b.len, cap - 1)] = 0;
    return (int64_t)b.len;
}

extern "C" uint32_t mcq_default_hits_min(uint32_t s) { return s >= 6 ? (uint32_t)(s / 3.0) : (s >= 4 ? 2u : 1u); }

static const char* kRankNames[] = {"sequence", "form", "variety", "subspecies", "species", "subgenus", "genus", "subtribe",
                                   "tribe", "subfamily", "family", "suborder", "order", "subclass", "class", "subphylum",
                                   "phylum", "subkingdom", "kingdom", "domain", "root", "none"};
extern "C" const char* mcq_rank_name(uint32_t r) { return kRankNames[r < 21 ? r : 21]; }
extern "C" uint32_t mcq_rank_from_name(const char* name) {
    if (!name) return MCQ_RANK_NONE;
    std::string s(name);
    std::transform(s.begin(), s.end(), s.begin(), ::tolower);
    static const std::map<std::string, uint32_t> m = {
        {"sequence", 0}, {"genome", 0}, {"form", 1}, {"forma", 1}, {"variety", 2}, {"varietas", 2}, {"subspecies", 3},
        {"species", 4}, {"species group", 5}, {"species subgroup", 5}, {"subgenus", 5}, {"genus", 6}, {"subtribe", 7},
        {"tribe", 8}, {"subfamily", 9}, {"family", 10}, {"superfamily", 11}, {"parvorder", 11}, {"infraorder", 11},
        {"suborder", 11}, {"order", 12}, {"superorder", 13}, {"infraclass", 13}, {"subclass", 13}, {"class", 14},
        {"superclass", 15}, {"subphylum", 15}, {"phylum", 16}, {"division", 16}, {"superphylum", 17}, {"subkingdom", 17},
        {"kingdom", 18}, {"subdomain", 18}, {"superkingdom", 19}, {"domain", 19}, {"root", 20}};
    auto it = m.find(s);
    return it == m.end() ? MCQ_RANK_NONE : it->second;
}

// ------------------------------------------------------------------ read files in chunks (mcq_query_cli's input stage)
#include <cerrno>
#include <fcntl.h>
#include <unistd.h>

struct mcq_read_stream {
    int fd = -1; bool eof = false;
    const char* carry = nullptr; uint64_t carry_len = 0;        // the unconsumed tail of the last fill (in the caller's buffer)
    const char* last = nullptr; uint64_t last_len = 0;
};

extern "C" int mcq_read_stream_open(const char* path, mcq_read_stream** out) {
    if (!path || !out) return fail("null argument");
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) return fail(std::string("can't open file ") + path);
#ifdef POSIX_FADV_SEQUENTIAL
    (void)posix_fadvise(fd, 0, 0, POSIX_FADV_SEQUENTIAL);
#endif
    mcq_read_stream* s = new mcq_read_stream();
    s->fd = fd;
    *out = s;
    return 0;
}

extern "C" int mcq_read_stream_fill(mcq_read_stream* s, char* buf, uint64_t cap, uint64_t want, uint64_t* len, int32_t* eof) {
    if (!s || !buf || !len || !eof) return fail("null argument");
    if (s->carry_len > cap) return fail("the carried bytes do not fit the buffer");
    if (s->carry_len && s->carry != buf) std::memmove(buf, s->carry, s->carry_len);
    uint64_t n = s->carry_len;
    s->carry = nullptr; s->carry_len = 0;
    want = std::max(std::min(want, cap), n);
    while (n < want && !s->eof) {
        const ssize_t r = ::read(s->fd, buf + n, (size_t)std::min<uint64_t>(want - n, 1ull << 30));
        if (r < 0) { if (errno == EINTR) continue; return fail(std::string("read failed: ") + std::strerror(errno)); }
        if (r == 0) s->eof = true;
        n += (uint64_t)r;
    }
    s->last = buf; s->last_len = n;
    *len = n; *eof = s->eof ? 1 : 0;
    return 0;
}

extern "C" int mcq_read_stream_consume(mcq_read_stream* s, uint64_t n_bytes) {
    if (!s || !s->last) return fail("no fill to consume from");
    if (n_bytes > s->last_len) return fail("consumed more than the last fill holds");
    s->carry = s->last + n_bytes; s->carry_len = s->last_len - n_bytes;
    s->last = nullptr; s->last_len = 0;
    return 0;
}

extern "C" int mcq_read_stream_close(mcq_read_stream* s) {
    if (!s) return 0;
    if (s->fd >= 0) ::close(s->fd);
    delete s;
    return 0;
}

namespace {
// the records of one chunk as std::getline reads them (mcq_query_mpi.cpp: read_records)
struct ChunkRecs {
    std::vector<uint64_t> start, hb, he, piece_at;     // per record: first byte, header line [hb, he) after '@' / '>', first piece
    std::vector<uint64_t> pieces;                      // (begin, end) byte ranges of sequence text, record after record
    uint64_t n_complete = 0, end = 0;                  // records [0, n_complete) are complete; `end` is just past the last one
    uint64_t seq_len(uint64_t r) const {
        uint64_t n = 0;
        const uint64_t e = r + 1 < piece_at.size() ? piece_at[r + 1] : pieces.size() / 2;
        for (uint64_t i = piece_at[r]; i < e; ++i) n += pieces[2 * i + 1] - pieces[2 * i];
        return n;
    }
};

void parse_chunk(const char* t, uint64_t L, bool eof, uint64_t max_recs, ChunkRecs& R) {
    // one getline from p: 1 = line [p, *le), next line at *next; 0 = none (end of file); -1 = the line is not whole in the chunk
    auto line = [&](uint64_t p, uint64_t* le, uint64_t* next) -> int {
        if (p >= L) return eof ? 0 : -1;
        const void* nl = std::memchr(t + p, '\n', L - p);
        if (nl) { *le = (uint64_t)((const char*)nl - t); *next = *le + 1; return 1; }
        if (!eof) return -1;
        *le = L; *next = L; return 1;
    };
    uint64_t pos = 0, le = 0, next = 0;
    auto last_incomplete = [&]() { R.n_complete = R.start.size() - 1; R.end = R.start.back(); };
    for (;;) {
        const int k = line(pos, &le, &next);
        if (k == 0) { R.n_complete = R.start.size(); R.end = L; return; }
        if (k < 0) {          // a line that goes on in the next chunk: if it starts a record, every record before it is complete
            if (!R.start.empty() && !(pos < L && (t[pos] == '@' || t[pos] == '>'))) last_incomplete();
            else { R.n_complete = R.start.size(); R.end = pos; }
            return;
        }
        if (le == pos) { pos = next; continue; }                    // empty line
        const char c = t[pos];
        if (c == '@' || c == '>') {
            if (R.start.size() == max_recs) { R.n_complete = max_recs; R.end = pos; return; }
            R.start.push_back(pos); R.hb.push_back(pos + 1); R.he.push_back(le); R.piece_at.push_back(R.pieces.size() / 2);
            pos = next;
            if (c == '@') {                                          // getline sequence, '+' and qualities
                for (int i = 0; i < 3; ++i) {
                    const int k2 = line(pos, &le, &next);
                    if (k2 < 0) { last_incomplete(); return; }
                    if (k2 == 0) break;                              // end of file: the failed getlines leave the record as it is
                    if (i == 0) { R.pieces.push_back(pos); R.pieces.push_back(le); }
                    pos = next;
                }
            }
            continue;
        }
        if (!R.start.empty()) { R.pieces.push_back(pos); R.pieces.push_back(le); }   // joined to the record before it
        pos = next;
    }
}
}  // namespace

extern "C" int mcq_reads_parse(const char* text1, uint64_t len1, const char* text2, uint64_t len2, uint32_t flags,
                               uint64_t max_queries, uint64_t max_bases, char* bases, uint64_t* seq_off, uint64_t* hdr, uint64_t* info) {
    if ((len1 && !text1) || (len2 && !text2) || !bases || !seq_off || !hdr || !info) return fail("null argument");
    if (max_queries < 1) return fail("max_queries must be >= 1");
    const bool paired = text2 != nullptr, inter = (flags & MCQ_READS_INTERLEAVED) != 0;
    if (inter && paired) return fail("MCQ_READS_INTERLEAVED is given with text2 == NULL");
    const bool eof1 = (flags & MCQ_READS_EOF1) != 0;
    ChunkRecs R[2];
    parse_chunk(text1, len1, eof1, inter ? (max_queries > (UINT64_MAX >> 1) ? UINT64_MAX : 2 * max_queries) : max_queries, R[0]);
    if (paired) parse_chunk(text2, len2, (flags & MCQ_READS_EOF2) != 0, max_queries, R[1]);
    // query q is record q of each text, or (interleaved) records 2q and 2q+1 of text1: sequence_pair_reader::next,
    // src/sequence_io.cpp:442-462.  There the second next() of a file that has run out gives an empty sequence, so an
    // unpaired last record (an odd count, which under eof1 only the end of the text leaves: max_recs is even) is a query.
    uint64_t nq = R[0].n_complete;
    if (paired) nq = std::min(nq, R[1].n_complete);
    if (inter) nq = nq / 2 + ((eof1 && (nq & 1)) ? 1 : 0);
    const int mates = (paired || inter) ? 2 : 1;
    const char* text[2] = {text1, inter ? text1 : text2};
    auto rec = [&](uint64_t q, int m) { return inter ? 2 * q + (uint64_t)m : q; };
    auto has = [&](uint64_t q, int m) { return !inter || rec(q, m) < R[0].n_complete; };
    uint64_t n = 0, nb = 0;
    seq_off[0] = 0;
    for (; n < nq; ++n) {
        uint64_t len = 0;
        for (int m = 0; m < mates; ++m) if (has(n, m)) len += R[inter ? 0 : m].seq_len(rec(n, m));
        if (n && nb + len > max_bases) break;
        for (int m = 0; m < mates; ++m) {
            const ChunkRecs& X = R[inter ? 0 : m];
            const uint64_t r = rec(n, m);
            const uint64_t e = r + 1 < X.piece_at.size() ? X.piece_at[r + 1] : X.pieces.size() / 2;
            for (uint64_t i = has(n, m) ? X.piece_at[r] : e; i < e; ++i) {
                const uint64_t b = X.pieces[2 * i], l = X.pieces[2 * i + 1] - b;
                std::memcpy(bases + nb, text[m] + b, l); nb += l;
            }
            seq_off[n * mates + m + 1] = nb;
        }
        const uint64_t r0 = rec(n, 0);
        const char* sp = (const char*)std::memchr(text1 + R[0].hb[r0], ' ', R[0].he[r0] - R[0].hb[r0]);
        hdr[2 * n] = R[0].hb[r0]; hdr[2 * n + 1] = sp ? (uint64_t)(sp - text1) : R[0].he[r0];
    }
    std::memset(info, 0, MCQ_READS_INFO_WORDS * 8);
    info[MCQ_READS_N] = n; info[MCQ_READS_BASES] = nb;
    for (int m = 0; m < (inter ? 1 : mates); ++m)        // the next chunk starts at the first record not taken, or behind everything this one held
        info[MCQ_READS_CUT1 + m] = rec(n, 0) < R[m].n_complete ? R[m].start[rec(n, 0)] : R[m].end;
    info[MCQ_READS_COMPLETE1] = inter ? nq : R[0].n_complete;
    info[MCQ_READS_COMPLETE2] = paired ? R[1].n_complete : 0;
    return 0;
}

// ---- a database that is a taxonomy alone: what `merge` works on (main_mode_merge reads the taxonomy dump, no shard file) ----------
extern "C" int mcq_refdb_from_taxdump(const mcq_taxdump* dump, mcq_refdb** out) {
    if (!dump || !out) return fail("bad argument");
    const uint64_t n = mcq_taxdump_count(dump);
    if (n == 0 || n >= (1ull << 31)) return fail("a taxonomy of 1 .. 2^31 - 1 taxa");
    const mcq_taxon_rec* recs = mcq_taxdump_taxa(dump);
    mcq_refdb* db = new mcq_refdb();
    db->taxa.reserve(n);
    for (uint64_t i = 0; i < n; ++i) {
        Taxon t; t.id = recs[i].id; t.parent = recs[i].parent; t.rank = recs[i].rank; t.name = recs[i].name ? recs[i].name : "";
        t.file = recs[i].file ? recs[i].file : ""; t.index = recs[i].index; t.windows = recs[i].windows;
        db->taxa.push_back(std::move(t));
    }
    db->info.n_taxa = (uint32_t)n;                // (no targets, no table, no sketching parameters: all 0)
    build_lineages(db);
    *out = db;
    return 0;
}

extern "C" int mcq_refdb_taxid_table(const mcq_refdb* db, int64_t* ids, uint32_t* index, uint64_t* n_ids) {
    if (!db || !ids || !index || !n_ids) return fail("bad argument");
    std::vector<std::pair<int64_t, uint32_t>> v;
    v.reserve(db->taxa.size());
    for (uint32_t i = 0; i < db->taxa.size(); ++i) v.emplace_back(db->taxa[i].id, i);
    std::sort(v.begin(), v.end());
    uint64_t n = 0;
    for (size_t i = 0; i < v.size(); ++i)
        if (i == 0 || v[i].first != v[i - 1].first) {
            const auto it = db->by_id.find(v[i].first);      // (taxon_with_id: the index the id map holds)
            ids[n] = v[i].first; index[n] = it != db->by_id.end() ? it->second : v[i].second; ++n;
        }
    *n_ids = n;
    return 0;
}
