// mcq_info_cli -- the reference's `metacache info` (src/mode_info.cpp) on a database of P shard files:
//   mcq_info_cli DB P                     static properties and the "hit classifier" block          (main_mode_info, nargs == 2)
//   mcq_info_cli DB P targets [NAME...]   show_target_info                                           (host)
//   mcq_info_cli DB P lineages            show_lineage_table                                         (host)
//   mcq_info_cli DB P rank RANK           show_rank_statistics                                       (host)
//   mcq_info_cli DB P statistics          print_static_properties + print_content_properties         (GPU: mcq_content_stats_*)
//   mcq_info_cli DB P locations           locations of every target, no counterpart in the reference (GPU)
//   mcq_info_cli DB P featurecounts       the statistics and a `feature -> size` line per bucket, in the files' order
// The metadata modes are host text over the heads of the shard files (mcq_refdb_open_meta).  The content statistics are a pass over
// every location of every file: a reader thread parses the records (mcq_shard_stream_*) into two pinned buffers, the main thread
// copies a filled one to the device, applies the bucket rule if one is given (mcq_bucket_limit_ws with a scratch buffer of its own)
// and hands the chunk to mcq_content_stats_add.  The text comes from the exact integer totals by the reference's formulas in the
// reference's types (float for the bucket count, double for the moments).  DESIGN.md section 32.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <mutex>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/mcq.h"
#include "../../../include/mcq_host.h"
#include "../../../include/mcq_open.hpp"
#include "mcq_cli_buffers.hpp"

namespace {

const char* const kUsage =
    "usage: mcq_info_cli DB P [MODE] [options]      (DB.db_0 .. DB.db_<P-1> are the shard files)\n"
    "  (no mode)                 the database's static properties\n"
    "  targets [NAME...]         every target, or the named ones (aliases: target, sequ, sequence, sequences)\n"
    "  lineages                  the ranked lineage of every target as a table (aliases: lineage, lin)\n"
    "  rank RANK                 targets per taxon of that rank\n"
    "  statistics                static properties and the table's content: buckets, bucket sizes, features, locations (alias: stat)\n"
    "  locations                 per target: name, windows, locations, locations / (windows x sketch size)   [not in the reference]\n"
    "  featurecounts             the statistics and one `feature -> size` line per bucket (alias: featuresizes)\n"
    "options of statistics, locations and featurecounts:\n"
    "  -shard R                  one shard file only: the output of the reference's `info DB.db_R statistics`\n"
    "  -histogram                after the content block one line `bucket size S: COUNT` per size that occurs (255: 255 and more)\n"
    "  -max-locations-per-feature N, -remove-overpopulated-features\n"
    "                            what the table would hold under these query options (the rule is applied on the GPU)\n"
    "  -device D                 the GPU to use (default 0)\n"
    "  -chunk TRIPLES            locations per chunk (default 4194304, at least 255)\n"
    "  -timing                   the phases' milliseconds on stderr\n"
    "not reproduced: `features` / `featuremap` (a dump of every location); `featurecounts` lists the files' order, the reference its\n"
    "hash table's.\n";

const char* const kRule = "------------------------------------------------\n";

struct Opts {
    std::string db, mode;
    uint32_t P = 0;
    std::vector<std::string> names;          // positional arguments behind the mode
    int shard = -1, device = 0;
    bool histogram = false, timing = false;
    mcq_query_tuning tuning;
    uint64_t chunk = 1u << 22;
};

int abort_with(const std::string& msg) { std::fprintf(stderr, "ABORT: %s\n", msg.c_str()); return 1; }

// print_static_properties (src/sketch_database.h:1161-1195), line for line; the type names are what the reference built with g++
// prints (MC_TARGET_ID_TYPE = uint32_t, as every shard file this project reads)
void static_block(std::ostream& os, const mcq_refdb_info& i) {
    os << kRule
       << "MetaCache version    0.5.0 (20182310)\n"
       << "database verion      20181001\n"
       << kRule
       << "sequence type        std::__cxx11::basic_string<char, std::char_traits<char>, std::allocator<char> >\n"
       << "target id type       unsigned int 32 bits\n"
       << "target limit         4294967295\n"
       << kRule
       << "window id type       unsigned int 32 bits\n"
       << "window limit         4294967295\n"
       << "window length        " << i.winlen << '\n'
       << "window stride        " << i.winstride << '\n'
       << kRule
       << "sketcher type        mc::single_function_unique_min_hasher<unsigned int, mc::same_size_hash<unsigned int> >\n"
       << "feature type         unsigned int 32 bits\n"
       << "feature hash         mc::same_size_hash<unsigned int>\n"
       << "kmer size            " << i.k << '\n'
       << "kmer limit           16\n"
       << "sketch size          " << i.sketch_size << '\n'
       << kRule
       << "bucket size type     unsigned char 8 bits\n"
       << "max. locations       " << i.max_locs_per_feature << '\n'
       << "location limit       254\n"
       << "------------------------------------------------" << std::endl;
}

// the taxa of the database as the reference's std::set holds them: ascending ids, the targets' (below zero) first
struct Taxa {
    std::vector<mcq_taxon_rec> rec;          // the handle's order: a taxon key indexes it
    std::vector<uint32_t> by_id;             // indices, ascending ids
    std::vector<uint32_t> targets;           // indices of the taxa with an id below zero, ascending ids: target_taxa()
    bool load(const mcq_refdb* db, uint32_t n_taxa) {
        rec.resize(n_taxa);
        if (mcq_refdb_taxa(db, rec.data())) return false;
        by_id.resize(n_taxa);
        for (uint32_t i = 0; i < n_taxa; ++i) by_id[i] = i;
        std::sort(by_id.begin(), by_id.end(), [&](uint32_t a, uint32_t b) { return rec[a].id < rec[b].id; });
        for (uint32_t i : by_id) if (rec[i].id < 0) targets.push_back(i);
        return true;
    }
};

// show_target_info(os, db, tax), src/mode_info.cpp:138-153 (the ")" behind the name is the reference's)
void target_info(std::ostream& os, const mcq_refdb* db, const Taxa& tx, uint32_t idx, const std::vector<uint32_t>& tgt_windows) {
    const mcq_taxon_rec& t = tx.rec[idx];
    const uint64_t target = (uint64_t)(-t.id - 1);
    const uint64_t windows = (t.id < 0 && target < tgt_windows.size()) ? tgt_windows[target] : t.windows;
    os << "Target " << t.name << "):\n"
       << "    source:     " << t.file << " / " << t.index
       << "\n    length:     " << windows << " windows";
    for (uint32_t r = 0; r <= MCQ_RANK_ROOT; ++r) {
        const uint32_t a = mcq_refdb_ancestor(db, idx, r);
        if (a == MCQ_NO_TAXON) continue;
        std::string rn = std::string(mcq_rank_name(tx.rec[a].rank)) + ":";
        rn.resize(12, ' ');
        os << "\n    " << rn << "(" << tx.rec[a].id << ") " << tx.rec[a].name;
    }
    os << '\n';
}

int mode_targets(const mcq_refdb* db, const mcq_refdb_info& info, const Opts& o) {
    Taxa tx;
    std::vector<uint32_t> tw(info.n_targets);
    if (!tx.load(db, info.n_taxa) || mcq_refdb_tgt_windows(db, tw.data())) return abort_with(mcq_host_last_error());
    if (!o.names.empty()) {
        std::map<std::string, uint32_t> name2tax;                            // sequence-level taxa by name, the first of a name stays
        for (uint32_t i : tx.by_id) if (tx.rec[i].rank == MCQ_RANK_SEQUENCE) name2tax.insert({tx.rec[i].name, i});
        for (const std::string& sid : o.names) {
            auto it = sid.empty() ? name2tax.end() : name2tax.find(sid);
            if (it != name2tax.end()) target_info(std::cout, db, tx, it->second, tw);
            else std::cout << "Target (reference sequence) " << sid << " not found in database.\n";
        }
    } else {
        std::cout << "Targets (reference sequences) in database:\n";
        for (uint32_t i : tx.targets) target_info(std::cout, db, tx, i, tw);
    }
    return 0;
}

int mode_lineages(const mcq_refdb* db, const mcq_refdb_info& info) {
    if (info.n_targets < 1) return 0;
    Taxa tx;
    if (!tx.load(db, info.n_taxa)) return abort_with(mcq_host_last_error());
    std::cout << "name";
    for (uint32_t r = MCQ_RANK_SEQUENCE; r <= MCQ_RANK_DOMAIN; ++r) std::cout << '\t' << mcq_rank_name(r);
    std::cout << '\n';
    for (uint32_t i : tx.targets) {
        std::cout << tx.rec[i].name;
        for (uint32_t r = MCQ_RANK_SEQUENCE; r <= MCQ_RANK_DOMAIN; ++r) {
            const uint32_t a = mcq_refdb_ancestor(db, i, r);
            std::cout << '\t' << (a != MCQ_NO_TAXON ? tx.rec[a].id : (int64_t)0);       // taxonomy::none_id()
        }
        std::cout << '\n';
    }
    return 0;
}

// show_rank_statistics, src/mode_info.cpp:231-264.  The reference's table is a std::map keyed by the taxa's addresses in a std::set
// -- the order of their allocation, which no file states --; here the rows come by ascending taxon id.
int mode_rank(const mcq_refdb* db, const mcq_refdb_info& info, const std::string& rank_name) {
    const uint32_t rank = mcq_rank_from_name(rank_name.c_str());
    if (rank >= MCQ_RANK_NONE) return abort_with("rank not recognized: " + rank_name);
    Taxa tx;
    if (!tx.load(db, info.n_taxa)) return abort_with(mcq_host_last_error());
    std::map<int64_t, std::pair<uint32_t, uint64_t>> stat;                   // taxon id -> (index, sequences)
    for (uint32_t i : tx.targets) {
        const uint32_t a = mcq_refdb_ancestor(db, i, rank);
        if (a == MCQ_NO_TAXON) continue;
        auto it = stat.insert({tx.rec[a].id, {a, 0}}).first;
        ++it->second.second;
    }
    std::cout << "Sequence distribution for rank " << rank_name << ":\n" << "taxid \t taxon_name \t sequences" << std::endl;
    for (const auto& s : stat) std::cout << s.first << " \t " << tx.rec[s.second.first].name << " \t " << s.second.second << '\n';
    return 0;
}

// ---- the content of the table ----------------------------------------------------------------------------------------------
// hash_multimap::reserve_keys (src/hash_multimap.h:611-613) on the empty table a file is read into: size_type(1 + (1 / 0.8f * n)), float
uint64_t reserve_buckets(uint64_t n_keys) {
    const float inv = 1 / 0.8f;
    const float scaled = inv * (float)n_keys;
    return (uint64_t)(1 + scaled);
}

// the bucket sizes' max / mean / stddev / skewness from the exact power sums, in double by the accumulator's own formulas
// (src/stat_moments.h:565-572, :680-696, :817-836), operation for operation (x86-64 without FMA: nothing is contracted)
void moments(const mcq_content_totals& t, double* mx, double* mean, double* sd, double* skew) {
    const double n = (double)t.n_buckets, sum = (double)t.n_locations, sum2 = (double)t.sum2, sum3 = (double)t.sum3;
    const uint64_t size = t.n_buckets;
    *mx = (double)t.max_size;
    *mean = size < 1 ? sum : sum / n;
    const double s2 = sum * sum;
    *sd = std::sqrt(size < 1 ? 0 : ((sum2 - s2 / n) / (n - 1)));
    if (size < 2) { *skew = 0; return; }
    const double n2 = n * n;
    const double cm2 = (sum2 - s2 / n) / (n - 1);
    const double cm3 = (n2 * sum3 - 3 * n * (sum * sum2) + 2 * (s2 * sum)) / (n * n2);
    *skew = cm3 / std::pow(cm2, 3 / 2.);
}

struct Meta { uint64_t targets = 0, ranked = 0, tree_taxa = 0; };

// print_content_properties, src/sketch_database.h:1205-1237
void content_block(std::ostream& os, const Meta& m, uint64_t buckets, uint64_t features, uint64_t dead, uint64_t locations, const mcq_content_totals& t) {
    if (m.targets > 0)
        os << "targets              " << m.targets << '\n' << "ranked targets       " << m.ranked << '\n' << "taxa in tree         " << m.tree_taxa << '\n';
    if (features > 0) {
        double mx, mean, sd, skew;
        moments(t, &mx, &mean, &sd, &skew);
        os << kRule << "buckets              " << buckets << '\n'
           << "bucket size          " << "max: " << mx << " mean: " << mean << " +/- " << sd << " <> " << skew << '\n'
           << "features             " << features << '\n' << "dead features        " << dead << '\n' << "locations            " << locations << '\n';
    }
    os << kRule;
}

// the chunks of the shard files named in `shards`, one file after the other, parsed by a thread of its own into two slots of pinned
// memory; a slot with n == 0 ends a file
struct Reader {
    struct Slot { PinnedBuf<uint32_t> f, t, w; uint64_t n = 0; bool full = false; };
    Slot slot[2];
    std::mutex mu; std::condition_variable cv;
    std::string err; bool stop = false;
    std::thread thr;
    double ms_parse = 0;
    bool start(const mcq_refdb* db, const std::vector<uint32_t>& shards, uint64_t chunk) {
        for (Slot& s : slot) if (!s.f.grow(chunk) || !s.t.grow(chunk) || !s.w.grow(chunk)) return false;
        thr = std::thread([this, db, shards, chunk]() {
            int b = 0;
            for (uint32_t r : shards) {
                mcq_shard_stream* st = nullptr;
                if (mcq_shard_stream_open(db, r, &st)) { fail(mcq_host_last_error()); return; }
                for (;;) {
                    Slot& s = slot[b];
                    { std::unique_lock<std::mutex> g(mu); cv.wait(g, [&] { return !s.full || stop; }); if (stop) { mcq_shard_stream_close(st); return; } }
                    uint64_t n = 0;
                    const auto t0 = std::chrono::steady_clock::now();
                    if (mcq_shard_stream_next(st, s.f.p, s.t.p, s.w.p, chunk, &n)) { mcq_shard_stream_close(st); fail(mcq_host_last_error()); return; }
                    ms_parse += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                    { std::lock_guard<std::mutex> g(mu); s.n = n; s.full = true; }
                    cv.notify_all();
                    b ^= 1;
                    if (!n) break;
                }
                mcq_shard_stream_close(st);
            }
        });
        return true;
    }
    void fail(const char* text) { { std::lock_guard<std::mutex> g(mu); err = text; } cv.notify_all(); }
    // the next filled slot (nullptr with the text in err after a failure); give it back with release()
    Slot* take(int b) {
        std::unique_lock<std::mutex> g(mu);
        cv.wait(g, [&] { return slot[b].full || !err.empty(); });
        return slot[b].full ? &slot[b] : nullptr;
    }
    void release(int b) { { std::lock_guard<std::mutex> g(mu); slot[b].full = false; } cv.notify_all(); }
    ~Reader() { { std::lock_guard<std::mutex> g(mu); stop = true; } cv.notify_all(); if (thr.joinable()) thr.join(); }
};

struct Pass {
    std::vector<mcq_content_totals> per_shard;      // in the order of `shards`
    std::vector<uint64_t> tgt_locs;
    double ms_parse = 0, ms_stats = 0, ms_all = 0;
    uint64_t chunks = 0, shrunk = 0, removed = 0;
};

// one pass over the shard files: every chunk to the device, through the rule, into the statistics.  lines != nullptr: the
// `feature -> size` line of every bucket that is left, from the host's copy of the chunk (rule off) or the device's (rule on)
int content_pass(const mcq_refdb* db, const mcq_refdb_info& info, const Opts& o, const std::vector<uint32_t>& shards, uint32_t keep_first,
                 uint32_t remove_above, Pass& out, std::ostream* lines) {
    const auto t_all = std::chrono::steady_clock::now();
    MCQ_HIP(hipSetDevice(o.device), return 1);
    mcq_content_stats* cs = nullptr;
    if (mcq_content_stats_create(std::max(1u, info.n_targets), &cs)) return abort_with(mcq_last_error());
    struct Free { mcq_content_stats* h; ~Free() { mcq_content_stats_free(h); } } free_cs{cs};
    Stream st, copy; Event copied, t_beg, t_end;
    if (!st.create() || !copy.create() || !copied.create()) return 1;
    MCQ_HIP(hipEventCreate(&t_beg.h), return 1); MCQ_HIP(hipEventCreate(&t_end.h), return 1);
    if (mcq_content_stats_set_stream(cs, st.h)) return abort_with(mcq_last_error());
    const bool rule = keep_first || remove_above;
    DeviceBuf<uint32_t> df, dt, dw; DeviceBuf<char> scratch;
    if (!df.grow(o.chunk) || !dt.grow(o.chunk)) return 1;
    const uint64_t scratch_bytes = rule ? mcq_bucket_limit_scratch_bytes(o.chunk) : 0;
    if (rule && (!dw.grow(o.chunk) || !scratch.grow(scratch_bytes))) return 1;
    std::vector<uint32_t> kept;                     // the features that are left of a chunk under a rule, for the lines
    Reader rd;
    if (!rd.start(db, shards, o.chunk)) return 1;
    out.per_shard.clear();
    int b = 0;
    for (size_t k = 0; k < shards.size(); ++k) {
        for (;;) {
            Reader::Slot* s = rd.take(b);
            if (!s) return abort_with(rd.err);
            uint64_t n = s->n;
            if (!n) { rd.release(b); b ^= 1; break; }
            MCQ_HIP(hipMemcpyAsync(df.p, s->f.p, n * 4, hipMemcpyHostToDevice, copy), return 1);
            MCQ_HIP(hipMemcpyAsync(dt.p, s->t.p, n * 4, hipMemcpyHostToDevice, copy), return 1);
            if (rule) MCQ_HIP(hipMemcpyAsync(dw.p, s->w.p, n * 4, hipMemcpyHostToDevice, copy), return 1);
            MCQ_HIP(hipEventRecord(copied, copy), return 1);
            MCQ_HIP(hipStreamWaitEvent(st, copied, 0), return 1);
            if (rule) {
                uint64_t counts[3] = {0, 0, 0};
                if (mcq_bucket_limit_ws(df.p, dt.p, dw.p, n, keep_first, remove_above, o.device, st.h, scratch.p, scratch_bytes, counts)) return abort_with(mcq_last_error());
                MCQ_HIP(hipStreamSynchronize(st), return 1);
                if (counts[0] > n) return abort_with("the bucket rule kept more triples than it was given");
                n = counts[0]; out.shrunk += counts[1]; out.removed += counts[2];
            }
            MCQ_HIP(hipEventRecord(t_beg, st), return 1);
            if (mcq_content_stats_add(cs, df.p, dt.p, nullptr, n, MCQ_DEVICE_PTRS)) return abort_with(mcq_last_error());
            MCQ_HIP(hipEventRecord(t_end, st), return 1);
            MCQ_HIP(hipEventSynchronize(t_end), return 1);
            float ms = 0; MCQ_HIP(hipEventElapsedTime(&ms, t_beg, t_end), return 1);
            out.ms_stats += ms; ++out.chunks;
            if (lines) {
                const uint32_t* f = s->f.p;
                if (rule) { kept.resize(n); MCQ_HIP(hipMemcpy(kept.data(), df.p, n * 4, hipMemcpyDeviceToHost), return 1); f = kept.data(); }
                for (uint64_t i = 0; i < n;) {
                    uint64_t j = i + 1;
                    while (j < n && f[j] == f[i]) ++j;
                    *lines << f[i] << " -> " << (j - i) << '\n';
                    i = j;
                }
            }
            rd.release(b); b ^= 1;
        }
        mcq_content_totals t;
        if (mcq_content_stats_totals(cs, &t) || mcq_content_stats_reset(cs)) return abort_with(mcq_last_error());
        out.per_shard.push_back(t);
    }
    out.tgt_locs.assign(std::max(1u, info.n_targets), 0);
    if (mcq_content_stats_target_locations(cs, out.tgt_locs.data())) return abort_with(mcq_last_error());
    rd.thr.join();                                  // (every file's last slot was taken: the thread has left its loop)
    out.ms_parse = rd.ms_parse;
    out.ms_all = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_all).count();
    return 0;
}

int mode_content(const mcq_refdb* db, const mcq_refdb_info& info, const Opts& o) {
    if (o.shard >= 0 && (uint32_t)o.shard >= o.P) return abort_with("-shard " + std::to_string(o.shard) + ": the database has shards 0 .. " + std::to_string(o.P - 1));
    uint32_t keep_first = 0, remove_above = 0;
    mcq_bucket_rule(o.tuning.max_locs, o.tuning.remove_overpopulated, info.max_locs_per_feature, &keep_first, &remove_above);
    const bool rule = keep_first || remove_above;
    std::vector<uint32_t> shards;
    if (o.shard >= 0) shards.push_back((uint32_t)o.shard); else for (uint32_t r = 0; r < o.P; ++r) shards.push_back(r);
    Taxa tx;
    if (!tx.load(db, info.n_taxa)) return abort_with(mcq_host_last_error());
    Meta meta;
    meta.targets = info.n_targets; meta.tree_taxa = info.n_taxa - info.n_targets;
    for (uint32_t i : tx.targets) meta.ranked += tx.rec[i].parent != 0;
    const bool featurecounts = o.mode == "featurecounts" || o.mode == "featuresizes";
    Pass pass;
    if (int rc = content_pass(db, info, o, shards, keep_first, remove_above, pass, nullptr)) return rc;
    if (o.timing)
        std::cerr << "phases ms: parse " << pass.ms_parse << ", content statistics " << pass.ms_stats << ", all " << pass.ms_all << " (" << pass.chunks
                  << " chunks; buckets shrunk " << pass.shrunk << ", removed " << pass.removed << ")" << std::endl;
    if (o.mode == "locations") {
        std::vector<uint32_t> tw(info.n_targets);
        if (mcq_refdb_tgt_windows(db, tw.data())) return abort_with(mcq_host_last_error());
        std::cout << "name\twindows\tlocations\tfill\n";
        char num[32];
        for (uint32_t t = 0; t < info.n_targets; ++t) {
            const uint32_t key = mcq_refdb_target_key(db, t);
            const double fill = tw[t] ? (double)pass.tgt_locs[t] / ((double)tw[t] * info.sketch_size) : 0.0;
            std::snprintf(num, sizeof num, "%.3f", fill);
            std::cout << (key == MCQ_NO_TAXON ? "" : tx.rec[key & 0x7FFFFFFFu].name) << '\t' << tw[t] << '\t' << pass.tgt_locs[t] << '\t' << num << '\n';
        }
        return 0;
    }
    // the block of the shard, or of every bucket of every shard: counts are summed, max and moments taken over all buckets
    mcq_content_totals t; std::memset(&t, 0, sizeof t);
    uint64_t buckets = 0, file_keys = 0;
    for (size_t k = 0; k < shards.size(); ++k) {
        const mcq_content_totals& s = pass.per_shard[k];
        t.n_buckets += s.n_buckets; t.n_locations += s.n_locations; t.sum2 += s.sum2; t.sum3 += s.sum3;
        t.max_size = std::max(t.max_size, s.max_size);
        for (int i = 0; i < 256; ++i) t.hist[i] += s.hist[i];
        uint64_t nk = 0;
        if (mcq_refdb_file_stats(db, shards[k], nullptr, &nk, nullptr)) return abort_with(mcq_host_last_error());
        buckets += nk ? reserve_buckets(nk) : 0; file_keys += nk;
    }
    // without a rule `features` is the files' key count and a key without locations a dead feature, as the reference counts; under a
    // rule both are what is left
    const uint64_t features = rule ? t.n_buckets : file_keys, dead = rule ? 0 : file_keys - t.n_buckets;
    static_block(std::cout, info);
    content_block(std::cout, meta, buckets, features, dead, t.n_locations, t);
    if (o.histogram) for (int s = 0; s < 256; ++s) if (t.hist[s]) std::cout << "bucket size " << s << ": " << t.hist[s] << '\n';
    if (featurecounts) {
        std::cout << "===================================================\n";
        Pass again;
        if (int rc = content_pass(db, info, o, shards, keep_first, remove_above, again, &std::cout)) return rc;
        std::cout << "===================================================\n";
    }
    return 0;
}

bool parse(int argc, char** argv, Opts& o) {
    std::vector<std::string> pos;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto next = [&]() -> const char* { return (i + 1 < argc) ? argv[++i] : ""; };
        if (a == "-help" || a == "--help" || a == "-h") { std::fputs(kUsage, stdout); return false; }
        else if (a.empty() || a[0] != '-') pos.push_back(a);
        else if (a == "-shard") o.shard = std::max(0, std::atoi(next()));
        else if (a == "-histogram") o.histogram = true;
        else if (a == "-max-locations-per-feature") o.tuning.max_locs = std::atoi(next());
        else if (a == "-remove-overpopulated-features") o.tuning.remove_overpopulated = true;
        else if (a == "-device") o.device = std::atoi(next());
        else if (a == "-chunk") o.chunk = std::max<uint64_t>(255, std::strtoull(next(), nullptr, 10));
        else if (a == "-timing") o.timing = true;
        else { abort_with("option " + a + " is not supported by mcq_info_cli"); return false; }
    }
    if (pos.size() < 2) { std::fputs(kUsage, stderr); abort_with("a database name and its number of shard files are needed"); return false; }
    o.db = pos[0];
    o.P = (uint32_t)std::max(0, std::atoi(pos[1].c_str()));
    if (o.P < 1) { abort_with("the number of shard files must be at least 1"); return false; }
    if (pos.size() > 2) o.mode = pos[2];
    o.names.assign(pos.begin() + std::min<size_t>(3, pos.size()), pos.end());
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    Opts o;
    if (!parse(argc, argv, o)) return 1;
    std::cerr << "Reading database from files '" << o.db << ".db_0' .. '.db_" << (o.P - 1) << "' ... " << std::flush;
    mcq_refdb* db = nullptr;
    if (mcq_refdb_open_meta(o.db.c_str(), o.P, &db)) { std::cerr << "FAIL" << std::endl; return abort_with(mcq_host_last_error()); }
    std::cerr << "done." << std::endl;
    struct Close { mcq_refdb* d; ~Close() { mcq_refdb_close(d); } } close_db{db};
    mcq_refdb_info info;
    mcq_refdb_get_info(db, &info);
    const std::string& m = o.mode;
    int rc = 0;
    if (m.empty()) {                                                         // show_database_config + print_query_config
        static_block(std::cout, info);
        std::cout << std::endl;
        std::cout << "hit classifier       mc::best_distinct_matches_in_contiguous_window_ranges\n" << kRule << std::endl;
    }
    else if (m == "target" || m == "targets" || m == "sequ" || m == "sequence" || m == "sequences") rc = mode_targets(db, info, o);
    else if (m == "lineages" || m == "lineage" || m == "lin") rc = mode_lineages(db, info);
    else if (m == "rank") {
        if (o.names.empty()) {
            std::cerr << "Please specify a taxonomic rank:\n";
            for (uint32_t r = MCQ_RANK_SEQUENCE; r <= MCQ_RANK_DOMAIN; ++r) std::cerr << "    " << mcq_rank_name(r) << '\n';
            rc = abort_with("mode rank needs a rank");
        } else rc = mode_rank(db, info, o.names[0]);
    }
    else if (m == "statistics" || m == "stat" || m == "locations" || m == "featurecounts" || m == "featuresizes") rc = mode_content(db, info, o);
    else if (m == "features" || m == "featuremap") rc = abort_with("mode " + m + " (a dump of every location) is not reproduced; see featurecounts and locations");
    else {
        std::cerr << "Info mode '" << m << "' not recognized.\n" << "Properties of database " << o.db << ":" << std::endl;
        static_block(std::cerr, info);
        rc = abort_with("info mode '" + m + "' not recognized");
    }
    std::cout.flush();
    return rc;
}
