/* mcq_open.hpp -- header-only C++ helper above the two C ABIs (include/mcq.h, include/mcq_host.h): the reference's shard files
 * -> the queryable GPU handle, by whichever route fits the database's size.  Used by the drop-in CLIs (csrc/host/) and by the
 * reference-side binding (integration/mcq_reference_binding.cpp).
 *
 * Replaces sketch_database::read (src/sketch_database.h:858-952) + hash_multimap::deserialize (src/hash_multimap.h:923-964):
 *   small databases: mcq_refdb_open unions the P shard tables on the host (16 B per location) -> mcq_db_create;
 *   from `stream_min_bytes` of shard files on: mcq_refdb_open_meta reads only the heads; the key records are streamed to the GPU in
 *   chunks of 4 M locations (48 MB of host memory each; up to 8 files are parsed at a time by as many host threads), the P ranks
 *   merged there per feature-hash range (mcq_parts_builder_*), the handle made from the parts (32-bit global-window words) -- host
 *   memory stays at a few chunks whatever the database's size.
 * Both functions take the reference's database query options as a last argument (mcq_query_tuning: another query sketcher, the
 * bucket rules of -max-locations-per-feature / -remove-overpopulated-features); a bucket rule always takes the streaming route,
 * where it is applied per chunk on the GPU (mcq_parts_builder_set_bucket_limit).                                            */
#ifndef MCQ_OPEN_HPP
#define MCQ_OPEN_HPP
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "mcq.h"
#include "mcq_host.h"

#define MCQ_STREAM_LOAD_DEFAULT_MIN_BYTES (1ull << 30)

/* MCQ_BUILD_TRACE=1: resident set of the process at the steps of the streaming route, on stderr */
inline void mcq_trace_rss(const char* what) {
    if (!std::getenv("MCQ_BUILD_TRACE")) return;
    long pages = 0, rss = 0;
    if (FILE* f = std::fopen("/proc/self/statm", "r")) { if (std::fscanf(f, "%ld %ld", &pages, &rss) != 2) rss = 0; std::fclose(f); }
    std::fprintf(stderr, "[mcq_open] %-34s rss %8.1f MB\n", what, rss * 4096.0 / 1048576.0);
}

/* threshold in bytes: MCQ_STREAM_LOAD_MIN_MB overrides the default of 1 GB (0 = always stream) */
inline uint64_t mcq_stream_load_min_bytes() {
    if (const char* e = std::getenv("MCQ_STREAM_LOAD_MIN_MB")) return std::strtoull(e, nullptr, 10) << 20;
    return MCQ_STREAM_LOAD_DEFAULT_MIN_BYTES;
}

/* The reference's database query options (get_database_query_options, src/query_options.cpp:41-66; applied to every rank's
 * table in src/mode_query.cpp:354-387).  Every int is -1 for "the database's".  DESIGN.md section 31. */
struct mcq_query_tuning {
    int winlen = -1, winstride = -1, sketchlen = -1;   // -winlen, -winstride, -sketchlen: how the READS are sketched (winstride 0: given
                                                       // and not applied -- then -winlen does not set the stride either)
    int max_locs = -1;                                 // -max-locations-per-feature N
    bool remove_overpopulated = false;                 // -remove-overpopulated-features
};

/* (N, removal, the database's own limit) -> the rule on every (feature, rank) bucket, as mcq_bucket_limit takes it: a bucket of
 * more than *remove_above locations goes (0: none does), then a bucket of more than *keep_first keeps its first *keep_first
 * (0: no shrink).  Line for line src/mode_query.cpp:354-377 with max_locations_per_feature, src/sketch_database.h:356-368; the
 * quirks are the reference's: without removal N <= 1 is ignored; with it the threshold is N - 1, 253 where that is negative or
 * 254 and more, at most the database's limit - 1, used only when positive; the setter takes N as the 8-bit bucket size type, so
 * N is narrowed modulo 256 first (300 -> 44, 256 -> 0), a value below 1 becomes 1, 254 and 255 mean "the largest": no shrink;
 * and it shrinks only below the database's limit. */
inline void mcq_bucket_rule(int max_locs, bool remove_overpopulated, uint32_t db_limit, uint32_t* keep_first, uint32_t* remove_above) {
    const int max_supported = 254;                                       // max_supported_locations_per_feature(): 255 - 1
    *keep_first = 0; *remove_above = 0;
    auto setter = [&](int n_int) {                                       // max_locations_per_feature(bucket_size_type n)
        int n = (int)(uint8_t)n_int;
        if (n < 1) n = 1;
        if (n >= max_supported) return;
        if ((uint32_t)n < db_limit) *keep_first = (uint32_t)n;
    };
    if (remove_overpopulated) {
        int maxlpf = max_locs - 1;
        if (maxlpf < 0 || maxlpf >= max_supported) maxlpf = max_supported - 1;
        maxlpf = std::min(maxlpf, (int)db_limit - 1);
        if (maxlpf > 0) *remove_above = (uint32_t)maxlpf;
        setter(max_locs);
    } else if (max_locs > 1)
        setter(max_locs);
}

/* the query sketcher under a tuning (src/query_options.cpp:55-59, src/mode_query.cpp:379-387): -winlen W without -winstride sets
 * the stride to W too; only positive values are applied (the setter's "below 1 becomes 1" is never reached with a value that is
 * applied).  false with the text in err when a value lies outside the engine's limits (include/mcq.h, mcq_db_desc). */
inline bool mcq_tuned_sketcher(const mcq_refdb_info& info, const mcq_query_tuning& t, uint32_t* winlen, uint32_t* winstride, uint32_t* sketch, std::string& err) {
    *winlen = info.q_winlen; *winstride = info.q_winstride; *sketch = info.q_sketch_size;
    const int stride = t.winstride >= 0 ? t.winstride : (t.winlen > 0 ? t.winlen : -1);
    if (t.winlen > 0) *winlen = (uint32_t)t.winlen;
    if (stride > 0) *winstride = (uint32_t)stride;
    if (t.sketchlen > 0) *sketch = (uint32_t)t.sketchlen;
    if (t.winlen > 0 && *winlen > 128) { err = "-winlen " + std::to_string(t.winlen) + ": the engine sketches query windows of at most 128 bases"; return false; }
    if (t.winlen > 0 && *winlen < info.k) { err = "-winlen " + std::to_string(t.winlen) + ": a query window holds at least k = " + std::to_string(info.k) + " bases"; return false; }
    if (t.sketchlen > 0 && *sketch > 32) { err = "-sketchlen " + std::to_string(t.sketchlen) + ": the engine takes sketches of at most 32 features"; return false; }
    return true;
}

/* opens <prefix>.db_0 .. db_<P-1>: the full host-side union below the threshold, heads only (mcq_refdb_open_meta) from it on;
 * *streamed says which.  A tuning with a bucket rule (-max-locations-per-feature, -remove-overpopulated-features) takes the
 * streaming route whatever the size -- the rule is applied per chunk on the GPU, there is no host-side filter --, and one whose
 * sketcher the engine cannot run fails here, before any table is read.  0 on success, else the text in err. */
inline int mcq_open_refdb(const std::string& prefix, uint32_t P, uint64_t stream_min_bytes, mcq_refdb** rdb, bool* streamed, std::string& err,
                          const mcq_query_tuning& tuning = mcq_query_tuning()) {
    uint64_t total = 0;
    for (uint32_t r = 0; r < P; ++r)
        if (FILE* f = std::fopen((prefix + ".db_" + std::to_string(r)).c_str(), "rb")) { std::fseek(f, 0, SEEK_END); total += (uint64_t)std::ftell(f); std::fclose(f); }
    *streamed = total >= stream_min_bytes;
    const bool tuned = tuning.winlen > 0 || tuning.winstride > 0 || tuning.sketchlen > 0 || tuning.max_locs > 1 || tuning.remove_overpopulated;
    if (tuned) {
        mcq_refdb* meta = nullptr;
        if (mcq_refdb_open_meta(prefix.c_str(), P, &meta)) { err = mcq_host_last_error(); return -1; }
        mcq_refdb_info info; mcq_refdb_get_info(meta, &info);
        uint32_t wl, ws, sk, keep = 0, rem = 0;
        const bool ok = mcq_tuned_sketcher(info, tuning, &wl, &ws, &sk, err);
        mcq_bucket_rule(tuning.max_locs, tuning.remove_overpopulated, info.max_locs_per_feature, &keep, &rem);
        if (!ok) { mcq_refdb_close(meta); return -1; }
        if (keep || rem) *streamed = true;
        if (*streamed) { *rdb = meta; return 0; }
        mcq_refdb_close(meta);
    }
    if (*streamed ? mcq_refdb_open_meta(prefix.c_str(), P, rdb) : mcq_refdb_open(prefix.c_str(), P, rdb)) { err = mcq_host_last_error(); return -1; }
    return 0;
}

/* the handle of shard `shard_id` of `n_shards` from an opened mcq_refdb; tgt2tax: [n_targets] taxon keys (mcq_refdb_tgt2tax or the
 * caller's own).  0 on success, else the text in err. */
inline int mcq_make_db(mcq_refdb* rdb, bool streamed, const uint32_t* tgt2tax, uint32_t n_shards, uint32_t shard_id, int device,
                       mcq_db** out, std::string& err, const mcq_query_tuning& tuning = mcq_query_tuning(),
                       uint64_t* n_shrunk = nullptr, uint64_t* n_removed = nullptr) {
    mcq_refdb_info info; mcq_refdb_get_info(rdb, &info);
    uint32_t q_winlen, q_winstride, q_sketch, keep_first = 0, remove_above = 0;
    if (!mcq_tuned_sketcher(info, tuning, &q_winlen, &q_winstride, &q_sketch, err)) return -1;
    mcq_bucket_rule(tuning.max_locs, tuning.remove_overpopulated, info.max_locs_per_feature, &keep_first, &remove_above);
    if (n_shrunk) *n_shrunk = 0;
    if (n_removed) *n_removed = 0;
    if ((keep_first || remove_above) && !streamed) { err = "a bucket rule needs the streaming route: open the database with the same tuning"; return -1; }
    if (!streamed) {
        mcq_db_desc d; std::memset(&d, 0, sizeof(d));
        d.k = info.k; d.sketch_size = q_sketch; d.winlen = q_winlen; d.winstride = q_winstride;
        d.tgt_winstride = info.winstride; d.n_targets = info.n_targets; d.n_keys = info.n_keys; d.n_locs = info.n_locs;
        d.keys = mcq_refdb_keys(rdb); d.list_off = mcq_refdb_list_off(rdb); d.locs = mcq_refdb_locs(rdb); d.tgt2tax = tgt2tax;
        d.n_shards = n_shards; d.shard_id = shard_id; d.flags = 0; d.device = device;
        static const uint64_t zero_off[1] = {0};
        if (!d.list_off) d.list_off = zero_off;
        if (mcq_db_create(&d, out)) { err = mcq_last_error(); return -1; }
        return 0;
    }
    mcq_trace_rss("heads read");
    std::vector<uint32_t> tw(info.n_targets);
    if (mcq_refdb_tgt_windows(rdb, tw.data())) { err = mcq_host_last_error(); return -1; }
    mcq_parts_builder_desc bd; std::memset(&bd, 0, sizeof(bd));
    bd.k = info.k; bd.sketch_size = q_sketch; bd.winlen = q_winlen; bd.winstride = q_winstride; bd.tgt_winstride = info.winstride;
    bd.n_targets = info.n_targets; bd.tgt_windows = tw.data(); bd.expected_locations = info.n_locs;
    bd.n_shards = n_shards; bd.shard_id = shard_id; bd.device = device;
    mcq_parts_builder* pb = nullptr;
    if (mcq_parts_builder_create(&bd, &pb)) { err = mcq_build_last_error(); return -1; }
    if ((keep_first || remove_above) && mcq_parts_builder_set_bucket_limit(pb, keep_first, remove_above)) {
        err = mcq_build_last_error(); mcq_parts_builder_free(pb); return -1;
    }
    mcq_trace_rss("builder created (GPU runtime up)");
    // the files are parsed by up to 8 host threads (one open stream and one 48 MB chunk each: record parsing is ~1 GB/s per thread),
    // which take turns handing their chunks to the builder (MCQ_STREAM_LOAD_THREADS overrides; 1 = the calling thread alone)
    const uint64_t chunk = 1u << 22;
    unsigned n_thr = std::thread::hardware_concurrency();
    if (const char* e = std::getenv("MCQ_STREAM_LOAD_THREADS")) n_thr = (unsigned)std::strtoul(e, nullptr, 10);
    n_thr = std::max(1u, std::min(std::min(n_thr, 8u), info.n_ranks));
    std::mutex mu; std::string first_err;
    auto work = [&](unsigned tix) {
        std::vector<uint32_t> cf(chunk), ct(chunk), cw(chunk);
        for (uint32_t r = tix; r < info.n_ranks; r += n_thr) {
            mcq_shard_stream* st = nullptr;
            if (mcq_shard_stream_open(rdb, r, &st)) { std::lock_guard<std::mutex> g(mu); if (first_err.empty()) first_err = mcq_host_last_error(); return; }
            for (;;) {
                uint64_t n = 0;
                if (mcq_shard_stream_next(st, cf.data(), ct.data(), cw.data(), chunk, &n)) {
                    std::lock_guard<std::mutex> g(mu); if (first_err.empty()) first_err = mcq_host_last_error(); n = 0; mcq_shard_stream_close(st); return;
                }
                if (!n) break;
                std::lock_guard<std::mutex> g(mu);
                if (!first_err.empty()) { mcq_shard_stream_close(st); return; }           // (another thread failed: stop)
                if (mcq_parts_builder_add(pb, cf.data(), ct.data(), cw.data(), n, 0)) { first_err = mcq_build_last_error(); mcq_shard_stream_close(st); return; }
            }
            mcq_shard_stream_close(st);
            mcq_trace_rss("a shard file streamed");
        }
    };
    if (n_thr == 1) work(0);
    else {
        std::vector<std::thread> thr;
        for (unsigned t = 0; t < n_thr; ++t) thr.emplace_back(work, t);
        for (auto& t : thr) t.join();
    }
    if (!first_err.empty()) { err = first_err; mcq_parts_builder_free(pb); return -1; }
    if (n_shrunk && n_removed) mcq_parts_builder_bucket_counts(pb, n_shrunk, n_removed);
    mcq_parts* parts = nullptr;
    if (mcq_parts_builder_finish(pb, &parts)) { err = mcq_build_last_error(); mcq_parts_builder_free(pb); return -1; }
    mcq_trace_rss("ranges sorted: parts made");
    const int rc = mcq_db_from_parts(parts, tgt2tax, n_shards, shard_id, 0, out);
    mcq_parts_free(parts);
    if (rc) { err = mcq_build_last_error(); return -1; }
    mcq_trace_rss("table made");
    return 0;
}
#endif
