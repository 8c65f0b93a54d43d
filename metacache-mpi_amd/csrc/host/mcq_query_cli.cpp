// mcq_query_cli -- `metacache query <db> <files and directories> [-pairfiles | -pairseq] ...` on one GPU: see mcq_cli_common.hpp
// for what is written and which reference code each part stands in for.
//
// The reads stream through three slots in rotation.  For batch j, ReadBatcher::next (mcq_read_batches.hpp)
// fills slot j % 3 from a chunk of each file of the unit it is in and leaves the batch on the device; mcq_query runs on it on a second stream, the
// candidates copied back behind it, while -threads host threads format the mapping lines of batch j - 2.  Host memory is fixed by
// -read-chunk and -batch.  All that is held has an owner (mcq_cli_buffers.hpp, Database, Run): every `return` of main frees it.
//
// -ground-truth / -precision alone change nothing of this: the writer threads resolve each read's truth from its whole header (the
// slot's chunk, from the printed token on to the end of the line) next to its classification.  -exclude RANK needs the truths BEFORE
// the query: the batch's header ranges come to the host and its clade keys go to the device before mcq_query is enqueued
// (Run::stage_clades), which costs overlap between the input and the query stage.  Only that option pays it.
#include "mcq_cli_common.hpp"
#include "mcq_read_batches.hpp"

#include <array>
#include <sstream>
#include <thread>

namespace {

// one of the three slots: a batch's input (mcq_read_batches.hpp) and its results
struct Slot : ReadSlot {
    DeviceBuf<mcq_cand> d_cands; DeviceBuf<uint32_t> d_ncand; PinnedBuf<mcq_cand> cands; PinnedBuf<uint32_t> ncand; Event done;
    std::vector<uint32_t> truth; PinnedBuf<uint32_t> clade; DeviceBuf<uint32_t> d_clade;   // -exclude: the truths and clade keys of the batch
};
constexpr int NS = 3;

// the batches in flight, the workspace they run in and what their lines add up to
struct Run {
    const Options& p; const Database& db; const Out o; const mcq_classify_opts co;
    mcq_taxonomy* tx = nullptr;                                  // -abundances / -abundance-per: every batch is also classified on the GPU
    std::vector<uint64_t> tax_counts; mcq_ws* ws = nullptr; uint64_t ws_cap = 0;
    std::ofstream fout; std::ostream* os = nullptr;
    Stream s_k; Event ev_in;
    Slot slot[NS];
    uint64_t assigned[MCQ_RANK_NONE + 1] = {0};
    mcq_eval_stats eval;                                         // -precision: assign_known_correct over all reads
    std::vector<uint32_t> tgt_clade;                             // -exclude: every target's clade key at the rank
    size_t issued = 0, retired = 0;                              // batches enqueued; batches whose lines are written or being written
    size_t announced = 0;                                        // units whose "# f1 + f2" line is written (by finish, in batch order)
    std::future<bool> pending;                                   // the formatting of batch `retired - 1`, beside the reading of the next

    Run(const Options& p_, const Database& db_) : p(p_), db(db_), o(make_out(db_.rdb, p_)), co(classify_opts(p_, db_.hitmin)) { std::memset(&eval, 0, sizeof(eval)); }
    ~Run() { if (pending.valid()) pending.wait(); mcq_ws_destroy(ws); mcq_taxonomy_destroy(tx); }

    bool init() {
        if (p.tax_counts()) {
            if (!(tx = make_taxonomy(db.rdb, 0))) return false;
            mcq_refdb_info rinfo; mcq_refdb_get_info(db.rdb, &rinfo);
            tax_counts.assign((size_t)rinfo.n_taxa + 1, 0);
        }
        if (excluding()) {
            tgt_clade.resize(db.t2t.size());
            if (mcq_refdb_clade_keys(db.rdb, p.exclude_rank, tgt_clade.data())) { std::fprintf(stderr, "ABORT: %s\n", mcq_host_last_error()); return false; }
        }
        if (!s_k.create() || !ev_in.create()) return false;
        for (Slot& S : slot) if (!S.done.create()) return false;
        os = &open_out(p, fout);
        write_head(*os, o, db.hitmin);
        return true;
    }

    bool excluding() const { return p.exclude_rank != MCQ_RANK_NONE; }
    // the ground truth of query q of the batch in S: from its whole header, which goes on behind the printed token to the end of its line
    uint32_t truth_of(const Slot& S, uint64_t q) const {
        const char* h = S.text[0].p + S.hdr.p[2 * q];
        const char* end = S.text[0].p + S.len[0];
        const char* nl = static_cast<const char*>(std::memchr(h, '\n', (size_t)(end - h)));
        return mcq_refdb_ground_truth(db.rdb, h, (uint64_t)((nl ? nl : end) - h));
    }
    // -exclude: the batch's header ranges on the host, its truths resolved, their clade keys on the device (ordered on `st`, which
    // has prepared the batch) and handed to the workspace for the query that follows
    bool stage_clades(Slot& S, hipStream_t st) {
        const uint64_t n = S.n;
        if (!S.clade.grow(n) || !S.d_clade.grow(n)) return false;
        if (!S.host_parsed) {
            MCQ_HIP(hipMemcpyAsync(S.hdr.p, S.d_hdr.p, 2 * n * 8, hipMemcpyDeviceToHost, st), return false);
            MCQ_HIP(hipStreamSynchronize(st), return false);
        }
        S.truth.resize(n);
        const unsigned T = (unsigned)std::min<uint64_t>(std::max(1u, p.threads), std::max<uint64_t>(1, n / 64));
        auto slice = [&](unsigned t) {
            for (uint64_t q = n * t / T; q < n * (t + 1) / T; ++q) {
                S.truth[q] = truth_of(S, q);
                S.clade.p[q] = mcq_refdb_taxon_clade(db.rdb, S.truth[q], p.exclude_rank);
            }
        };
        std::vector<std::thread> th;
        for (unsigned t = 1; t < T; ++t) th.emplace_back(slice, t);
        slice(0);
        for (auto& x : th) x.join();
        MCQ_HIP(hipMemcpyAsync(S.d_clade.p, S.clade.p, n * 4, hipMemcpyHostToDevice, st), return false);
        if (mcq_ws_set_query_clades(ws, S.d_clade.p, n, MCQ_DEVICE_PTRS)) { std::fprintf(stderr, "FAIL: %s\n", mcq_last_error()); return false; }
        return true;
    }

    // the mapping lines of batch j, in input order: -threads slices, each into a string of its own, written in order
    bool finish(size_t j) {
        Slot& S = slot[j % NS];
        if (hipEventSynchronize(S.done) != hipSuccess) { std::fprintf(stderr, "FAIL: batch %zu did not complete\n", j); return false; }
        announce(S.unit + 1);
        const uint64_t n = S.n;
        const unsigned T = (unsigned)std::min<uint64_t>(std::max(1u, p.threads), std::max<uint64_t>(1, n / 64));
        std::vector<std::string> out(T);
        std::vector<std::array<uint64_t, MCQ_RANK_NONE + 1>> asg(T);
        std::vector<mcq_eval_stats> evs(T);
        auto slice = [&](unsigned t) {
            std::ostringstream ss;
            asg[t].fill(0);
            std::memset(&evs[t], 0, sizeof(evs[t]));
            for (uint64_t q = n * t / T; q < n * (t + 1) / T; ++q) {
                const uint32_t truth = !p.wants_truth() ? MCQ_NO_TAXON : (excluding() ? S.truth[q] : truth_of(S, q));
                write_query(ss, o, db.hitmin, S.text[0].p + S.hdr.p[2 * q], (size_t)(S.hdr.p[2 * q + 1] - S.hdr.p[2 * q]),
                            &S.cands.p[q * p.maxcand], S.ncand.p[q], asg[t].data(), truth, p.precision ? &evs[t] : nullptr);
            }
            out[t] = ss.str();
        };
        if (T == 1) slice(0);
        else {
            std::vector<std::thread> th;
            for (unsigned t = 0; t < T; ++t) th.emplace_back(slice, t);
            for (auto& x : th) x.join();
        }
        for (unsigned t = 0; t < T; ++t) {
            os->write(out[t].data(), (std::streamsize)out[t].size());
            for (int r = 0; r <= MCQ_RANK_NONE; ++r) assigned[r] += asg[t][r];
            mcq_eval_stats_add(&eval, &evs[t]);
        }
        return true;
    }
    // the lines of the units before `end` that have none yet: a batch's own unit, and units without records before it
    void announce(size_t end) { for (; announced < end; ++announced) write_unit_line(*os, o, p.units[announced]); }
    bool join() { return !pending.valid() || pending.get(); }
    void finish_next_beside() { const size_t r = retired++; pending = std::async(std::launch::async, [this, r] { return finish(r); }); }
    bool drain() {
        if (!join()) return false;
        for (; retired < issued; ++retired) if (!finish(retired)) return false;
        return true;
    }
    // a workspace for n queries; a larger one replaces it once the batches in flight are written (taxon counts carried over)
    bool ensure_ws(uint64_t n) {
        if (ws && ws_cap >= n) return true;
        if (!drain()) return false;
        uint64_t cap = 1024;
        while (cap < n) cap *= 2;
        cap = std::min<uint64_t>(std::max<uint64_t>(cap, n), std::max<uint64_t>(p.batch, n));
        if (ws && tx && !add_taxon_counts(ws, tax_counts)) return false;
        mcq_ws_destroy(ws); ws = nullptr;
        if (mcq_ws_create(db.edb, cap, 1, 0, &ws)) { std::fprintf(stderr, "ABORT: %s\n", mcq_last_error()); return false; }
        if (tx && mcq_ws_set_classify(ws, tx, &co)) { std::fprintf(stderr, "ABORT: %s\n", mcq_last_error()); return false; }
        if (excluding() && mcq_ws_set_exclusion(ws, tgt_clade.data(), (uint32_t)tgt_clade.size(), 0)) { std::fprintf(stderr, "ABORT: %s\n", mcq_last_error()); return false; }
        ws_cap = cap;
        return true;
    }
};

}  // namespace

// one output: the units of p through the GPU, head, mapping lines, tables and summary into p's -out file
static int run_queries(const Options& p, const Database& db) {
    const auto t_start = std::chrono::steady_clock::now();                  // the reference times map_queries_to_targets, readers included (src/mode_query.cpp:130-132)
    ReadBatcher reads(p.units, p.read_chunk, p.batch, p.batch_bases, p.host_reader, 0);
    Run run(p, db);
    if (!reads.ok() || !run.init()) return 1;
    const mcq_query_opts qo = query_opts(p);
    const int mates = p.paired() ? 2 : 1;
    for (;;) {
        Slot& S = run.slot[run.issued % NS];
        if (!run.join()) return 1;                               // batch j - 3 (this slot) is written
        if (run.issued >= 2) run.finish_next_beside();           // batch j - 2
        const ReadBatcher::Status got = reads.next(S);
        if (got == ReadBatcher::ERROR) return 1;
        if (got == ReadBatcher::END) break;
        const uint64_t n = S.n;
        if (!run.ensure_ws(n) || !S.d_cands.grow(n * p.maxcand) || !S.d_ncand.grow(n) || !S.cands.grow(n * p.maxcand) || !S.ncand.grow(n)) return 1;
        mcq_batch in; std::memset(&in, 0, sizeof(in));
        in.n_seqs = n * mates; in.bases = S.d_bases.p; in.seq_off = S.d_seq_off.p; in.paired = mates == 2; in.flags = MCQ_DEVICE_PTRS;
        mcq_result res; res.cands = S.d_cands.p; res.n_cand = S.d_ncand.p; res.flags = MCQ_DEVICE_PTRS;
        if (run.excluding() && !run.stage_clades(S, reads.stream())) return 1;
        MCQ_HIP(hipEventRecord(run.ev_in, reads.stream()), return 1);
        MCQ_HIP(hipStreamWaitEvent(run.s_k, run.ev_in, 0), return 1);
        if (mcq_query(db.edb, run.ws, &in, &qo, &res, run.s_k)) { std::fprintf(stderr, "FAIL: %s\n", mcq_last_error()); return 1; }
        MCQ_HIP(hipMemcpyAsync(S.cands.p, S.d_cands.p, n * p.maxcand * sizeof(mcq_cand), hipMemcpyDeviceToHost, run.s_k), return 1);
        MCQ_HIP(hipMemcpyAsync(S.ncand.p, S.d_ncand.p, n * 4, hipMemcpyDeviceToHost, run.s_k), return 1);
        if (!S.host_parsed && !run.excluding()) MCQ_HIP(hipMemcpyAsync(S.hdr.p, S.d_hdr.p, 2 * n * 8, hipMemcpyDeviceToHost, run.s_k), return 1);
        MCQ_HIP(hipEventRecord(S.done, run.s_k), return 1);
        ++run.issued;
    }
    if (!run.drain()) return 1;
    run.announce(p.units.size());
    if (run.tx) {
        if (run.ws && !add_taxon_counts(run.ws, run.tax_counts)) return 1;
        if (!write_abundances(*run.os, db.rdb, p, run.tax_counts, run.assigned)) return 1;
    }
    write_summary(*run.os, run.o, run.assigned, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count(),
                  p.precision ? &run.eval : nullptr);
    return 0;
}

int main(int argc, char** argv) {
    Options p;
    if (!parse_options(argc, argv, p)) return 2;
    if (p.list_inputs) { list_inputs(std::cout, p); return 0; }
    Database db;
    if (!open_database(p, db, 1, 0, 0)) return 1;
    if (p.split && !inputs_readable(p)) return 1;               // (one run: its ReadBatcher tries them all)
    for (const Options& r : output_runs(p))
        if (const int rc = run_queries(r, db)) return rc;
    return 0;
}
