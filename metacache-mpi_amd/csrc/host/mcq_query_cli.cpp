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
//
// -hits-per-seq (with -lowest sequence; above it the table has no rows and nothing of this runs): behind a batch's query, on the
// same stream, mcq_target_slots turns the batch's device results into slot targets (the sequence-level candidates with hits >=
// hitmin) and mcq_target_hits answers each with its window range and per-window counts, which come back with the results.  The
// width of the count rows is the range width of the batch's longest query, so the batch's offsets are looked at on the host first
// (Run::stage_hits).  The writer threads feed one accumulator each (mcq_hits_table_*), merged and written after the last
// mapping line; host memory grows with the input, as the reference's does.  A read beyond the kernel's capacity ends the run.
//
// -allhits: behind a batch's query, on the same stream, mcq_all_hits_count leaves the batch's segment offsets on the device; the host
// waits for their total, grows the device and pinned entry buffers to it, and enqueues mcq_all_hits and the copies out
// (Run::stage_all_hits).  The writer threads format the all_hits column from the pinned entries with the targets' names; with
// -exclude they leave out the entries on the read's own clade.  This host round trip is paid by -allhits alone.  A batch whose
// entries need more than 2 GiB, or a read beyond the kernel's capacity, ends the run.  Every slot has entry
// buffers of its own: up to three times 2 GiB on the device, and as much pinned.
//
// -align (with -lowest sequence; above it only the parameter line is written and nothing of this runs): the genome files the
// database names are read once at the start (mcq_align_subjects.hpp).  Behind a batch's query, on the same stream, the host waits
// for the batch's candidates, builds one job per read that is classified, whose first candidate is a sequence and whose target's
// bases are known -- the slice comes from that candidate's window range, which after a fold (n_ranks > 1) is (0,0) as in the
// reference's MPI program; -align-candidate-range first asks mcq_target_slots / mcq_target_hits (one slot) for the real range --,
// gathers the slices into a pinned buffer, copies them in, calls mcq_align and copies the results back (Run::stage_align).  This
// host round trip between the query and the alignment is paid by -align alone.  A read beyond the kernel's capacities ends the run.
//
// -coverage / -cov-percentile (not options of the reference): behind a batch's query, on the same stream,
// mcq_target_slots and mcq_target_hits as for -hits-per-seq -- with -hits-per-seq on, its very outputs -- and then mcq_coverage_add, which
// folds the ranges and count rows into a bitmap of windows and three numbers per sequence ON THE DEVICE (Coverage, Run::stage_cov):
// only status[] comes back, nothing grows with the input.  The candidates are taken at sequence level: under another -lowest the
// engine's candidates are taxa above it, so the table is made a second time with sequence-level keys (Database::seq_edb) and every
// batch is queried there too.  -cov-percentile P runs the input twice: pass 1 is query and coverage alone, without any output; then
// mcq_coverage_read and mcq_coverage_cut name the removed sequences; pass 2 is the ordinary run with the workspace's exclusion table
// set to 1 for removed and 0 for kept targets and the key 1 for every query, so a removed sequence is no candidate of any read.  The
// report shows pass 1's numbers, the ones the cut was made from.
#include "mcq_cli_common.hpp"
#include "mcq_read_batches.hpp"
#include "mcq_align_subjects.hpp"

#include <array>
#include <sstream>
#include <thread>

namespace {

// one of the three slots: a batch's input (mcq_read_batches.hpp) and its results
struct Slot : ReadSlot {
    DeviceBuf<mcq_cand> d_cands; DeviceBuf<uint32_t> d_ncand; PinnedBuf<mcq_cand> cands; PinnedBuf<uint32_t> ncand; Event done;
    std::vector<uint32_t> truth; PinnedBuf<uint32_t> clade; DeviceBuf<uint32_t> d_clade;   // -exclude: the truths and clade keys of the batch
    // -hits-per-seq: the batch's slot targets, and per slot the range and the counts of its windows (mcq_target_hits)
    DeviceBuf<uint32_t> d_tgt, d_cnt, d_hst; DeviceBuf<mcq_target_range> d_rng;
    PinnedBuf<uint32_t> cnt, hst; PinnedBuf<mcq_target_range> rng; PinnedBuf<uint64_t> seq_off;
    uint32_t range_cap = 0; bool hits = false;
    // -allhits: the batch's segment offsets, entries, entry counts and status words (mcq_all_hits)
    DeviceBuf<uint64_t> d_ah_off; DeviceBuf<mcq_hit> d_ah; DeviceBuf<uint32_t> d_ah_n, d_ah_st;
    PinnedBuf<uint64_t> ah_off; PinnedBuf<mcq_hit> ah; PinnedBuf<uint32_t> ah_n, ah_st;
    bool all_hits = false;
    // -coverage / -cov-percentile: the sequence-level candidates of the batch where the run's own are above it, and whether it was gathered
    DeviceBuf<mcq_cand> d_cands_seq; DeviceBuf<uint32_t> d_ncand_seq; bool cov = false;
    AlignSlot al;                                                                        // -align
    uint64_t first_id = 0;                                                               // query id of the batch's first query
};
constexpr int NS = 3;
constexpr uint64_t kAllHitsMaxEntries = (2ull << 30) / sizeof(mcq_hit);                  // -allhits: entries of one batch, so of one slot: NS times that in flight

// -coverage / -cov-percentile: the accumulator on the device and what was read from it, over all runs of one command line
struct Coverage {
    mcq_coverage* h = nullptr;
    std::vector<uint32_t> windows;                               // windows of every target
    std::vector<mcq_target_coverage> rec; uint64_t out_of_range = 0;   // what mcq_coverage_read gave
    std::vector<uint8_t> removed;                                // -cov-percentile: the cut; empty without
    std::vector<uint32_t> tgt_clade;                             // ... as the exclusion table of pass 2: 1 removed, 0 kept
    uint64_t skipped = 0;                                        // queries beyond mcq_target_hits' capacity: they added nothing
    bool gather = false;                                         // the runs to come add their batches
    ~Coverage() { mcq_coverage_free(h); }
    bool create(const Database& db) {
        mcq_refdb_info info; mcq_refdb_get_info(db.rdb, &info);
        windows.resize(info.n_targets);
        if (mcq_refdb_seq_windows(db.rdb, windows.data())) { std::fprintf(stderr, "ABORT: %s\n", mcq_host_last_error()); return false; }
        if (mcq_coverage_create(windows.data(), info.n_targets, 0, &h)) { std::fprintf(stderr, "ABORT: %s\n", mcq_last_error()); return false; }
        return true;
    }
    bool read() {
        rec.resize(windows.size());
        if (mcq_coverage_read(h, rec.data(), &out_of_range, nullptr)) { std::fprintf(stderr, "FAIL: %s\n", mcq_last_error()); return false; }
        return true;
    }
    // mcq_coverage_cut over what pass 1 gathered; one line on stderr
    bool cut(double percentile) {
        removed.assign(windows.size(), 0);
        if (mcq_coverage_cut(rec.data(), windows.data(), (uint32_t)windows.size(), percentile, removed.data())) { std::fprintf(stderr, "ABORT: %s\n", mcq_host_last_error()); return false; }
        uint64_t hit = 0, gone = 0;
        tgt_clade.assign(windows.size(), 0);
        for (size_t t = 0; t < windows.size(); ++t) { hit += rec[t].windows_covered > 0; gone += removed[t]; tgt_clade[t] = removed[t]; }
        std::fprintf(stderr, "coverage percentile %g: %llu of %llu hit sequences removed\n", percentile, (unsigned long long)gone, (unsigned long long)hit);
        return true;
    }
    // the report into the -coverage FILE if one was named, else into `os`
    bool write(const Options& p, const Out& o, std::ostream& os) {
        // (a row names its sequence whatever -lowest says: the lowest rank shown is the sequence's own)
        const mcq_taxon_print mode = {o.mode.rank_prefix ? 1u : 0u, (uint32_t)o.mode.body, p.lineage ? 1u : 0u, MCQ_RANK_SEQUENCE, p.highest};
        std::ofstream fc;
        if (!p.coverage_file.empty()) {
            fc.open(p.coverage_file);
            if (!fc.good()) { std::fprintf(stderr, "ABORT: Could not write to file %s\n", p.coverage_file.c_str()); return false; }
            std::cout << "Per-sequence coverage will be written to file: " << p.coverage_file << std::endl;
        }
        std::ostream& co = p.coverage_file.empty() ? os : fc;
        auto sink = [](void* user, const char* data, size_t n) -> int {
            std::ostream& out = *static_cast<std::ostream*>(user);
            out.write(data, (std::streamsize)n);
            return out.good() ? 0 : 1;
        };
        if (mcq_coverage_write(o.db, rec.data(), windows.data(), (uint32_t)windows.size(), removed.empty() ? nullptr : removed.data(), skipped,
                               out_of_range, o.comment, o.col, &mode, sink, &co)) { std::fprintf(stderr, "ABORT: %s\n", mcq_host_last_error()); return false; }
        co.flush();
        return co.good();
    }
};

// the batches in flight, the workspace they run in and what their lines add up to
struct Run {
    const Options& p; const Database& db; const Out o; const mcq_classify_opts co;
    Coverage* cov = nullptr; bool pass1 = false;                 // -coverage / -cov-percentile; pass1: query and coverage alone, no output
    mcq_ws* ws_seq = nullptr;                                    // ... the workspace of db.seq_edb
    DeviceBuf<uint32_t> d_ones; uint64_t n_ones = 0;             // -cov-percentile, pass 2: the key 1 for every query of a batch
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
    uint64_t next_id = 1;                                        // query ids: the 1-based running number of the read (pair) over all units of this output
    std::vector<mcq_hits_table*> hit_acc;                        // -hits-per-seq: one accumulator per writer thread
    DeviceBuf<uint32_t> d_tax2tgt; uint32_t n_taxa = 0, n_slots = 0;
    AlignSubjects subjects;                                      // -align: the sequences the database names, in host memory

    Run(const Options& p_, const Database& db_, Coverage* cov_ = nullptr, bool pass1_ = false)
        : p(p_), db(db_), o(make_out(db_.rdb, p_)), co(classify_opts(p_, db_.hitmin)), cov(cov_), pass1(pass1_) { std::memset(&eval, 0, sizeof(eval)); }
    ~Run() { if (pending.valid()) pending.wait(); mcq_ws_destroy(ws); mcq_ws_destroy(ws_seq); mcq_taxonomy_destroy(tx); for (mcq_hits_table* t : hit_acc) mcq_hits_table_free(t); }

    bool init() {
        if (pass1) {
            if (!make_tax2tgt()) return false;
            if (!s_k.create() || !ev_in.create()) return false;
            for (Slot& S : slot) if (!S.done.create()) return false;
            return true;
        }
        if (p.tax_counts()) {
            if (!(tx = make_taxonomy(db.rdb, 0))) return false;
            mcq_refdb_info rinfo; mcq_refdb_get_info(db.rdb, &rinfo);
            tax_counts.assign((size_t)rinfo.n_taxa + 1, 0);
        }
        if (excluding()) {
            tgt_clade.resize(db.t2t.size());
            if (mcq_refdb_clade_keys(db.rdb, p.exclude_rank, tgt_clade.data())) { std::fprintf(stderr, "ABORT: %s\n", mcq_host_last_error()); return false; }
        }
        if (p.hits_per_seq) {
            hit_acc.assign(std::max(1u, p.threads), nullptr);
            for (mcq_hits_table*& t : hit_acc) if (mcq_hits_table_create(&t)) return false;
        }
        if (align_on() && !subjects.load(db.rdb)) return false;
        if ((hits_on() || gather_on() || (align_on() && p.align_range && p.P > 1)) && !make_tax2tgt()) return false;   // candidates above sequence level are skipped: no kernel, no rows
        if (!s_k.create() || !ev_in.create()) return false;
        for (Slot& S : slot) if (!S.done.create()) return false;
        os = &open_out(p, fout);
        write_head(*os, o, db.hitmin);
        return true;
    }

    // what mcq_target_slots needs: the target of every sequence-level taxon, on the device
    bool make_tax2tgt() {
        mcq_refdb_info rinfo; mcq_refdb_get_info(db.rdb, &rinfo);
        std::vector<uint32_t> t2g(rinfo.n_taxa);
        if (mcq_refdb_tax2tgt(db.rdb, t2g.data())) { std::fprintf(stderr, "ABORT: %s\n", mcq_host_last_error()); return false; }
        n_taxa = rinfo.n_taxa; n_slots = std::min<uint32_t>(std::max(1u, p.maxcand), MCQ_TARGET_HITS_MAX_SLOTS);
        if (!d_tax2tgt.grow(n_taxa)) return false;
        MCQ_HIP(hipMemcpy(d_tax2tgt.p, t2g.data(), (size_t)n_taxa * 4, hipMemcpyHostToDevice), return false);
        return true;
    }
    bool gather_on() const { return cov && cov->gather; }        // this run's batches go into the coverage accumulator
    bool cut_on() const { return cov && !pass1 && !cov->tgt_clade.empty(); }   // pass 2: the removed sequences are excluded
    bool excluding() const { return p.exclude_rank != MCQ_RANK_NONE; }
    bool hits_on() const { return p.hits_per_seq && p.lowest == MCQ_RANK_SEQUENCE; }
    bool align_on() const { return p.align && !p.nomap && p.lowest == MCQ_RANK_SEQUENCE; }   // (no mapping lines, no blocks: nothing is aligned)
    // -align: behind the batch's query and the copies of its candidates on s_k.  The host waits for the candidates, makes the jobs,
    // gathers their subjects, and enqueues the copies in, mcq_align and the copies out on s_k (`st` has prepared the batch).
    bool stage_align(Slot& S, const mcq_batch& in, const mcq_result& res, hipStream_t st) {
        AlignSlot& A = S.al;
        const uint64_t n = S.n, ns = in.n_seqs;
        A.on = false;
        MCQ_HIP(hipStreamSynchronize(s_k), return false);       // the candidates are on the host
        const uint64_t* off = S.h_seq_off.data();
        if (!S.host_parsed) {
            if (!S.seq_off.grow(ns + 1)) return false;
            MCQ_HIP(hipMemcpyAsync(S.seq_off.p, S.d_seq_off.p, (ns + 1) * 8, hipMemcpyDeviceToHost, st), return false);
            MCQ_HIP(hipStreamSynchronize(st), return false);
            off = S.seq_off.p;
        }
        uint64_t longest_mate = 0, longest_query = 0;
        const uint64_t m = in.paired ? 2 : 1;
        for (uint64_t s = 0; s < ns; ++s) longest_mate = std::max(longest_mate, off[s + 1] - off[s]);
        for (uint64_t q = 0; q < n; ++q) longest_query = std::max(longest_query, off[m * q + m] - off[m * q]);
        if (!A.jobs.grow(n) || !A.d_jobs.grow(n) || !A.res.grow(n) || !A.d_res.grow(n)) return false;
        A.beg.assign(n, 0); A.end.assign(n, 0);
        // who is aligned, and to which windows
        std::vector<uint32_t> tgt(n, MCQ_NO_TAXON);
        uint64_t n_on = 0;
        for (uint64_t q = 0; q < n; ++q) {
            const mcq_cand* c = &S.cands.p[q * p.maxcand];
            const uint32_t nc = S.ncand.p[q];
            if (nc == 0 || mcq_refdb_classify(db.rdb, reinterpret_cast<const uint32_t*>(c), nc, db.hitmin, p.hitdiff, p.highest) == MCQ_NO_TAXON) continue;
            if (mcq_refdb_taxon_rank(db.rdb, c[0].tax) != MCQ_RANK_SEQUENCE) continue;
            tgt[q] = subjects.target_of(c[0].tax);
            if (tgt[q] == MCQ_NO_TAXON) continue;
            A.beg[q] = c[0].win_beg; A.end[q] = c[0].win_end;
            ++n_on;
        }
        if (n_on == 0) return true;
        if (p.align_range && p.P > 1) {                         // the fold has zeroed the positions: the top target's range once more
            const uint32_t cap = mcq_target_hits_range_cap(db.edb, longest_query, p.insertsize);
            if (!A.d_tgt.grow(n) || !A.d_rng.grow(n) || !A.rng.grow(n) || !A.d_cnt.grow(n * cap) || !A.d_hst.grow(n) || !A.hst.grow(n)) return false;
            if (mcq_target_slots(&res, n, p.maxcand, db.hitmin, d_tax2tgt.p, n_taxa, A.d_tgt.p, 1, s_k) ||
                mcq_target_hits(db.edb, ws, &in, A.d_tgt.p, 1, p.insertsize, cap, A.d_rng.p, A.d_cnt.p, A.d_hst.p, s_k)) {
                std::fprintf(stderr, "FAIL: %s\n", mcq_last_error()); return false;
            }
            MCQ_HIP(hipMemcpyAsync(A.rng.p, A.d_rng.p, n * sizeof(mcq_target_range), hipMemcpyDeviceToHost, s_k), return false);
            MCQ_HIP(hipMemcpyAsync(A.hst.p, A.d_hst.p, n * 4, hipMemcpyDeviceToHost, s_k), return false);
            MCQ_HIP(hipStreamSynchronize(s_k), return false);
            for (uint64_t q = 0; q < n; ++q) {
                if (tgt[q] == MCQ_NO_TAXON) continue;
                if (A.hst.p[q]) {
                    std::fprintf(stderr, "ABORT: -align-candidate-range: read %llu is beyond what mcq_target_hits takes\n", (unsigned long long)(S.first_id + q));
                    return false;
                }
                const mcq_target_range& r = A.rng.p[q];
                if (r.tgt == tgt[q] && r.n_win) { A.beg[q] = r.win_beg; A.end[q] = r.win_beg + r.n_win - 1; }
            }
        }
        uint64_t total = 0, longest_sub = 0;
        for (uint64_t q = 0; q < n; ++q) {
            mcq_align_job& j = A.jobs.p[q];
            j.sub_off = total; j.sub_len = 0; j.on = 0;
            if (tgt[q] == MCQ_NO_TAXON) continue;
            uint64_t o, l;
            subjects.slice(tgt[q], A.beg[q], A.end[q], o, l);
            j.on = 1; j.sub_len = (uint32_t)std::min<uint64_t>(l, 0xFFFFFFFFu);
            if (l <= MCQ_ALIGN_MAX_SUBJECT) { total += l; longest_sub = std::max(longest_sub, l); }     // (a longer one is reported by the kernel and never read)
        }
        if (!A.sub.grow(total + 1) || !A.d_sub.grow(total + 1)) return false;
        for (uint64_t q = 0; q < n; ++q) {
            const mcq_align_job& j = A.jobs.p[q];
            if (!j.on || j.sub_len > MCQ_ALIGN_MAX_SUBJECT) continue;
            uint64_t o, l;
            subjects.slice(tgt[q], A.beg[q], A.end[q], o, l);
            std::memcpy(A.sub.p + j.sub_off, subjects.bases.data() + o, l);
        }
        const uint32_t max_query = (uint32_t)std::min<uint64_t>(longest_mate, MCQ_ALIGN_MAX_QUERY), max_subject = (uint32_t)longest_sub;
        A.text_cap = std::max(1u, max_query + max_subject);
        const uint64_t text = n * (uint64_t)A.text_cap;
        if (!A.text_q.grow(text) || !A.text_s.grow(text) || !A.d_text_q.grow(text) || !A.d_text_s.grow(text)) return false;
        MCQ_HIP(hipMemcpyAsync(A.d_sub.p, A.sub.p, total, hipMemcpyHostToDevice, s_k), return false);
        MCQ_HIP(hipMemcpyAsync(A.d_jobs.p, A.jobs.p, n * sizeof(mcq_align_job), hipMemcpyHostToDevice, s_k), return false);
        if (mcq_align(ws, &in, A.d_sub.p, A.d_jobs.p, max_query, max_subject, A.d_res.p, A.d_text_q.p, A.d_text_s.p, A.text_cap, s_k)) {
            std::fprintf(stderr, "FAIL: %s\n", mcq_last_error()); return false;
        }
        MCQ_HIP(hipMemcpyAsync(A.res.p, A.d_res.p, n * sizeof(mcq_alignment), hipMemcpyDeviceToHost, s_k), return false);
        MCQ_HIP(hipMemcpyAsync(A.text_q.p, A.d_text_q.p, text, hipMemcpyDeviceToHost, s_k), return false);
        MCQ_HIP(hipMemcpyAsync(A.text_s.p, A.d_text_s.p, text, hipMemcpyDeviceToHost, s_k), return false);
        A.on = true;
        return true;
    }
    // -allhits: behind the batch's query on s_k.  Count, wait for the total, make room, emit, copy out.
    bool stage_all_hits(Slot& S, const mcq_batch& in) {
        const uint64_t n = S.n;
        if (!S.d_ah_off.grow(n + 1) || !S.ah_off.grow(n + 1) || !S.d_ah_n.grow(n) || !S.ah_n.grow(n) || !S.d_ah_st.grow(n) || !S.ah_st.grow(n)) return false;
        if (mcq_all_hits_count(db.edb, ws, &in, S.d_ah_off.p, s_k)) { std::fprintf(stderr, "FAIL: %s\n", mcq_last_error()); return false; }
        MCQ_HIP(hipMemcpyAsync(S.ah_off.p, S.d_ah_off.p, (n + 1) * 8, hipMemcpyDeviceToHost, s_k), return false);
        MCQ_HIP(hipStreamSynchronize(s_k), return false);
        const uint64_t total = S.ah_off.p[n];
        if (total > kAllHitsMaxEntries) {                        // 2 GiB of entries, on the device and pinned
            std::fprintf(stderr, "ABORT: -allhits needs %llu MB for the hits of a batch of %llu reads: use a smaller -batch\n",
                         (unsigned long long)((total * sizeof(mcq_hit)) >> 20), (unsigned long long)n);
            return false;
        }
        if (!S.d_ah.grow(std::max<uint64_t>(total, 1)) || !S.ah.grow(std::max<uint64_t>(total, 1))) return false;   // (a batch without any hit: still a buffer to name)
        if (mcq_all_hits(db.edb, ws, &in, S.d_ah_off.p, S.d_ah.p, total, S.d_ah_n.p, S.d_ah_st.p, s_k)) { std::fprintf(stderr, "FAIL: %s\n", mcq_last_error()); return false; }
        if (total) MCQ_HIP(hipMemcpyAsync(S.ah.p, S.d_ah.p, total * sizeof(mcq_hit), hipMemcpyDeviceToHost, s_k), return false);
        MCQ_HIP(hipMemcpyAsync(S.ah_n.p, S.d_ah_n.p, n * 4, hipMemcpyDeviceToHost, s_k), return false);
        MCQ_HIP(hipMemcpyAsync(S.ah_st.p, S.d_ah_st.p, n * 4, hipMemcpyDeviceToHost, s_k), return false);
        return true;
    }
    // -hits-per-seq: behind the batch's query on s_k, its slot targets, their ranges and window counts, and the copies out.  The count
    // rows are as wide as the range of the batch's longest query: its offsets come to the host first (`st` has prepared the batch).
    bool stage_hits(Slot& S, const mcq_batch& in, const mcq_result& res, hipStream_t st) {
        const uint64_t n = S.n, ns = in.n_seqs;
        const uint64_t* off = S.h_seq_off.data();
        if (!S.host_parsed) {
            if (!S.seq_off.grow(ns + 1)) return false;
            MCQ_HIP(hipMemcpyAsync(S.seq_off.p, S.d_seq_off.p, (ns + 1) * 8, hipMemcpyDeviceToHost, st), return false);
            MCQ_HIP(hipStreamSynchronize(st), return false);
            off = S.seq_off.p;
        }
        const uint64_t m = in.paired ? 2 : 1;
        uint64_t longest = 0;
        for (uint64_t q = 0; q < n; ++q) longest = std::max(longest, off[m * q + m] - off[m * q]);
        S.range_cap = mcq_target_hits_range_cap(db.edb, longest, p.insertsize);
        const uint64_t words = n * n_slots * S.range_cap;
        if (words > (1ull << 29)) {                              // 2 GiB of counts: one very long read among many
            std::fprintf(stderr, "ABORT: -hits-per-seq needs %llu MB for the window counts of a batch of %llu reads whose longest has %llu bases: "
                                 "use a smaller -batch\n", (unsigned long long)(words >> 18), (unsigned long long)n, (unsigned long long)longest);
            return false;
        }
        if (!S.d_tgt.grow(n * n_slots) || !S.d_rng.grow(n * n_slots) || !S.rng.grow(n * n_slots) || !S.d_cnt.grow(words) || !S.cnt.grow(words) ||
            !S.d_hst.grow(n) || !S.hst.grow(n)) return false;
        if (mcq_target_slots(&res, n, p.maxcand, db.hitmin, d_tax2tgt.p, n_taxa, S.d_tgt.p, n_slots, s_k) ||
            mcq_target_hits(db.edb, ws, &in, S.d_tgt.p, n_slots, p.insertsize, S.range_cap, S.d_rng.p, S.d_cnt.p, S.d_hst.p, s_k)) {
            std::fprintf(stderr, "FAIL: %s\n", mcq_last_error()); return false;
        }
        MCQ_HIP(hipMemcpyAsync(S.rng.p, S.d_rng.p, n * n_slots * sizeof(mcq_target_range), hipMemcpyDeviceToHost, s_k), return false);
        MCQ_HIP(hipMemcpyAsync(S.cnt.p, S.d_cnt.p, words * 4, hipMemcpyDeviceToHost, s_k), return false);
        MCQ_HIP(hipMemcpyAsync(S.hst.p, S.d_hst.p, n * 4, hipMemcpyDeviceToHost, s_k), return false);
        return true;
    }
    // -coverage / -cov-percentile: behind the batch's query on s_k (`res`: its sequence-level candidates on `gdb` / `gws`).  With
    // -hits-per-seq on, stage_hits has made the ranges and count rows already; else they are made here and stay on the device.  Only
    // status[] comes back.
    bool stage_cov(Slot& S, const mcq_batch& in, const mcq_result& res, const mcq_db* gdb, mcq_ws* gws, hipStream_t st) {
        const uint64_t n = S.n, ns = in.n_seqs;
        if (!S.hits) {
            const uint64_t* off = S.h_seq_off.data();
            if (!S.host_parsed) {
                if (!S.seq_off.grow(ns + 1)) return false;
                MCQ_HIP(hipMemcpyAsync(S.seq_off.p, S.d_seq_off.p, (ns + 1) * 8, hipMemcpyDeviceToHost, st), return false);
                MCQ_HIP(hipStreamSynchronize(st), return false);
                off = S.seq_off.p;
            }
            const uint64_t m = in.paired ? 2 : 1;
            uint64_t longest = 0;
            for (uint64_t q = 0; q < n; ++q) longest = std::max(longest, off[m * q + m] - off[m * q]);
            S.range_cap = mcq_target_hits_range_cap(gdb, longest, p.insertsize);
            const uint64_t words = n * n_slots * S.range_cap;
            if (words > (1ull << 29)) {                          // 2 GiB of counts: one very long read among many
                std::fprintf(stderr, "ABORT: -coverage needs %llu MB for the window counts of a batch of %llu reads whose longest has %llu bases: "
                                     "use a smaller -batch\n", (unsigned long long)(words >> 18), (unsigned long long)n, (unsigned long long)longest);
                return false;
            }
            if (!S.d_tgt.grow(n * n_slots) || !S.d_rng.grow(n * n_slots) || !S.d_cnt.grow(words) || !S.d_hst.grow(n) || !S.hst.grow(n)) return false;
            if (mcq_target_slots(&res, n, p.maxcand, db.hitmin, d_tax2tgt.p, n_taxa, S.d_tgt.p, n_slots, s_k) ||
                mcq_target_hits(gdb, gws, &in, S.d_tgt.p, n_slots, p.insertsize, S.range_cap, S.d_rng.p, S.d_cnt.p, S.d_hst.p, s_k)) {
                std::fprintf(stderr, "FAIL: %s\n", mcq_last_error()); return false;
            }
            MCQ_HIP(hipMemcpyAsync(S.hst.p, S.d_hst.p, n * 4, hipMemcpyDeviceToHost, s_k), return false);
        }
        if (mcq_coverage_add(cov->h, S.d_rng.p, S.d_cnt.p, n, n_slots, S.range_cap, s_k)) { std::fprintf(stderr, "FAIL: %s\n", mcq_last_error()); return false; }
        S.cov = true;
        return true;
    }
    // -cov-percentile, pass 2: every query of the batch carries the key 1, the key of the removed sequences
    bool stage_ones(uint64_t n) {
        if (n > n_ones) {
            MCQ_HIP(hipStreamSynchronize(s_k), return false);    // (batches in flight read the array that grow() replaces)
            if (!d_ones.grow(n)) return false;
            const std::vector<uint32_t> ones(n, 1u);
            MCQ_HIP(hipMemcpy(d_ones.p, ones.data(), n * 4, hipMemcpyHostToDevice), return false);
            n_ones = n;
        }
        if (mcq_ws_set_query_clades(ws, d_ones.p, n, MCQ_DEVICE_PTRS)) { std::fprintf(stderr, "FAIL: %s\n", mcq_last_error()); return false; }
        return true;
    }
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
        const uint64_t n = S.n;
        if (S.cov && !S.hits) for (uint64_t q = 0; q < n; ++q) if (S.hst.p[q]) ++cov->skipped;   // beyond mcq_target_hits' capacity: it added nothing, and is counted
        if (pass1) return true;
        announce(S.unit + 1);
        if (S.hits) for (uint64_t q = 0; q < n; ++q) if (S.hst.p[q]) {        // beyond mcq_target_hits' capacity: reported, never dropped in silence
            std::fprintf(stderr, "ABORT: -hits-per-seq: read %llu (%.*s) %s\n", (unsigned long long)(S.first_id + q),
                         (int)(S.hdr.p[2 * q + 1] - S.hdr.p[2 * q]), S.text[0].p + S.hdr.p[2 * q],
                         (S.hst.p[q] & MCQ_TARGET_HITS_KEYS) ? ("hits more than " + std::to_string(MCQ_TARGET_HITS_MAX_KEYS) + " (MCQ_TARGET_HITS_MAX_KEYS) distinct windows of its candidate sequences").c_str()
                                                             : "is beyond what mcq_target_hits takes (range width, window ids of 2^28 and more, 2^31 bases)");
            return false;
        }
        if (S.all_hits) for (uint64_t q = 0; q < n; ++q) if (S.ah_st.p[q]) {      // beyond mcq_all_hits' capacity: reported, never dropped in silence
            std::fprintf(stderr, "ABORT: -allhits: read %llu (%.*s) %s\n", (unsigned long long)(S.first_id + q),
                         (int)(S.hdr.p[2 * q + 1] - S.hdr.p[2 * q]), S.text[0].p + S.hdr.p[2 * q],
                         (S.ah_st.p[q] & MCQ_ALL_HITS_LOCS) ? "has more locations than the workspace takes (max_locs_per_query), or 2^31 bases or more"
                                                            : "was not answered by mcq_all_hits (its segment of the entry buffer does not fit its locations)");
            return false;
        }
        if (S.al.on) for (uint64_t q = 0; q < n; ++q) if (S.al.res.p[q].status) {   // beyond mcq_align's capacity: reported, never dropped in silence
            std::fprintf(stderr, "ABORT: -align: read %llu (%.*s) %s\n", (unsigned long long)(S.first_id + q),
                         (int)(S.hdr.p[2 * q + 1] - S.hdr.p[2 * q]), S.text[0].p + S.hdr.p[2 * q],
                         (S.al.res.p[q].status & MCQ_ALIGN_QUERY_LONG) ? ("has a mate of more than " + std::to_string(MCQ_ALIGN_MAX_QUERY) + " (MCQ_ALIGN_MAX_QUERY) bases").c_str()
                                                                      : ("has a candidate window range of more than " + std::to_string(MCQ_ALIGN_MAX_SUBJECT) + " (MCQ_ALIGN_MAX_SUBJECT) bases").c_str());
            return false;
        }
        const unsigned T = (unsigned)std::min<uint64_t>(std::max(1u, p.threads), std::max<uint64_t>(1, n / 64));
        std::vector<std::string> out(T);
        std::vector<std::array<uint64_t, MCQ_RANK_NONE + 1>> asg(T);
        std::vector<mcq_eval_stats> evs(T);
        std::vector<char> add_failed(T, 0);                                       // -hits-per-seq: a thread's accumulator refused an entry
        auto slice = [&](unsigned t) {
            std::ostringstream ss;
            asg[t].fill(0);
            std::memset(&evs[t], 0, sizeof(evs[t]));
            for (uint64_t q = n * t / T; q < n * (t + 1) / T; ++q) {
                const uint32_t truth = !p.wants_truth() ? MCQ_NO_TAXON : (excluding() ? S.truth[q] : truth_of(S, q));
                AlignBlock ab;
                if (S.al.on && S.al.res.p[q].length) {
                    const mcq_alignment& r = S.al.res.p[q];
                    const uint32_t key = S.cands.p[q * p.maxcand].tax;
                    const uint64_t w = subjects.winstride;
                    ab.score = r.score; ab.length = r.length;
                    ab.file = mcq_refdb_taxon_file(db.rdb, key); ab.index = mcq_refdb_taxon_index(db.rdb, key);
                    ab.range_beg = w * S.al.beg[q]; ab.range_end = w * S.al.end[q] + w;
                    ab.query = S.al.text_q.p + q * (uint64_t)S.al.text_cap; ab.target = S.al.text_s.p + q * (uint64_t)S.al.text_cap;
                }
                AllHits ah;
                if (S.all_hits) {
                    ah.e = S.ah.p + S.ah_off.p[q]; ah.n = S.ah_n.p[q]; ah.tgt_key = db.t2t.data();
                    if (excluding()) { ah.tgt_clade = tgt_clade.data(); ah.query_clade = S.clade.p[q]; }
                }
                write_query(ss, o, db.hitmin, S.text[0].p + S.hdr.p[2 * q], (size_t)(S.hdr.p[2 * q + 1] - S.hdr.p[2 * q]),
                            &S.cands.p[q * p.maxcand], S.ncand.p[q], asg[t].data(), truth, p.precision ? &evs[t] : nullptr, S.first_id + q,
                            ab.length ? &ab : nullptr, S.all_hits ? &ah : nullptr);
                if (S.hits) for (uint32_t s = 0; s < n_slots; ++s) {        // matches_per_target::insert of this read's candidates
                    const mcq_target_range& r = S.rng.p[q * n_slots + s];
                    if (r.tgt != MCQ_TARGET_UNUSED && r.n_win &&
                        mcq_hits_table_add(hit_acc[t], S.first_id + q, r.tgt, r.win_beg, r.n_win, &S.cnt.p[(q * n_slots + s) * (uint64_t)S.range_cap]))
                        add_failed[t] = 1;
                }
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
            if (add_failed[t]) { std::fprintf(stderr, "ABORT: -hits-per-seq: an entry of batch %zu could not be kept\n", j); return false; }
        }
        return true;
    }
    // -hits-per-seq: the writer threads' accumulators merged, sorted and written (show_matches_per_targets) into the -hits-per-seq FILE
    // if one was named, else behind the mapping lines
    bool write_hits_table() {
        for (size_t t = 1; t < hit_acc.size(); ++t) mcq_hits_table_merge(hit_acc[0], hit_acc[t]);
        const mcq_taxon_print mode = {o.mode.rank_prefix ? 1u : 0u, (uint32_t)o.mode.body, p.lineage ? 1u : 0u, p.lowest, p.highest};
        std::ofstream fh;
        if (!p.hits_file.empty()) {
            fh.open(p.hits_file);
            if (!fh.good()) { std::fprintf(stderr, "ABORT: Could not write to file %s\n", p.hits_file.c_str()); return false; }
            std::cout << "Per-Target mappings will be written to file: " << p.hits_file << std::endl;
        }
        std::ostream& ho = p.hits_file.empty() ? *os : fh;
        auto sink = [](void* user, const char* data, size_t n) -> int {          // row by row: the table is formatted once and never held whole
            std::ostream& out = *static_cast<std::ostream*>(user);
            out.write(data, (std::streamsize)n);
            return out.good() ? 0 : 1;
        };
        if (mcq_hits_table_write(hit_acc[0], db.rdb, o.comment, o.col, &mode, sink, &ho)) { std::fprintf(stderr, "ABORT: %s\n", mcq_host_last_error()); return false; }
        return ho.good();
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
        if (cut_on() && mcq_ws_set_exclusion(ws, cov->tgt_clade.data(), (uint32_t)cov->tgt_clade.size(), 0)) { std::fprintf(stderr, "ABORT: %s\n", mcq_last_error()); return false; }
        if (gather_on() && db.seq_edb) {                         // the sequence-level twin, under the same exclusion
            mcq_ws_destroy(ws_seq); ws_seq = nullptr;
            if (mcq_ws_create(db.seq_edb, cap, 1, 0, &ws_seq)) { std::fprintf(stderr, "ABORT: %s\n", mcq_last_error()); return false; }
            if (excluding() && mcq_ws_set_exclusion(ws_seq, tgt_clade.data(), (uint32_t)tgt_clade.size(), 0)) { std::fprintf(stderr, "ABORT: %s\n", mcq_last_error()); return false; }
        }
        ws_cap = cap;
        return true;
    }
};

}  // namespace

// one output: the units of p through the GPU, head, mapping lines, tables and summary into p's -out file
// (cov: the coverage accumulator of the command line, or none; pass1: query and coverage alone, nothing is written; report: the
//  coverage report belongs into this run's output)
static int run_queries(const Options& p, const Database& db, Coverage* cov = nullptr, bool pass1 = false, bool report = false) {
    const auto t_start = std::chrono::steady_clock::now();                  // the reference times map_queries_to_targets, readers included (src/mode_query.cpp:130-132)
    ReadBatcher reads(p.units, p.read_chunk, p.batch, p.batch_bases, p.host_reader, 0);
    Run run(p, db, cov, pass1);
    if (!reads.ok() || !run.init()) return 1;
    const bool gather = run.gather_on();
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
        S.first_id = run.next_id; run.next_id += n; S.hits = !pass1 && run.hits_on(); S.cov = false;
        if (!run.ensure_ws(n) || !S.d_cands.grow(n * p.maxcand) || !S.d_ncand.grow(n) || !S.cands.grow(n * p.maxcand) || !S.ncand.grow(n)) return 1;
        mcq_batch in; std::memset(&in, 0, sizeof(in));
        in.n_seqs = n * mates; in.bases = S.d_bases.p; in.seq_off = S.d_seq_off.p; in.paired = mates == 2; in.flags = MCQ_DEVICE_PTRS;
        mcq_result res; res.cands = S.d_cands.p; res.n_cand = S.d_ncand.p; res.flags = MCQ_DEVICE_PTRS;
        if (run.excluding() && !run.stage_clades(S, reads.stream())) return 1;
        MCQ_HIP(hipEventRecord(run.ev_in, reads.stream()), return 1);
        MCQ_HIP(hipStreamWaitEvent(run.s_k, run.ev_in, 0), return 1);
        const bool seq_twin = gather && db.seq_edb;             // the run's candidates are above sequence level: coverage asks the twin
        if (!(pass1 && seq_twin)) {
            if (run.cut_on() && !run.stage_ones(n)) return 1;
            if (mcq_query(db.edb, run.ws, &in, &qo, &res, run.s_k)) { std::fprintf(stderr, "FAIL: %s\n", mcq_last_error()); return 1; }
        }
        if (!pass1) {
            MCQ_HIP(hipMemcpyAsync(S.cands.p, S.d_cands.p, n * p.maxcand * sizeof(mcq_cand), hipMemcpyDeviceToHost, run.s_k), return 1);
            MCQ_HIP(hipMemcpyAsync(S.ncand.p, S.d_ncand.p, n * 4, hipMemcpyDeviceToHost, run.s_k), return 1);
            if (!S.host_parsed && !run.excluding()) MCQ_HIP(hipMemcpyAsync(S.hdr.p, S.d_hdr.p, 2 * n * 8, hipMemcpyDeviceToHost, run.s_k), return 1);
        }
        if (S.hits && !run.stage_hits(S, in, res, reads.stream())) return 1;
        if (gather) {
            mcq_result gres = res;
            if (seq_twin) {
                if (!S.d_cands_seq.grow(n * p.maxcand) || !S.d_ncand_seq.grow(n)) return 1;
                gres.cands = S.d_cands_seq.p; gres.n_cand = S.d_ncand_seq.p;
                if (run.excluding() && mcq_ws_set_query_clades(run.ws_seq, S.d_clade.p, n, MCQ_DEVICE_PTRS)) { std::fprintf(stderr, "FAIL: %s\n", mcq_last_error()); return 1; }
                if (mcq_query(db.seq_edb, run.ws_seq, &in, &qo, &gres, run.s_k)) { std::fprintf(stderr, "FAIL: %s\n", mcq_last_error()); return 1; }
            }
            if (!run.stage_cov(S, in, gres, seq_twin ? db.seq_edb : db.edb, seq_twin ? run.ws_seq : run.ws, reads.stream())) return 1;
        }
        S.all_hits = !pass1 && p.allhits && !p.nomap;
        if (S.all_hits && !run.stage_all_hits(S, in)) return 1;
        S.al.on = false;
        if (!pass1 && run.align_on() && !run.stage_align(S, in, res, reads.stream())) return 1;
        MCQ_HIP(hipEventRecord(S.done, run.s_k), return 1);
        ++run.issued;
    }
    if (!run.drain()) return 1;
    if (pass1) return 0;
    run.announce(p.units.size());
    if (p.hits_per_seq && !run.write_hits_table()) return 1;     // before the abundance tables: src/classification.cpp:847-862
    if (report) {                                                // behind the table, in front of the abundance tables
        if (gather && !cov->read()) return 1;
        if (!cov->write(p, run.o, *run.os)) return 1;
    }
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
    Coverage cov;
    if (p.cov_on()) {
        if (!cov.create(db)) return 1;
        if (p.lowest != MCQ_RANK_SEQUENCE && !open_seq_twin(p, db)) return 1;
    }
    if (p.cov_cut()) {                                          // pass 1: all units as one input, query and coverage alone
        Options one = p; one.split = false;
        cov.gather = true;
        if (const int rc = run_queries(one, db, &cov, true)) return rc;
        if (!cov.read() || !cov.cut(p.cov_percentile)) return 1;
        mcq_db_destroy(db.seq_edb); db.seq_edb = nullptr;      // pass 2 gathers nothing
    }
    cov.gather = p.coverage && !p.cov_cut();
    // (a run of -splitout has no report of its own: split_options; the accumulator goes with every run all the same)
    for (const Options& r : output_runs(p))
        if (const int rc = run_queries(r, db, p.cov_on() ? &cov : nullptr, false, p.coverage && !p.split)) return rc;
    if (p.coverage && p.split) {                                // over all units together, written once: into FILE, else to stdout
        if (cov.gather && !cov.read()) return 1;
        if (!cov.write(p, make_out(db.rdb, p), std::cout)) return 1;
    }
    return 0;
}
