// mcq_query_cli -- `metacache query <db> r1.fq r2.fq -pairfiles ...` on one GPU: see mcq_cli_common.hpp for what is
// written and which reference code each part stands in for.
//
// The reads stream through three buffer sets in rotation.  For batch j: read() a chunk of each file
// into set j % 3's pinned buffers (the bytes that the last batch did not use first), copy it to the GPU and index and
// compact it there (mcq_reads_prepare; a chunk not in the strict form is parsed on the host instead, mcq_reads_parse),
// carry the rest of the chunk into the next one, then mcq_query on the device buffers and copy the candidates back.  The
// mapping lines of batch j - 2 are formatted meanwhile, by -threads host threads, from the header ranges into the host
// copy of its chunk.  Host memory is fixed by -read-chunk and -batch: a file with no complete record in a chunk gets a
// buffer twice as large, once.
#include "mcq_cli_common.hpp"

#include <array>
#include <future>
#include <sstream>
#include <thread>

#include <hip/hip_runtime.h>

#define CLI_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "FAIL: %s: %s\n", #x, hipGetErrorString(e_)); return false; } } while (0)

namespace {

template <class T> bool grow_host(T*& p, uint64_t& cap, uint64_t need) {          // pinned, contents not kept
    if (cap >= need) return true;
    if (p) CLI_HIP(hipHostFree(p));
    p = nullptr; cap = 0;
    CLI_HIP(hipHostMalloc((void**)&p, std::max<uint64_t>(1, need) * sizeof(T), hipHostMallocDefault));
    cap = need;
    return true;
}
template <class T> bool grow_dev(T*& p, uint64_t& cap, uint64_t need) {
    if (cap >= need) return true;
    if (p) CLI_HIP(hipFree(p));
    p = nullptr; cap = 0;
    CLI_HIP(hipMalloc((void**)&p, std::max<uint64_t>(1, need) * sizeof(T)));
    cap = need;
    return true;
}

// one of the three sets: a batch's text, its device copy and batch, its results
struct Set {
    char* text[2] = {nullptr, nullptr}; uint64_t text_cap[2] = {0, 0}, len[2] = {0, 0};
    char* d_text[2] = {nullptr, nullptr}; uint64_t d_text_cap[2] = {0, 0};
    char* d_bases = nullptr; uint64_t d_bases_cap = 0;
    uint64_t *d_seq_off = nullptr, *d_hdr = nullptr, *d_info = nullptr; uint64_t d_seq_cap = 0, d_hdr_cap = 0, d_info_cap = 0;
    char* d_scratch = nullptr; uint64_t d_scratch_cap = 0;
    mcq_cand* d_cands = nullptr; uint32_t* d_ncand = nullptr; uint64_t d_cands_cap = 0, d_ncand_cap = 0;
    mcq_cand* cands = nullptr; uint32_t* ncand = nullptr; uint64_t* hdr = nullptr; uint64_t* info = nullptr;
    uint64_t cands_cap = 0, ncand_cap = 0, hdr_cap = 0, info_cap = 0;
    std::vector<char> h_bases; std::vector<uint64_t> h_seq_off;       // a chunk parsed on the host
    uint64_t n = 0; bool host_parsed = false;
    hipEvent_t done = nullptr;
    void release() {
        for (int m = 0; m < 2; ++m) { if (text[m]) (void)hipHostFree(text[m]); if (d_text[m]) (void)hipFree(d_text[m]); }
        for (void* d : {(void*)d_bases, (void*)d_seq_off, (void*)d_hdr, (void*)d_info, (void*)d_scratch, (void*)d_cands, (void*)d_ncand}) if (d) (void)hipFree(d);
        for (void* h : {(void*)cands, (void*)ncand, (void*)hdr, (void*)info}) if (h) (void)hipHostFree(h);
        if (done) (void)hipEventDestroy(done);
    }
};

}  // namespace

int main(int argc, char** argv) {
    Options p;
    if (!parse_options(argc, argv, p)) return 2;
    mcq_refdb* rdb = nullptr; std::vector<uint32_t> t2t; uint32_t hitmin = 0;
    mcq_db* edb = nullptr;
    if (!open_database(p, &rdb, t2t, &edb, hitmin, 1, 0, 0)) return 1;

    const auto t_start = std::chrono::steady_clock::now();                  // the reference times map_queries_to_targets, readers included (src/mode_query.cpp:130-132)
    const bool paired = p.paired();
    const int mates = paired ? 2 : 1;
    mcq_read_stream* rs[2] = {nullptr, nullptr};
    for (int m = 0; m < mates; ++m)
        if (mcq_read_stream_open(m ? p.f2.c_str() : p.f1.c_str(), &rs[m])) { std::fprintf(stderr, "FAIL: can't open file %s\n", (m ? p.f2 : p.f1).c_str()); return 1; }

    mcq_query_opts qo; qo.max_cand = p.maxcand; qo.emulate_ranks = p.P; qo.insert_size_max = p.insertsize;
    qo.flags = p.quirks ? MCQ_QUIRK_SEQ_DROP : 0;
    const mcq_classify_opts co = classify_opts(p, hitmin);
    mcq_taxonomy* tx = nullptr;                                 // -abundances / -abundance-per: every batch is also classified on the GPU
    if (p.tax_counts() && !(tx = make_taxonomy(rdb, 0))) return 1;
    mcq_refdb_info rinfo; mcq_refdb_get_info(rdb, &rinfo);
    std::vector<uint64_t> tax_counts(p.tax_counts() ? (size_t)rinfo.n_taxa + 1 : 0, 0);
    mcq_ws* ws = nullptr; uint64_t ws_cap = 0;

    std::ofstream fout; if (!p.outfile.empty()) fout.open(p.outfile);
    std::ostream& os = p.outfile.empty() ? std::cout : fout;
    const Out o = make_out(rdb, p);
    write_head(os, o, p, hitmin);
    uint64_t assigned[MCQ_RANK_NONE + 1] = {0};
    const unsigned n_threads = std::max(1u, p.threads);

    constexpr int NS = 3;
    Set set[NS];
    hipStream_t s_in = nullptr, s_k = nullptr;
    hipEvent_t ev_in = nullptr;
    auto init = [&]() -> bool {
        CLI_HIP(hipSetDevice(0));
        CLI_HIP(hipStreamCreateWithFlags(&s_in, hipStreamNonBlocking));
        CLI_HIP(hipStreamCreateWithFlags(&s_k, hipStreamNonBlocking));
        CLI_HIP(hipEventCreateWithFlags(&ev_in, hipEventDisableTiming));
        for (Set& S : set) CLI_HIP(hipEventCreateWithFlags(&S.done, hipEventDisableTiming));
        return true;
    };
    if (!init()) return 1;

    // the mapping lines of batch j, in input order: -threads slices, each into a string of its own, written in order
    auto finish = [&](size_t j) -> bool {
        Set& S = set[j % NS];
        if (hipEventSynchronize(S.done) != hipSuccess) { std::fprintf(stderr, "FAIL: batch %zu did not complete\n", j); return false; }
        const uint64_t n = S.n;
        const unsigned T = (unsigned)std::min<uint64_t>(n_threads, std::max<uint64_t>(1, n / 64));
        std::vector<std::string> out(T);
        std::vector<std::array<uint64_t, MCQ_RANK_NONE + 1>> asg(T);
        auto slice = [&](unsigned t) {
            std::ostringstream ss;
            asg[t].fill(0);
            for (uint64_t q = n * t / T; q < n * (t + 1) / T; ++q)
                write_query(ss, o, p, hitmin, S.text[0] + S.hdr[2 * q], (size_t)(S.hdr[2 * q + 1] - S.hdr[2 * q]),
                            &S.cands[q * p.maxcand], S.ncand[q], asg[t].data());
            out[t] = ss.str();
        };
        if (T == 1) slice(0);
        else {
            std::vector<std::thread> th;
            for (unsigned t = 0; t < T; ++t) th.emplace_back(slice, t);
            for (auto& x : th) x.join();
        }
        for (unsigned t = 0; t < T; ++t) {
            os.write(out[t].data(), (std::streamsize)out[t].size());
            for (int r = 0; r <= MCQ_RANK_NONE; ++r) assigned[r] += asg[t][r];
        }
        return true;
    };
    size_t issued = 0, retired = 0;                              // batches enqueued; batches whose lines are written or being written
    std::future<bool> pending;                                   // the formatting of batch `retired - 1`, beside the reading of the next
    auto join = [&]() -> bool { return !pending.valid() || pending.get(); };
    auto drain = [&]() -> bool {
        if (!join()) return false;
        for (; retired < issued; ++retired) if (!finish(retired)) return false;
        return true;
    };
    // a workspace for n queries; a larger one replaces it once the batches in flight are written (taxon counts carried over)
    auto ensure_ws = [&](uint64_t n) -> bool {
        if (ws && ws_cap >= n) return true;
        if (!drain()) return false;
        uint64_t cap = 1024;
        while (cap < n) cap *= 2;
        cap = std::min<uint64_t>(std::max<uint64_t>(cap, n), std::max<uint64_t>(p.batch, n));
        if (ws) {
            if (tx) {
                std::vector<uint64_t> c(tax_counts.size());
                if (mcq_ws_taxon_counts(ws, c.data(), 0)) { std::fprintf(stderr, "ABORT: %s\n", mcq_last_error()); return false; }
                for (size_t i = 0; i < c.size(); ++i) tax_counts[i] += c[i];
            }
            mcq_ws_destroy(ws); ws = nullptr;
        }
        if (mcq_ws_create(edb, cap, 1, 0, &ws)) { std::fprintf(stderr, "ABORT: %s\n", mcq_last_error()); return false; }
        if (tx && mcq_ws_set_classify(ws, tx, &co)) { std::fprintf(stderr, "ABORT: %s\n", mcq_last_error()); return false; }
        ws_cap = cap;
        return true;
    };

    uint64_t want[2] = {p.read_chunk, p.read_chunk}, carry[2] = {0, 0};
    bool ok = true, at_end = false;
    while (ok && !at_end) {
        const size_t j = issued;
        Set& S = set[j % NS];
        if (!(ok = join())) break;                               // batch j - 3 (this set) is written
        if (j >= 2) { const size_t r = retired++; pending = std::async(std::launch::async, finish, r); }
        // read, prepare; a chunk without a complete record in some file is read again into a buffer twice as large
        for (;;) {
            int32_t eof[2] = {0, 0};
            uint32_t flags = 0;
            char* old[2] = {nullptr, nullptr};
            for (int m = 0; m < mates; ++m) {
                const uint64_t need = std::max(want[m], carry[m]);
                if (S.text_cap[m] < need) {                      // (the old buffer may hold the carry: freed after the fill)
                    old[m] = S.text[m]; S.text[m] = nullptr; S.text_cap[m] = 0;
                    if (!grow_host(S.text[m], S.text_cap[m], need)) return 1;
                }
            }
            auto fill = [&](int m) { return mcq_read_stream_fill(rs[m], S.text[m], S.text_cap[m], std::max(want[m], carry[m]), &S.len[m], &eof[m]); };
            std::future<int> fill2;                              // the two files side by side
            if (paired) fill2 = std::async(std::launch::async, fill, 1);
            int rc = fill(0);
            if (paired && fill2.get()) rc = -1;
            if (rc) { std::fprintf(stderr, "FAIL: reading the read files\n"); return 1; }
            for (int m = 0; m < mates; ++m) {
                if (old[m] && hipHostFree(old[m]) != hipSuccess) return 1;
                if (eof[m]) flags |= (m ? MCQ_READS_EOF2 : MCQ_READS_EOF1);
            }
            const uint64_t L1 = S.len[0], L2 = paired ? S.len[1] : 0;
            const uint64_t qcap = std::min<uint64_t>(p.batch, std::min(L1, paired ? L2 : L1) / 2 + 2);
            if (!grow_host(S.hdr, S.hdr_cap, 2 * qcap) || !grow_host(S.info, S.info_cap, MCQ_READS_INFO_WORDS)) return 1;
            if (!grow_dev(S.d_bases, S.d_bases_cap, L1 + L2 + 1) || !grow_dev(S.d_seq_off, S.d_seq_cap, 2 * qcap + 1)) return 1;
            bool on_host = p.host_reader;
            if (!on_host) {
                const uint64_t sb = mcq_reads_scratch_bytes(L1, L2, qcap);
                if (!grow_dev(S.d_scratch, S.d_scratch_cap, sb) || !grow_dev(S.d_hdr, S.d_hdr_cap, 2 * qcap) ||
                    !grow_dev(S.d_info, S.d_info_cap, MCQ_READS_INFO_WORDS)) return 1;
                for (int m = 0; m < mates; ++m) {
                    if (!grow_dev(S.d_text[m], S.d_text_cap[m], S.len[m] + 1)) return 1;
                    if (S.len[m] && hipMemcpyAsync(S.d_text[m], S.text[m], S.len[m], hipMemcpyHostToDevice, s_in) != hipSuccess) return 1;
                }
                if (mcq_reads_prepare(S.d_text[0], L1, paired ? S.d_text[1] : nullptr, L2, flags, qcap, p.batch_bases, S.d_scratch, sb,
                                      S.d_bases, S.d_seq_off, S.d_hdr, S.d_info, s_in)) { std::fprintf(stderr, "FAIL: %s\n", mcq_last_error()); return 1; }
                if (hipMemcpyAsync(S.info, S.d_info, MCQ_READS_INFO_WORDS * 8, hipMemcpyDeviceToHost, s_in) != hipSuccess ||
                    hipStreamSynchronize(s_in) != hipSuccess) { std::fprintf(stderr, "FAIL: reading on the GPU\n"); return 1; }
                on_host = (S.info[MCQ_READS_STATUS] & MCQ_READS_NOT_STRICT) != 0;
            }
            if (on_host) {                                       // the host parser: -reader host, or a chunk not in the strict form
                S.h_bases.resize(L1 + L2 + 1); S.h_seq_off.resize(2 * qcap + 1);
                if (mcq_reads_parse(S.text[0], L1, paired ? S.text[1] : nullptr, L2, flags, qcap, p.batch_bases, S.h_bases.data(),
                                    S.h_seq_off.data(), S.hdr, S.info)) { std::fprintf(stderr, "FAIL: %s\n", mcq_host_last_error()); return 1; }
                const uint64_t n = S.info[MCQ_READS_N];
                if (n && (hipMemcpyAsync(S.d_bases, S.h_bases.data(), S.info[MCQ_READS_BASES] + 1, hipMemcpyHostToDevice, s_in) != hipSuccess ||
                          hipMemcpyAsync(S.d_seq_off, S.h_seq_off.data(), (n * mates + 1) * 8, hipMemcpyHostToDevice, s_in) != hipSuccess ||
                          hipStreamSynchronize(s_in) != hipSuccess)) { std::fprintf(stderr, "FAIL: copying a batch to the GPU\n"); return 1; }
            }
            S.n = S.info[MCQ_READS_N]; S.host_parsed = on_host;
            if (S.n) {
                for (int m = 0; m < mates; ++m) {
                    const uint64_t cut = S.info[MCQ_READS_CUT1 + m];
                    if (mcq_read_stream_consume(rs[m], cut)) { std::fprintf(stderr, "FAIL: %s\n", mcq_host_last_error()); return 1; }
                    carry[m] = S.len[m] - cut; want[m] = p.read_chunk;
                }
                break;
            }
            for (int m = 0; m < mates; ++m) {                    // nothing to take: the end of a file, or a record larger than its chunk
                if (mcq_read_stream_consume(rs[m], 0)) { std::fprintf(stderr, "FAIL: %s\n", mcq_host_last_error()); return 1; }
                carry[m] = S.len[m];
                if (S.info[MCQ_READS_COMPLETE1 + m] == 0) {
                    if (eof[m]) at_end = true;
                    else want[m] = std::max<uint64_t>(1, 2 * S.len[m]);
                }
            }
            if (at_end) break;
        }
        if (at_end) break;
        if (!(ok = ensure_ws(S.n))) break;
        const uint64_t n = S.n;
        if (!grow_dev(S.d_cands, S.d_cands_cap, n * p.maxcand) || !grow_dev(S.d_ncand, S.d_ncand_cap, n) ||
            !grow_host(S.cands, S.cands_cap, n * p.maxcand) || !grow_host(S.ncand, S.ncand_cap, n)) return 1;
        mcq_batch in; std::memset(&in, 0, sizeof(in));
        in.n_seqs = n * mates; in.bases = S.d_bases; in.seq_off = S.d_seq_off; in.paired = paired ? 1 : 0; in.flags = MCQ_DEVICE_PTRS;
        mcq_result res; res.cands = S.d_cands; res.n_cand = S.d_ncand; res.flags = MCQ_DEVICE_PTRS;
        if (hipEventRecord(ev_in, s_in) != hipSuccess || hipStreamWaitEvent(s_k, ev_in, 0) != hipSuccess) return 1;
        if (mcq_query(edb, ws, &in, &qo, &res, s_k)) { std::fprintf(stderr, "FAIL: %s\n", mcq_last_error()); return 1; }
        if (hipMemcpyAsync(S.cands, S.d_cands, n * p.maxcand * sizeof(mcq_cand), hipMemcpyDeviceToHost, s_k) != hipSuccess ||
            hipMemcpyAsync(S.ncand, S.d_ncand, n * 4, hipMemcpyDeviceToHost, s_k) != hipSuccess) return 1;
        if (!S.host_parsed && hipMemcpyAsync(S.hdr, S.d_hdr, 2 * n * 8, hipMemcpyDeviceToHost, s_k) != hipSuccess) return 1;
        if (hipEventRecord(S.done, s_k) != hipSuccess) return 1;
        ++issued;
    }
    if (!ok || !drain()) return 1;
    if (tx) {
        std::vector<uint64_t> c(tax_counts.size(), 0);
        if (ws && mcq_ws_taxon_counts(ws, c.data(), 0)) { std::fprintf(stderr, "ABORT: %s\n", mcq_last_error()); return 1; }
        for (size_t i = 0; i < c.size(); ++i) tax_counts[i] += c[i];
        if (!write_abundances(os, rdb, p, tax_counts, assigned)) return 1;
    }
    write_summary(os, o, p, assigned, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count());
    for (int m = 0; m < mates; ++m) mcq_read_stream_close(rs[m]);
    for (Set& S : set) S.release();
    (void)hipEventDestroy(ev_in); (void)hipStreamDestroy(s_in); (void)hipStreamDestroy(s_k);
    mcq_ws_destroy(ws); mcq_taxonomy_destroy(tx); mcq_db_destroy(edb); mcq_refdb_close(rdb);
    return 0;
}
