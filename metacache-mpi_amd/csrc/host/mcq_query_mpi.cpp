// mcq_query_mpi -- `mpiexec -n N mcq_query_mpi <db> P r1.fq r2.fq ...`: the multi-GPU form of the reference's
// `mpiexec -n P metacache query` (src/main.cpp:41-104, src/mode_query.cpp:404-458), host code in C++ around the C ABI.
//
// One process per GPU (rank r uses device r mod device count).  Where the reference gives every rank the targets
// tgt % P and lets every rank sketch every read (src/sketch_database.h:540-542, src/querying.h:792-825), here every
// rank holds the hash range of the feature table it owns (mcq_db_desc.n_shards = N, .shard_id = rank: the union of the
// reference's P shard files, filtered by mcq_owner) and queries ITS slice of the reads through mcq_shard_query:
// features travel to their owners and location lists back -- ncclSend / ncclRecv groups over RCCL, the communicator's
// id made on rank 0 and carried by MPI_Bcast -- instead of the reference's tree of blocking MPI_Send / MPI_Recv of
// (query, taxon, hits) triplets (src/querying.h:867-1073).  emulate_ranks = P reproduces that tree's fold order, so the
// output is the reference's for `mpiexec -n P`, whatever N is.  Rank 0 gathers the mapping lines (MPI_Gatherv) and the
// statistics (MPI_Reduce) and writes the -out file (mcq_cli_common.hpp).
//
// -transport mpi moves the blocks through the host and MPI_Alltoallv instead (mcq_shard_set_exchange): for boxes where
// several ranks share one GPU, which RCCL refuses -- and the way this program is tested on a one-GPU box.
//
// The reads go through in batches (-batch queries, -batch-bases bases per rank and batch; the context and the communicator
// are set up for that shape before the clock starts): batch j+1 is staged and announced while batch j is enqueued and
// batch j-1 may still run, results come back behind the kernels and are written out while the next batches run.
//
// The inputs are mcq_query_cli's (mcq_cli_common.hpp): the units go through one after the other, every rank reading each
// unit's files whole; an interleaved file (-pairseq) is paired by the host parser (mcq_reads_parse, MCQ_READS_INTERLEAVED).
//
// usage: mpiexec -n N mcq_query_mpi <dbprefix> <P> <file|directory>... [options of mcq_query_cli] [-transport rccl|mpi]
//                                   [-batch N] [-batch-bases N]
// -align (and its aliases) is rejected the same way.
// -exclude, -ground-truth and -precision are rejected with a line that names mcq_query_cli: the sharded kernels have no exclusion.
// -hits-per-seq is rejected the same way: mcq_target_hits is a kernel of the one-GPU path.  So is -allhits (mcq_all_hits), and so
// are -coverage and -cov-percentile (mcq_coverage_* work on mcq_target_hits' outputs).
// -queryids and -locations come through the shared parser and writer.
#include <mpi.h>
#include <hip/hip_runtime_api.h>

#include <sstream>

#include "mcq_cli_buffers.hpp"
#include "mcq_cli_common.hpp"

#define HIP_OR_DIE(expr) MCQ_HIP_AS("ABORT", expr, MPI_Abort(MPI_COMM_WORLD, 1))
#define MCQ_OR_DIE(expr) do { if ((expr) != MCQ_OK) { \
    std::fprintf(stderr, "ABORT: %s: %s\n", #expr, mcq_last_error()); MPI_Abort(MPI_COMM_WORLD, 1); } } while (0)

struct Rec { std::string header, seq; };

// FASTA ('>') and FASTQ ('@') records; sequence may span lines in FASTA (src/sequence_io.cpp:122-285)
static bool read_records(const std::string& path, std::vector<Rec>& out) {
    std::ifstream is(path);
    if (!is.good()) return false;
    std::string line;
    while (std::getline(is, line)) {
        if (line.empty()) continue;
        if (line[0] == '@') {
            Rec r; r.header = line.substr(1);
            std::getline(is, r.seq);
            std::getline(is, line); std::getline(is, line);          // '+' and qualities
            out.push_back(std::move(r));
        } else if (line[0] == '>') {
            Rec r; r.header = line.substr(1);
            out.push_back(std::move(r));
        } else if (!out.empty()) {
            out.back().seq += line;
        }
    }
    return true;
}

// an interleaved file: records 2q, 2q+1 -> r1[q], r2[q] (an unpaired last record gets an empty mate), through the host parser
static bool read_interleaved(const std::string& path, std::vector<Rec>& r1, std::vector<Rec>& r2) {
    std::ifstream is(path, std::ios::binary);
    if (!is.good()) return false;
    const std::string text((std::istreambuf_iterator<char>(is)), std::istreambuf_iterator<char>());
    const uint64_t cap = text.size() / 2 + 2;
    std::vector<char> bases(text.size() + 1); std::vector<uint64_t> off(2 * cap + 1), hdr(2 * cap), info(MCQ_READS_INFO_WORDS);
    if (mcq_reads_parse(text.data(), text.size(), nullptr, 0, MCQ_READS_EOF1 | MCQ_READS_INTERLEAVED, cap, ~0ull, bases.data(), off.data(),
                        hdr.data(), info.data())) { std::fprintf(stderr, "ABORT: %s\n", mcq_host_last_error()); return false; }
    for (uint64_t q = 0; q < info[MCQ_READS_N]; ++q) {
        Rec a, b;
        a.header.assign(text, hdr[2 * q], hdr[2 * q + 1] - hdr[2 * q]);
        a.seq.assign(bases.data() + off[2 * q], off[2 * q + 1] - off[2 * q]);
        b.seq.assign(bases.data() + off[2 * q + 1], off[2 * q + 2] - off[2 * q + 1]);
        r1.push_back(std::move(a)); r2.push_back(std::move(b));
    }
    return true;
}

// one of the three sets of device inputs / outputs
struct DevSet {
    DeviceBuf<char> bases; DeviceBuf<uint64_t> off; DeviceBuf<mcq_cand> d_cands; DeviceBuf<uint32_t> d_ncand;
    PinnedBuf<mcq_cand> cands; PinnedBuf<uint32_t> ncand; Event out;
};

// mcq_exchange_fn over MPI: device blocks -> host, MPI_Alltoallv, host -> device
static int exchange_over_mpi(void*, const void* send_base, const uint64_t* send_off, const uint64_t* send_bytes,
                             void* recv_base, const uint64_t* recv_off, const uint64_t* recv_bytes, uint32_t n, uint32_t) {
    std::vector<int> sc(n), sd(n), rc(n), rd(n);
    uint64_t st = 0, rt = 0;
    for (uint32_t p = 0; p < n; ++p) {
        if (send_bytes[p] > 0x7FFFFFFFull || recv_bytes[p] > 0x7FFFFFFFull || st > 0x7FFFFFFFull || rt > 0x7FFFFFFFull) return 1;   // int counts of MPI
        sc[p] = (int)send_bytes[p]; sd[p] = (int)st; st += send_bytes[p];
        rc[p] = (int)recv_bytes[p]; rd[p] = (int)rt; rt += recv_bytes[p];
    }
    std::vector<char> hs(st ? st : 1), hr(rt ? rt : 1);
    for (uint32_t p = 0; p < n; ++p)
        if (sc[p] && hipMemcpy(hs.data() + sd[p], (const char*)send_base + send_off[p], send_bytes[p], hipMemcpyDeviceToHost) != hipSuccess) return 1;
    if (MPI_Alltoallv(hs.data(), sc.data(), sd.data(), MPI_BYTE, hr.data(), rc.data(), rd.data(), MPI_BYTE, MPI_COMM_WORLD) != MPI_SUCCESS) return 1;
    for (uint32_t p = 0; p < n; ++p)
        if (rc[p] && hipMemcpy((char*)recv_base + recv_off[p], hr.data() + rd[p], recv_bytes[p], hipMemcpyHostToDevice) != hipSuccess) return 1;
    return 0;
}

int main(int argc, char** argv) {
    MPI_Init(&argc, &argv);
    int rank = 0, N = 1;
    MPI_Comm_rank(MPI_COMM_WORLD, &rank);
    MPI_Comm_size(MPI_COMM_WORLD, &N);
    Options p;                                                              // the command line; `run` below: one output's part of it
    if (!parse_options(argc, argv, p)) { MPI_Finalize(); return 2; }
    if (p.list_inputs) { if (rank == 0) list_inputs(std::cout, p); MPI_Finalize(); return 0; }
    if (p.wants_truth()) {                                                  // (before any GPU work)
        if (rank == 0) std::fprintf(stderr, "ABORT: -exclude, -ground-truth and -precision are options of mcq_query_cli; mcq_query_mpi does not evaluate against a ground truth\n");
        MPI_Finalize(); return 2;
    }
    if (p.hits_per_seq) {                                                   // (before any GPU work)
        if (rank == 0) std::fprintf(stderr, "ABORT: -hits-per-seq is an option of mcq_query_cli; mcq_query_mpi keeps no window hit lists (the sharded path has none)\n");
        MPI_Finalize(); return 2;
    }
    if (p.align || p.align_range) {                                         // (before any GPU work)
        if (rank == 0) std::fprintf(stderr, "ABORT: -align is an option of mcq_query_cli; mcq_query_mpi aligns no reads (its ranks hold neither the candidates' positions nor the genomes)\n");
        MPI_Finalize(); return 2;
    }
    if (p.allhits) {                                                        // (before any GPU work)
        if (rank == 0) std::fprintf(stderr, "ABORT: -allhits is an option of mcq_query_cli; mcq_query_mpi lists no hits (mcq_all_hits is a kernel of the one-GPU path)\n");
        MPI_Finalize(); return 2;
    }
    if (p.cov_on()) {                                                       // (before any GPU work)
        if (rank == 0) std::fprintf(stderr, "ABORT: -coverage and -cov-percentile are options of mcq_query_cli; mcq_query_mpi keeps no window coverage (mcq_target_hits is a kernel of the one-GPU path)\n");
        MPI_Finalize(); return 2;
    }
    int n_dev = 0;
    HIP_OR_DIE(hipGetDeviceCount(&n_dev));
    if (n_dev < 1) { std::fprintf(stderr, "ABORT: no GPU\n"); MPI_Abort(MPI_COMM_WORLD, 1); }
    const int device = rank % n_dev;
    HIP_OR_DIE(hipSetDevice(device));

    // this rank's hash range of the table
    Database db;
    if (!open_database(p, db, (uint32_t)N, (uint32_t)rank, device)) MPI_Abort(MPI_COMM_WORLD, 1);

    // the context for a fixed batch shape and the communicator: set up before the clock starts, like the reference's
    // database load and MPI_Init (identical capacities on every rank)
    const uint64_t B = p.batch, MB = p.batch_bases;
    mcq_shard_cfg cfg; std::memset(&cfg, 0, sizeof(cfg));
    cfg.n_ranks = (uint32_t)N; cfg.rank = (uint32_t)rank;
    cfg.max_queries = B; cfg.max_seqs = 2 * B; cfg.max_bases = MB;
    mcq_shard* ctx = nullptr;
    MCQ_OR_DIE(mcq_shard_create(db.edb, &cfg, &ctx));
    if (p.transport == "mpi") MCQ_OR_DIE(mcq_shard_set_exchange(ctx, exchange_over_mpi, nullptr));
    else if (N > 1 || std::getenv("MCQ_SHARD_FORCE_RCCL")) {
        char id[MCQ_SHARD_UNIQUE_ID_BYTES];
        if (rank == 0) MCQ_OR_DIE(mcq_shard_unique_id(id));                // ncclGetUniqueId
        MPI_Bcast(id, sizeof id, MPI_BYTE, 0, MPI_COMM_WORLD);
        MCQ_OR_DIE(mcq_shard_comm_rccl(ctx, id));                          // ncclCommInitRank
    }
    // three sets of device inputs / outputs: batch j+1 is staged while batch j-1 may still run (its set is the one batch
    // j+2 will take), results come back on the stream behind the kernels
    constexpr int NS = 3;
    Stream st; DevSet set[NS];
    bool made = st.create();
    for (DevSet& S : set)
        made = made && S.bases.grow(MB + 64) && S.off.grow(2 * B + 1) && S.d_cands.grow(B * p.maxcand) && S.d_ncand.grow(B) &&
               S.cands.grow(B * p.maxcand) && S.ncand.grow(B) && S.out.create();

    // -abundances / -abundance-per: every batch's device results are classified on the GPU into per-taxon counts (reduced to rank 0)
    mcq_taxonomy* tx = nullptr; DeviceBuf<uint64_t> d_counts; uint32_t n_taxa = 0;
    const mcq_classify_opts co = classify_opts(p, db.hitmin);
    if (p.tax_counts()) {
        mcq_refdb_info info; mcq_refdb_get_info(db.rdb, &info); n_taxa = info.n_taxa;
        if (!(tx = make_taxonomy(db.rdb, device))) MPI_Abort(MPI_COMM_WORLD, 1);
        made = made && d_counts.grow((size_t)n_taxa + 1);
    }
    if (!made) MPI_Abort(MPI_COMM_WORLD, 1);

    if (p.split && !inputs_readable(p)) MPI_Abort(MPI_COMM_WORLD, 1);
    for (const Options& run : output_runs(p)) {                             // one output, or (-splitout) one per unit
        MPI_Barrier(MPI_COMM_WORLD);                                            // src/mode_query.cpp:129
        const auto t_start = std::chrono::steady_clock::now();
        const mcq_query_opts qo = query_opts(run);
        const Out o = make_out(db.rdb, run);
        const bool paired = run.paired();
        std::string all;                                                        // rank 0: unit lines and mapping lines, in input order
        uint64_t assigned[MCQ_RANK_NONE + 1] = {0};                             // this rank's queries, over all units
        std::vector<uint64_t> counts((size_t)n_taxa + 1, 0), counts_u((size_t)n_taxa + 1), counts_all((size_t)n_taxa + 1);
        uint64_t id_base = 1;                                                   // -queryids: the 1-based number of a unit's first query over all units of this output
        for (const ReadUnit& U : run.units) {
            // every rank reads the unit's files and keeps its contiguous slice of the queries
            std::vector<Rec> r1, r2;
            if (!(U.interleaved ? read_interleaved(U.f1, r1, r2) : read_records(U.f1, r1))) { std::fprintf(stderr, "FAIL: can't open file %s\n", U.f1.c_str()); MPI_Abort(MPI_COMM_WORLD, 1); }
            if (U.files() == 2 && !read_records(U.f2, r2)) { std::fprintf(stderr, "FAIL: can't open file %s\n", U.f2.c_str()); MPI_Abort(MPI_COMM_WORLD, 1); }
            const size_t nq_all = paired ? std::min(r1.size(), r2.size()) : r1.size();
            const size_t q0 = nq_all * (size_t)rank / (size_t)N, q1 = nq_all * (size_t)(rank + 1) / (size_t)N;
            // the slice in batches of at most B queries and MB bases; every rank makes the same number of (collective) calls
            std::vector<size_t> cut{q0};
            {
                size_t nb_q = 0; uint64_t nb_b = 0;
                for (size_t q = q0; q < q1; ++q) {
                    const uint64_t len = r1[q].seq.size() + (paired ? r2[q].seq.size() : 0);
                    if (len > MB) { std::fprintf(stderr, "ABORT: query %zu is longer than -batch-bases\n", q); MPI_Abort(MPI_COMM_WORLD, 1); }
                    if (nb_q == B || nb_b + len > MB) { cut.push_back(q); nb_q = 0; nb_b = 0; }
                    ++nb_q; nb_b += len;
                }
                cut.push_back(q1);
            }
            unsigned long long nb_mine = cut.size() - 1, nb = 0;
            MPI_Allreduce(&nb_mine, &nb, 1, MPI_UNSIGNED_LONG_LONG, MPI_MAX, MPI_COMM_WORLD);
            auto lo = [&](size_t j) { return j < cut.size() - 1 ? cut[j] : q1; };
            auto hi = [&](size_t j) { return j < cut.size() - 1 ? cut[j + 1] : q1; };

            std::ostringstream lines;
            uint64_t assigned_u[MCQ_RANK_NONE + 1] = {0};
            std::vector<mcq_batch> in(nb ? nb : 1);
            std::string bases; std::vector<uint64_t> off;
            auto stage = [&](size_t j) {                                           // batch j of this rank to its device set
                DevSet& S = set[j % NS];
                bases.clear(); off.assign(1, 0);
                for (size_t q = lo(j); q < hi(j); ++q) {
                    bases += r1[q].seq; off.push_back(bases.size());
                    if (paired) { bases += r2[q].seq; off.push_back(bases.size()); }
                }
                if (!bases.empty()) HIP_OR_DIE(hipMemcpy(S.bases.p, bases.data(), bases.size(), hipMemcpyHostToDevice));
                HIP_OR_DIE(hipMemcpy(S.off.p, off.data(), off.size() * 8, hipMemcpyHostToDevice));
                std::memset(&in[j], 0, sizeof(mcq_batch));
                in[j].n_seqs = off.size() - 1; in[j].bases = S.bases.p; in[j].seq_off = S.off.p; in[j].paired = paired ? 1 : 0; in[j].flags = MCQ_DEVICE_PTRS;
            };
            auto finish = [&](size_t j) {                                          // results of batch j: wait, write its mapping lines
                const DevSet& S = set[j % NS];
                HIP_OR_DIE(hipEventSynchronize(S.out));
                for (size_t q = lo(j); q < hi(j); ++q)
                    write_query(lines, o, db.hitmin, r1[q].header, &S.cands.p[(q - lo(j)) * p.maxcand], S.ncand.p[q - lo(j)], assigned_u, id_base + q);
            };
            // the first batch of a context exchanges exact sizes and learns the block sizes the others travel at; should a later
            // batch not fit them (MCQ_E_CAPACITY at the end), everything is repeated with exact sizes
            for (int attempt = 0; attempt < 2; ++attempt) {
                const uint32_t flags = attempt ? MCQ_SHARD_EXACT : 0;
                lines.str(""); std::memset(assigned_u, 0, sizeof(assigned_u));
                if (tx) HIP_OR_DIE(hipMemsetAsync(d_counts.p, 0, ((size_t)n_taxa + 1) * 8, st));
                if (nb) stage(0);
                for (size_t j = 0; j < nb; ++j) {
                    DevSet& S = set[j % NS];
                    if (j >= 2) finish(j - 2);                                      // (its device set is the one batch j+1 takes)
                    if (j + 1 < nb) stage(j + 1);
                    mcq_result res; res.cands = S.d_cands.p; res.n_cand = S.d_ncand.p; res.flags = MCQ_DEVICE_PTRS;
                    MCQ_OR_DIE(mcq_shard_query(ctx, &in[j], &qo, &res, st, flags, j + 1 < nb ? &in[j + 1] : nullptr));
                    const size_t nqj = hi(j) - lo(j);
                    if (tx && nqj) MCQ_OR_DIE(mcq_classify(tx, &res, nqj, p.maxcand, &co, nullptr, d_counts.p, st));
                    if (nqj) {
                        HIP_OR_DIE(hipMemcpyAsync(S.cands.p, S.d_cands.p, nqj * p.maxcand * sizeof(mcq_cand), hipMemcpyDeviceToHost, st));
                        HIP_OR_DIE(hipMemcpyAsync(S.ncand.p, S.d_ncand.p, nqj * 4, hipMemcpyDeviceToHost, st));
                    }
                    HIP_OR_DIE(hipEventRecord(S.out, st));
                }
                if (nb >= 2) finish(nb - 2);
                if (nb >= 1) finish(nb - 1);
                const int rc = mcq_shard_sync(ctx, st, nullptr);
                int bad = rc == MCQ_E_CAPACITY ? 1 : 0, any = 0;
                if (rc != MCQ_OK && rc != MCQ_E_CAPACITY) { std::fprintf(stderr, "ABORT: %s\n", mcq_last_error()); MPI_Abort(MPI_COMM_WORLD, 1); }
                MPI_Allreduce(&bad, &any, 1, MPI_INT, MPI_MAX, MPI_COMM_WORLD);
                if (!any) break;
                if (attempt) { std::fprintf(stderr, "ABORT: %s\n", mcq_last_error()); MPI_Abort(MPI_COMM_WORLD, 1); }
            }

            for (int i = 0; i <= (int)MCQ_RANK_NONE; ++i) assigned[i] += assigned_u[i];
            if (tx) {                                                               // (d_counts holds this unit's: an attempt starts it at zero)
                HIP_OR_DIE(hipStreamSynchronize(st));
                HIP_OR_DIE(hipMemcpy(counts_u.data(), d_counts.p, counts_u.size() * 8, hipMemcpyDeviceToHost));
                for (size_t i = 0; i < counts.size(); ++i) counts[i] += counts_u[i];
            }
            // rank 0 collects the unit's mapping lines behind its "# f1 + f2" line
            const std::string mine_s = lines.str();
            if (mine_s.size() > 0x7FFFFFFFull) { std::fprintf(stderr, "ABORT: more than 2 GB of mapping lines on one rank\n"); MPI_Abort(MPI_COMM_WORLD, 1); }
            int len = (int)mine_s.size();
            std::vector<int> lens(N), disp(N);
            MPI_Gather(&len, 1, MPI_INT, lens.data(), 1, MPI_INT, 0, MPI_COMM_WORLD);
            std::string unit_lines;
            if (rank == 0) { int t = 0; for (int r = 0; r < N; ++r) { disp[r] = t; t += lens[r]; } unit_lines.resize((size_t)t); }
            MPI_Gatherv(mine_s.data(), len, MPI_CHAR, rank == 0 ? &unit_lines[0] : nullptr, lens.data(), disp.data(), MPI_CHAR, 0, MPI_COMM_WORLD);
            if (rank == 0) { std::ostringstream ul; write_unit_line(ul, o, U); all += ul.str(); all += unit_lines; }
            id_base += nq_all;
        }
        // ... and the statistics, and writes
        unsigned long long a_loc[MCQ_RANK_NONE + 1], a_all[MCQ_RANK_NONE + 1];
        for (int i = 0; i <= (int)MCQ_RANK_NONE; ++i) a_loc[i] = assigned[i];
        MPI_Reduce(a_loc, a_all, MCQ_RANK_NONE + 1, MPI_UNSIGNED_LONG_LONG, MPI_SUM, 0, MPI_COMM_WORLD);
        if (tx) {
            static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "u64 counts travel as MPI_UNSIGNED_LONG_LONG");
            MPI_Reduce(counts.data(), counts_all.data(), (int)counts.size(), MPI_UNSIGNED_LONG_LONG, MPI_SUM, 0, MPI_COMM_WORLD);
        }
        if (rank == 0) {
            std::ofstream fout;
            std::ostream& os = open_out(run, fout);
            write_head(os, o, db.hitmin);
            os << all;
            for (int i = 0; i <= (int)MCQ_RANK_NONE; ++i) assigned[i] = a_all[i];
            if (tx && !write_abundances(os, db.rdb, run, counts_all, assigned)) MPI_Abort(MPI_COMM_WORLD, 1);
            write_summary(os, o, assigned, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count());
        }
    }
    mcq_taxonomy_destroy(tx);
    mcq_shard_destroy(ctx);
    MPI_Finalize();
    return 0;                                                               // (the owners give back the rest)
}
