// mcq_build_cli -- stand-in for `mpiexec -n P metacache_mpi build DB GENOMES... -taxonomy DIR` (src/mode_build.cpp:1145-1172,
// add_to_database :797-1108) on one GPU: writes DB.db_0 .. DB.db_<P-1>, the files the P ranks of that run write.
//
//   1. the inputs (include/mcq_host.h): the taxonomy dump (mcq_taxdump_read), the genome files in the reference's order
//      (mcq_genome_files), their sequences streamed through two pinned buffers into device memory (mcq_genome_reader_*): target
//      ids, names and parents as the reference gives them
//   2. the union of the P rank tables on the GPU (mcq_build_table: sketch, per-(feature, rank) limit, rank merge,
//      -remove-overpopulated-features), then -remove-ambig-features on that union (mcq_table_remove_ambiguous with the targets'
//      clade keys from mcq_taxa_clade_keys); the unfiltered table is released before the rank split
//   3. per rank: its table cut out of the union on the GPU (mcq_table_rank_split), copied to the host and written by
//      mcq_refdb_write_shard with the whole taxon list (`windows` set for the targets the rank owns, src/sketch_database.h:540-542)
// Host memory: two read buffers (-read-buffer) and the tables of -ranks-per-pass ranks; never the union table.
//
// usage: mcq_build_cli DB P GENOMES... -taxonomy DIR [-kmerlen K] [-sketchlen S] [-winlen W] [-winstride X]
//            [-max-locations-per-feature N] [-remove-overpopulated-features] [-remove-ambig-features RANK] [-max-ambig-per-feature N]
//            [-device D] [-ranks-per-pass R] [-read-buffer BYTES]
// -remove-ambig-features RANK [-max-ambig-per-feature N, default 1]: a feature whose locations, over all P ranks and after the limit
// and -remove-overpopulated-features, name more than N distinct taxa at RANK (targets without one count as one taxon; the targets
// themselves for `sequence`) is left out of every file: remove_ambiguous_features (src/sketch_database.h:428-470) as the
// non-distributed post_process_features calls it (src/mode_build.cpp:729-747), on the whole database.  N is narrowed to 8 bits, then
// 0 becomes 1; RANK `none` or unknown leaves the option off (a warning); nothing happens when the dump holds at most one taxon.
// DIVERGENCE: the reference's `mpiexec -n P metacache_mpi build` accepts the options and ignores them (the call is commented out in
// post_process_features_distributed, src/mode_build.cpp:770-789, at every P): there is no reference file to compare with.
// Not reproduced: the order of the keys inside a file (the reference's hash table order; its reader inserts key by key, any order
// reads back the same), and the mapping of sequences to taxa through assembly_summary.txt / *.accession2taxid files: a target's
// parent is the N of "taxid|N" in its header, or 0.  The sequences and the temporaries of the one-piece build must fit the
// GPU (about 60 B per feature slot: tens of Gbp on one MI355X); MCQ_BUILD_TRACE=1 prints the times of the phases.
#include "mcq_cli_common.hpp"
#include "mcq_cli_buffers.hpp"

#include <sys/stat.h>
#include <thread>

namespace {

struct BuildOptions {
    std::string db, taxonomy; uint32_t P = 1; std::vector<std::string> inputs;
    int kmerlen = 16, sketchlen = 16, winlen = 128, winstride = -1, max_locs = 254;      // src/mode_build.cpp:63-72, :108-119
    bool remove_overpopulated = false;
    uint32_t ambig_rank = MCQ_RANK_NONE; int max_ambig = 1;                             // src/mode_build.cpp:74-75, :124-131
    int device = 0; uint32_t ranks_per_pass = 1; uint64_t read_buffer = 64u << 20;
};

const char* kUsage =
    "usage: mcq_build_cli DB P GENOMES... -taxonomy DIR [-kmerlen K] [-sketchlen S] [-winlen W] [-winstride X]\n"
    "           [-max-locations-per-feature N] [-remove-overpopulated-features] [-remove-ambig-features RANK] [-max-ambig-per-feature N]\n"
    "           [-device D] [-ranks-per-pass R] [-read-buffer BYTES]\n"
    "writes DB.db_0 .. DB.db_<P-1>: the files `mpiexec -n P metacache_mpi build DB GENOMES... -taxonomy DIR` writes\n"
    "  GENOMES        FASTA files or directories of them (before the first option); directories are read recursively\n"
    "  -taxonomy DIR  nodes.dmp, names.dmp and, if present, merged.dmp\n"
    "  defaults       -kmerlen 16 -sketchlen 16 -winlen 128 -winstride winlen-kmerlen+1 -max-locations-per-feature 254\n"
    "  limits         kmerlen <= 16, sketchlen <= 32, winlen <= 128 (the kernels' limits)\n"
    "  -remove-ambig-features RANK [-max-ambig-per-feature N]   leaves out every feature whose locations, over all P ranks, name more\n"
    "                 than N (default 1; narrowed to 8 bits, 0 -> 1) distinct taxa at RANK (sequence .. root; targets without a taxon there\n"
    "                 count as one); `none` or an unknown RANK leaves it off.  Divergence: the reference's `mpiexec -n P metacache_mpi\n"
    "                 build` accepts the options and ignores them; here they do what the reference documents\n"
    "  -ranks-per-pass R   ranks whose tables are in host memory at a time (default 1); -read-buffer: bytes of each of the two read buffers\n"
    "not supported: assembly_summary.txt / *.accession2taxid mapping files (a target's parent is the N of 'taxid|N' in its\n"
    "header, else none), FASTQ genome files, adding to an existing database; the key order inside a file is not the reference's\n";

bool parse(int argc, char** argv, BuildOptions& o) {
    for (int i = 1; i < argc; ++i) if (opt_named(argv[i], {"-help", "--help", "-h"})) { std::fputs(kUsage, stdout); return false; }
    if (argc < 4) { std::fputs(kUsage, stderr); return false; }
    o.db = argv[1];
    if (o.db.find(".db") == std::string::npos) o.db += ".db";                // database_name, src/args_handling.cpp:33-45
    o.P = (uint32_t)std::atoi(argv[2]);
    int i = 3;
    for (; i < argc && argv[i][0] != '-'; ++i) o.inputs.push_back(argv[i]);   // files come before the options (src/args_handling.cpp:56-75)
    for (; i < argc; ++i) {
        const std::string a = argv[i];
        auto next = [&]() -> const char* { return (i + 1 < argc) ? argv[++i] : ""; };
        if (opt_named(a, {"-taxonomy"})) o.taxonomy = next();
        else if (opt_named(a, {"-kmerlen"})) o.kmerlen = std::atoi(next());
        else if (opt_named(a, {"-sketchlen"})) o.sketchlen = std::atoi(next());
        else if (opt_named(a, {"-winlen"})) o.winlen = std::atoi(next());
        else if (opt_named(a, {"-winstride"})) o.winstride = std::atoi(next());
        else if (opt_named(a, {"-max-locations-per-feature", "-max_locations_per_feature"})) o.max_locs = std::atoi(next());
        else if (opt_named(a, {"-remove-overpopulated-features", "-remove_overpopulated_features"})) o.remove_overpopulated = true;
        else if (opt_named(a, {"-remove-ambig-features", "-remove_ambig_features"})) {
            const std::string name = next();
            o.ambig_rank = mcq_rank_from_name(name.c_str());                // (`none` and unknown names: off, src/taxonomy.h:173-213)
            if (o.ambig_rank >= MCQ_RANK_NONE) std::fprintf(stderr, "warning: -remove-ambig-features %s names no rank: no feature is removed\n", name.c_str());
        }
        else if (opt_named(a, {"-max-ambig-per-feature", "-max_ambig_per_feature"})) o.max_ambig = std::atoi(next());
        else if (opt_named(a, {"-device"})) o.device = std::atoi(next());
        else if (opt_named(a, {"-ranks-per-pass"})) o.ranks_per_pass = (uint32_t)std::max(1, std::atoi(next()));
        else if (opt_named(a, {"-read-buffer"})) o.read_buffer = std::max<uint64_t>(1, std::strtoull(next(), nullptr, 10));
        else { std::fprintf(stderr, "ABORT: unknown option %s\n%s", a.c_str(), kUsage); return false; }
    }
    if (o.P < 1 || o.P > 64) { std::fprintf(stderr, "ABORT: P must be 1..64\n"); return false; }
    if (o.inputs.empty()) { std::fprintf(stderr, "ABORT: Nothing to do - no reference sequences provided.\n"); return false; }
    if (o.taxonomy.empty()) { std::fprintf(stderr, "ABORT: -taxonomy DIR is required\n"); return false; }
    if (o.winstride < 0) o.winstride = o.winlen - o.kmerlen + 1;             // src/mode_build.cpp:111
    if (o.winstride < 1) o.winstride = 1;                                    // src/sketch_database.h:321-324
    // -max-locations-per-feature N as the reference takes it: applied only if N > 0 (src/mode_build.cpp:658-660), then narrowed to
    // the bucket size type, 8 bits (src/config.h:77: 256 -> 0, 300 -> 44), then brought into 1..254 (src/sketch_database.h:356-368)
    if (o.max_locs <= 0) o.max_locs = 254;
    else { o.max_locs &= 0xFF; o.max_locs = std::min(std::max(o.max_locs, 1), 254); }
    // -max-ambig-per-feature N: the parameter is a bucket_size_type, 8 bits (256 -> 0, 300 -> 44); then 0 -> 1 (src/sketch_database.h:437)
    o.max_ambig &= 0xFF;
    if (o.max_ambig == 0) o.max_ambig = 1;
    return true;
}

struct Phases {                          // wall time per phase; MCQ_BUILD_TRACE=1 prints them as they end
    const bool on = std::getenv("MCQ_BUILD_TRACE") != nullptr;
    std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
    void operator()(const char* name) {
        const auto now = std::chrono::steady_clock::now();
        if (on) std::fprintf(stderr, "[mcq_build_cli] %-28s %8.3f s\n", name, std::chrono::duration<double>(now - last).count());
        last = now;
    }
};

// owners of the library handles: every `return` of main gives them back
struct TaxDump { mcq_taxdump* h = nullptr; ~TaxDump() { mcq_taxdump_free(h); } };
struct FileList { mcq_file_list* h = nullptr; ~FileList() { mcq_file_list_free(h); } };
struct GenomeReader { mcq_genome_reader* h = nullptr; ~GenomeReader() { mcq_genome_reader_close(h); } };
struct Table { mcq_table* h = nullptr; ~Table() { mcq_table_free(h); } void reset() { mcq_table_free(h); h = nullptr; } };

// one rank's table and taxon list in host memory
struct RankOut {
    PinnedBuf<uint32_t> keys; PinnedBuf<uint64_t> off, locs; uint64_t n_keys = 0, n_locs = 0;
    std::vector<mcq_taxon_rec> taxa; std::string path; int rc = 0; std::string err;
};

int host_fail() { std::fprintf(stderr, "ABORT: %s\n", mcq_host_last_error()); return 1; }

}  // namespace

int main(int argc, char** argv) {
    BuildOptions o;
    if (!parse(argc, argv, o)) return 2;
    Phases phase;
    MCQ_HIP(hipSetDevice(o.device), return 1);
    {   // the kernels' limits, before anything is read or written: a key-less handle carries the sketching parameters
        mcq_db_desc sd; std::memset(&sd, 0, sizeof(sd));
        sd.k = (uint32_t)o.kmerlen; sd.sketch_size = (uint32_t)o.sketchlen; sd.winlen = (uint32_t)o.winlen; sd.winstride = (uint32_t)o.winstride;
        const uint64_t zero = 0; sd.list_off = &zero; sd.n_shards = 1; sd.device = o.device;
        mcq_db* probe = nullptr;
        if (o.kmerlen < 0 || o.sketchlen < 0 || o.winlen < 0) { std::fprintf(stderr, "ABORT: negative parameter\n"); return 1; }
        if (mcq_db_create(&sd, &probe)) { std::fprintf(stderr, "ABORT: %s\n", mcq_last_error()); return 1; }
        mcq_db_destroy(probe);
    }
    TaxDump tax;
    if (mcq_taxdump_read(o.taxonomy.c_str(), &tax.h)) return host_fail();

    // ---- 1. the sequences: files -> two pinned buffers in turn -> device memory, back to back
    FileList files;
    {
        std::vector<const char*> args;
        for (const std::string& s : o.inputs) args.push_back(s.c_str());
        if (mcq_genome_files(args.data(), (uint32_t)args.size(), &files.h)) return host_fail();
    }
    std::vector<const char*> paths;
    uint64_t total_bytes = 0;
    for (uint32_t i = 0; i < mcq_file_list_count(files.h); ++i) {
        paths.push_back(mcq_file_list_get(files.h, i));
        struct stat st;
        if (::stat(paths.back(), &st) == 0 && S_ISREG(st.st_mode)) total_bytes += (uint64_t)st.st_size;     // (a file holds at least its bases)
    }
    GenomeReader reader;
    if (mcq_genome_reader_open(paths.data(), (uint32_t)paths.size(), std::min<uint64_t>(o.read_buffer, 16u << 20), &reader.h)) return host_fail();
    DeviceBuf<char> d_bases; PinnedBuf<char> stage[2]; Event copied[2]; Stream s_in;
    if (!d_bases.grow(total_bytes + 1) || !stage[0].grow(o.read_buffer) || !stage[1].grow(o.read_buffer) || !s_in.create() ||
        !copied[0].create() || !copied[1].create()) return 1;
    uint64_t n_bases = 0;
    for (int j = 0;; ++j) {
        PinnedBuf<char>& S = stage[j & 1];
        if (j >= 2) MCQ_HIP(hipEventSynchronize(copied[j & 1]), return 1);      // the copy that last read this buffer
        uint64_t n = 0; int32_t done = 0;
        if (mcq_genome_reader_next(reader.h, S.p, o.read_buffer, &n, &done)) return host_fail();
        if (n_bases + n > total_bytes + 1) { std::fprintf(stderr, "ABORT: the genome files grew while they were read\n"); return 1; }
        if (n) MCQ_HIP(hipMemcpyAsync(d_bases.p + n_bases, S.p, n, hipMemcpyHostToDevice, s_in), return 1);
        MCQ_HIP(hipEventRecord(copied[j & 1], s_in), return 1);
        n_bases += n;
        if (done) break;
    }
    MCQ_HIP(hipStreamSynchronize(s_in), return 1);
    const uint32_t nt = mcq_genome_reader_n_targets(reader.h);
    if (nt < 1) { std::fprintf(stderr, "ABORT: no reference sequence found in the genome files\n"); return 1; }
    std::vector<mcq_taxon_rec> targets(nt);
    std::vector<uint64_t> seq_off((size_t)nt + 1, 0);
    for (uint32_t t = 0; t < nt; ++t) {
        uint64_t len = 0;
        if (mcq_genome_reader_target(reader.h, t, &targets[t], &len)) return host_fail();
        seq_off[t + 1] = seq_off[t] + len;
    }
    DeviceBuf<uint64_t> d_seq_off;
    if (!d_seq_off.grow((uint64_t)nt + 1)) return 1;
    MCQ_HIP(hipMemcpy(d_seq_off.p, seq_off.data(), ((size_t)nt + 1) * 8, hipMemcpyHostToDevice), return 1);
    stage[0] = PinnedBuf<char>(); stage[1] = PinnedBuf<char>();              // (the read buffers are not needed any more)
    phase("read");

    // ---- 2. the union of the P rank tables
    Table table;
    {
        mcq_build_desc d; std::memset(&d, 0, sizeof(d));
        d.k = (uint32_t)o.kmerlen; d.sketch_size = (uint32_t)o.sketchlen; d.winlen = (uint32_t)o.winlen; d.winstride = (uint32_t)o.winstride;
        d.n_targets = nt; d.bases = d_bases.p; d.seq_off = d_seq_off.p; d.emulate_ranks = o.P; d.max_locs = (uint32_t)o.max_locs;
        d.flags = MCQ_DEVICE_PTRS | (o.remove_overpopulated ? MCQ_BUILD_REMOVE_OVERPOPULATED : 0); d.device = o.device;
        if (mcq_build_table(&d, &table.h)) { std::fprintf(stderr, "ABORT: %s\n", mcq_build_last_error()); return 1; }
    }
    d_bases = DeviceBuf<char>();
    std::vector<uint32_t> windows(nt);
    if (mcq_table_tgt_windows(table.h, windows.data())) { std::fprintf(stderr, "ABORT: %s\n", mcq_build_last_error()); return 1; }
    phase("sketch + sort");

    // The taxon list: sequence-level taxa (id -(target + 1): the last target first) before the taxonomy's, both in ascending id
    // (src/taxonomy.h:290-294, :348)
    std::vector<mcq_taxon_rec> taxa;
    for (uint32_t t = nt; t-- > 0;) taxa.push_back(targets[t]);
    for (uint64_t i = 0; i < mcq_taxdump_count(tax.h); ++i) taxa.push_back(mcq_taxdump_taxa(tax.h)[i]);

    // ---- 2b. -remove-ambig-features: once, on the union table (non_target_taxon_count() > 1, src/mode_build.cpp:729-730)
    std::string ambig_line;
    if (o.ambig_rank < MCQ_RANK_NONE && mcq_taxdump_count(tax.h) > 1) {
        std::vector<uint32_t> tgt_key(nt);
        if (o.ambig_rank == MCQ_RANK_SEQUENCE) for (uint32_t t = 0; t < nt; ++t) tgt_key[t] = t;
        else if (mcq_taxa_clade_keys(taxa.data(), taxa.size(), nt, o.ambig_rank, tgt_key.data())) return host_fail();
        uint64_t keys_before = 0, removed = 0;
        Table kept;
        if (mcq_table_info(table.h, &keys_before, nullptr, nullptr, nullptr, nullptr, nullptr) ||
            mcq_table_remove_ambiguous(table.h, tgt_key.data(), nt, (uint32_t)o.max_ambig, 0, &kept.h, &removed)) {
            std::fprintf(stderr, "ABORT: %s\n", mcq_build_last_error()); return 1;
        }
        table.reset();                                                       // (the unfiltered table goes before the rank split)
        std::swap(table.h, kept.h);
        ambig_line = "ambiguous features on rank " + std::string(mcq_rank_name(o.ambig_rank)) + " (more than " + std::to_string(o.max_ambig) +
                     " taxa): " + std::to_string(removed) + " of " + std::to_string(keys_before) + " removed\n";
        phase("remove ambiguous features");
    }

    // ---- 3. rank by rank: split on the device, copy, write
    mcq_shard_params sp;
    sp.k = sp.q_k = (uint64_t)o.kmerlen; sp.sketch_size = sp.q_sketch_size = (uint64_t)o.sketchlen;     // the query sketcher starts as the target
    sp.winlen = sp.q_winlen = (uint64_t)o.winlen; sp.winstride = sp.q_winstride = (uint64_t)o.winstride;   // sketcher (src/sketch_database.h:247-260)
    sp.max_locs_per_feature = (uint64_t)o.max_locs;
    double t_split = 0, t_write = 0;
    uint64_t keys_total = 0, locs_total = 0;
    std::vector<RankOut> outs(std::min(o.ranks_per_pass, o.P));
    for (uint32_t r0 = 0; r0 < o.P; r0 += (uint32_t)outs.size()) {
        const uint32_t nr = std::min<uint32_t>((uint32_t)outs.size(), o.P - r0);
        const auto ta = std::chrono::steady_clock::now();
        for (uint32_t i = 0; i < nr; ++i) {
            RankOut& R = outs[i];
            const uint32_t r = r0 + i;
            Table part;
            if (mcq_table_rank_split(table.h, o.P, r, &part.h)) { std::fprintf(stderr, "ABORT: %s\n", mcq_build_last_error()); return 1; }
            const uint32_t* dk = nullptr; const uint64_t *doff = nullptr, *dl = nullptr;
            if (mcq_table_info(part.h, &R.n_keys, &R.n_locs, &dk, &doff, &dl, nullptr)) { std::fprintf(stderr, "ABORT: %s\n", mcq_build_last_error()); return 1; }
            if (!R.keys.grow(R.n_keys) || !R.off.grow(R.n_keys + 1) || !R.locs.grow(R.n_locs)) return 1;
            if (R.n_keys) MCQ_HIP(hipMemcpy(R.keys.p, dk, R.n_keys * 4, hipMemcpyDeviceToHost), return 1);
            MCQ_HIP(hipMemcpy(R.off.p, doff, (R.n_keys + 1) * 8, hipMemcpyDeviceToHost), return 1);
            if (R.n_locs) MCQ_HIP(hipMemcpy(R.locs.p, dl, R.n_locs * 8, hipMemcpyDeviceToHost), return 1);
            R.taxa = taxa;
            for (uint32_t t = r; t < nt; t += o.P) R.taxa[nt - 1 - t].windows = windows[t];
            R.path = o.db + "_" + std::to_string(r);                         // src/mode_build.cpp:1079-1082
            keys_total += R.n_keys; locs_total += R.n_locs;
        }
        const auto tb = std::chrono::steady_clock::now();
        auto write = [&](RankOut& R) {
            R.rc = mcq_refdb_write_shard(R.path.c_str(), &sp, R.taxa.data(), R.taxa.size(), nt, R.keys.p, R.off.p, R.locs.p, R.n_keys);
            if (R.rc) R.err = mcq_host_last_error();                         // (the error text is per thread)
        };
        std::vector<std::thread> th;
        for (uint32_t i = 1; i < nr; ++i) th.emplace_back(write, std::ref(outs[i]));
        write(outs[0]);
        for (auto& x : th) x.join();
        for (uint32_t i = 0; i < nr; ++i) if (outs[i].rc) { std::fprintf(stderr, "ABORT: %s\n", outs[i].err.c_str()); return 1; }
        const auto tc = std::chrono::steady_clock::now();
        t_split += std::chrono::duration<double>(tb - ta).count(); t_write += std::chrono::duration<double>(tc - tb).count();
    }
    if (phase.on) std::fprintf(stderr, "[mcq_build_cli] %-28s %8.3f s\n[mcq_build_cli] %-28s %8.3f s\n", "rank split", t_split, "write", t_write);
    std::fputs(ambig_line.c_str(), stdout);
    std::printf("%u targets, %llu bases -> %u files %s_0 .. _%u: %llu keys, %llu locations\n", nt, (unsigned long long)n_bases, o.P, o.db.c_str(),
                o.P - 1, (unsigned long long)keys_total, (unsigned long long)locs_total);
    return 0;
}
