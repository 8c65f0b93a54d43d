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
//            [-device D] [-ranks-per-pass R] [-read-buffer BYTES] [-ranges N]
// -ranges N, and by itself a build whose one-piece temporaries do not fit: steps 2 and 3 run once per feature-hash range
// (build_in_ranges below): the sequences stay on the device and are sketched once per range.
// -remove-ambig-features RANK [-max-ambig-per-feature N, default 1]: a feature whose locations, over all P ranks and after the limit
// and -remove-overpopulated-features, name more than N distinct taxa at RANK (targets without one count as one taxon; the targets
// themselves for `sequence`) is left out of every file: remove_ambiguous_features (src/sketch_database.h:428-470) as the
// non-distributed post_process_features calls it (src/mode_build.cpp:729-747), on the whole database.  N is narrowed to 8 bits, then
// 0 becomes 1; RANK `none` or unknown leaves the option off (a warning); nothing happens when the dump holds at most one taxon.
// DIVERGENCE: the reference's `mpiexec -n P metacache_mpi build` accepts the options and ignores them (the call is commented out in
// post_process_features_distributed, src/mode_build.cpp:770-789, at every P): there is no reference file to compare with.
// Not reproduced: the order of the keys inside a file (the reference's hash table order; its reader inserts key by key, any order
// reads back the same), and the mapping of sequences to taxa through assembly_summary.txt / *.accession2taxid files: a target's
// parent is the N of "taxid|N" in its header, or 0.  The sequences must fit the GPU, and so must the temporaries of the one-piece
// build (about 60 B per feature slot: tens of Gbp on one MI355X) or of one range; MCQ_BUILD_TRACE=1 prints the times of the phases.
//
// -modify: `metacache_mpi modify DB NEW_GENOMES...` (main_mode_build_modify, src/mode_build.cpp:1117-1136: the database is read, its
// build options are taken from it, then the same add_to_database runs) on DB.db_0 .. DB.db_<P-1> -- which the reference's own MPI
// program cannot do on its sharded files (every rank opens DB.db).  The files are opened with mcq_refdb_open_meta: sketch parameters
// and bucket limit come from there; every file is streamed into mcq_table_extend_* (include/mcq.h), the new genomes are read as above
// by a reader that knows the database's names and target count (mcq_genome_reader_open_after), the extender's finish gives the union
// table of old and new, and step 2b and 3 go on as in a build.  The taxon list: old and new sequence-level taxa, last target first,
// then the dump's taxa with -taxonomy (reset_taxa_above_sequence_level), else the database's own above the sequences; the old
// sequence-level taxa keep name, parent, file and index.  -max-locations-per-feature N > 0 becomes the files' limit (below the
// database's value the old buckets are cut to their first N entries); without it the database's value stays.
// DIVERGENCES of -modify: -kmerlen, -sketchlen, -winlen, -winstride that differ from the database's end the run before anything is
// written (the reference parses them and goes on with the database's); every file is written as <name>.tmp and renamed once the last
// one is written, so a run that fails leaves the database as it was; -out NEWDB writes a second database.
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
    bool modify = false; std::string out_db;                                            // -modify [-out NEWDB]
    int64_t ranges = 0;                                                                 // -ranges N (0: not given)
    bool set_kmerlen = false, set_sketchlen = false, set_winlen = false, set_winstride = false, set_max_locs = false;
};

const char* kUsage =
    "usage: mcq_build_cli DB P GENOMES... -taxonomy DIR [-kmerlen K] [-sketchlen S] [-winlen W] [-winstride X]\n"
    "           [-max-locations-per-feature N] [-remove-overpopulated-features] [-remove-ambig-features RANK] [-max-ambig-per-feature N]\n"
    "           [-device D] [-ranks-per-pass R] [-read-buffer BYTES] [-ranges N]\n"
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
    "  -ranges N      builds the table in N ranges of the feature hash, one after the other: every range sketches the sequences again, its\n"
    "                 key records are made on the GPU and appended to the P files, which are written under temporary names and renamed after\n"
    "                 the last range.  For genomes whose one-piece build does not fit the GPU (about 60 B per feature slot); without the\n"
    "                 option the program goes this way by itself when it does not fit, with a number of ranges from the free memory.  The\n"
    "                 files hold what the one-piece build's hold; for N > 1 the keys inside a file come in another order.  -ranks-per-pass\n"
    "                 has no meaning here (host memory: one rank's records of one range); not with -modify\n"
    "       mcq_build_cli DB P NEW_GENOMES... -modify [-taxonomy DIR] [-remove-overpopulated-features] [-max-locations-per-feature N]\n"
    "           [-remove-ambig-features RANK [-max-ambig-per-feature N]] [-out NEWDB] [-device D] [-ranks-per-pass R] [-read-buffer BYTES]\n"
    "  -modify        adds the sequences of NEW_GENOMES to the existing DB.db_0 .. DB.db_<P-1> (`metacache_mpi modify DB GENOMES...`): the files\n"
    "                 then hold what a build of the old and the new genomes together writes.  New sequences get the target ids behind the\n"
    "                 old ones; a sequence whose name the database has, or that came earlier in this run, is skipped; a bucket keeps its first\n"
    "                 -max-locations-per-feature entries, the old ones first (N below the database's value shrinks the old buckets, N becomes\n"
    "                 the files' value; default: the database's); -remove-overpopulated-features works on old and new together; with -taxonomy\n"
    "                 the taxa above the sequences are replaced by the dump's, without it they are kept.  k, sketch size, window length and\n"
    "                 stride are the database's.  Divergences: -kmerlen / -sketchlen / -winlen / -winstride that differ from the database's\n"
    "                 end the run (the reference parses and ignores them); the files are written under temporary names and renamed after\n"
    "                 the last one, so a run that fails leaves DB as it was; -out NEWDB writes NEWDB.db_* and leaves DB untouched.\n"
    "                 Limits: the old locations and the new sketches go through the one-piece build on the GPU together (about 12 B per old\n"
    "                 location, then about 44 B per old location and new feature slot); fewer than 2^32 windows in all\n"
    "not supported: assembly_summary.txt / *.accession2taxid mapping files (a target's parent is the N of 'taxid|N' in its\n"
    "header, else none), FASTQ genome files; the key order inside a file is not the reference's\n";

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
        else if (opt_named(a, {"-kmerlen"})) { o.kmerlen = std::atoi(next()); o.set_kmerlen = true; }
        else if (opt_named(a, {"-sketchlen"})) { o.sketchlen = std::atoi(next()); o.set_sketchlen = true; }
        else if (opt_named(a, {"-winlen"})) { o.winlen = std::atoi(next()); o.set_winlen = true; }
        else if (opt_named(a, {"-winstride"})) { o.winstride = std::atoi(next()); o.set_winstride = true; }
        else if (opt_named(a, {"-max-locations-per-feature", "-max_locations_per_feature"})) { o.max_locs = std::atoi(next()); o.set_max_locs = o.max_locs > 0; }
        else if (opt_named(a, {"-modify"})) o.modify = true;
        else if (opt_named(a, {"-out"})) o.out_db = next();
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
        else if (opt_named(a, {"-ranges"})) {
            o.ranges = std::strtoll(next(), nullptr, 10);
            if (o.ranges < 1 || o.ranges > 0xFFFFFFFFll) { std::fprintf(stderr, "ABORT: -ranges N needs N >= 1\n"); return false; }
        }
        else { std::fprintf(stderr, "ABORT: unknown option %s\n%s", a.c_str(), kUsage); return false; }
    }
    if (o.P < 1 || o.P > 64) { std::fprintf(stderr, "ABORT: P must be 1..64\n"); return false; }
    if (o.inputs.empty()) { std::fprintf(stderr, "ABORT: Nothing to do - no reference sequences provided.\n"); return false; }
    if (o.taxonomy.empty() && !o.modify) { std::fprintf(stderr, "ABORT: -taxonomy DIR is required\n"); return false; }
    if (!o.out_db.empty() && !o.modify) { std::fprintf(stderr, "ABORT: -out NEWDB goes with -modify\n"); return false; }
    if (o.modify && o.ranges) { std::fprintf(stderr, "ABORT: -modify works on the whole table: -ranges goes with a build\n"); return false; }
    if (!o.out_db.empty() && o.out_db.find(".db") == std::string::npos) o.out_db += ".db";
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
struct RefDb { mcq_refdb* h = nullptr; ~RefDb() { mcq_refdb_close(h); } };
struct ShardStream { mcq_shard_stream* h = nullptr; ~ShardStream() { mcq_shard_stream_close(h); } };
struct Extender { mcq_table_extend* h = nullptr; ~Extender() { mcq_table_extend_free(h); } };
// -modify writes its files under temporary names; they get their own once the last one is written: a run that ends before that
// takes its temporary files away and leaves the database that was there.  (A build writes under the final names, as it always did.)
struct OutFiles {
    const bool temporary;
    std::vector<std::pair<std::string, std::string>> names;      // (temporary, final)
    bool kept = false;
    explicit OutFiles(bool t) : temporary(t) {}
    std::string add(const std::string& path) { if (!temporary) return path; names.emplace_back(path + ".tmp", path); return names.back().first; }
    bool commit() {
        for (const auto& n : names)
            if (std::rename(n.first.c_str(), n.second.c_str())) { std::fprintf(stderr, "ABORT: can't rename %s to %s\n", n.first.c_str(), n.second.c_str()); return false; }
        return kept = true;
    }
    ~OutFiles() { if (!kept) for (const auto& n : names) std::remove(n.first.c_str()); }
};

// one rank's table and taxon list in host memory
struct RankOut {
    PinnedBuf<uint32_t> keys; PinnedBuf<uint64_t> off, locs; uint64_t n_keys = 0, n_locs = 0;
    std::vector<mcq_taxon_rec> taxa; std::string path; int rc = 0; std::string err;
};

int host_fail() { std::fprintf(stderr, "ABORT: %s\n", mcq_host_last_error()); return 1; }
int build_fail() { std::fprintf(stderr, "ABORT: %s\n", mcq_build_last_error()); return 1; }

// The taxon list: sequence-level taxa (id -(target + 1): the last target first) before the taxonomy's, both in ascending id
// (src/taxonomy.h:290-294, :348).  -modify: the taxa above the sequences are the dump's if one is given
// (reset_taxa_above_sequence_level), else the database's own.
std::vector<mcq_taxon_rec> taxon_list(const std::vector<mcq_taxon_rec>& targets, const mcq_taxdump* dump, const std::vector<mcq_taxon_rec>& old_taxa) {
    std::vector<mcq_taxon_rec> taxa;
    for (size_t t = targets.size(); t-- > 0;) taxa.push_back(targets[t]);
    if (dump) for (uint64_t i = 0; i < mcq_taxdump_count(dump); ++i) taxa.push_back(mcq_taxdump_taxa(dump)[i]);
    else for (const mcq_taxon_rec& x : old_taxa) if (x.id >= 0) taxa.push_back(x);
    return taxa;
}
// -remove-ambig-features: is it on (non_target_taxon_count() > 1, src/mode_build.cpp:729-730), and the targets' keys at the rank
bool ambig_on(const BuildOptions& o, const std::vector<mcq_taxon_rec>& taxa, uint32_t nt) { return o.ambig_rank < MCQ_RANK_NONE && taxa.size() - nt > 1; }
bool ambig_keys(const BuildOptions& o, const std::vector<mcq_taxon_rec>& taxa, uint32_t nt, std::vector<uint32_t>& tgt_key) {
    tgt_key.resize(nt);
    if (o.ambig_rank == MCQ_RANK_SEQUENCE) { for (uint32_t t = 0; t < nt; ++t) tgt_key[t] = t; return true; }
    return mcq_taxa_clade_keys(taxa.data(), taxa.size(), nt, o.ambig_rank, tgt_key.data()) == 0;
}
std::string ambig_text(const BuildOptions& o, uint64_t removed, uint64_t keys_before) {
    return "ambiguous features on rank " + std::string(mcq_rank_name(o.ambig_rank)) + " (more than " + std::to_string(o.max_ambig) +
           " taxa): " + std::to_string(removed) + " of " + std::to_string(keys_before) + " removed\n";
}
// the sketch parameters of a file: the query sketcher starts as the target sketcher (src/sketch_database.h:247-260)
mcq_shard_params shard_params(const BuildOptions& o) {
    mcq_shard_params sp;
    sp.k = sp.q_k = (uint64_t)o.kmerlen; sp.sketch_size = sp.q_sketch_size = (uint64_t)o.sketchlen;
    sp.winlen = sp.q_winlen = (uint64_t)o.winlen; sp.winstride = sp.q_winstride = (uint64_t)o.winstride;
    sp.max_locs_per_feature = (uint64_t)o.max_locs;
    return sp;
}

struct RangeBuild { mcq_range_build* h = nullptr; ~RangeBuild() { mcq_range_build_free(h); } };
struct ShardWriters {
    std::vector<mcq_shard_writer*> w;
    ~ShardWriters() { for (mcq_shard_writer* x : w) mcq_shard_writer_close(x); }
    bool close() {                       // every file is closed, whatever the ones before it said
        bool ok = true;
        for (mcq_shard_writer*& x : w) { if (mcq_shard_writer_close(x)) ok = false; x = nullptr; }
        return ok;
    }
};

// ---- the build in feature ranges (-ranges N, or by itself when the one-piece build does not fit): steps 2 and 3 of a build, one
// range of the union table at a time (mcq_range_build_* of include/mcq.h: every range sketches the sequences again).  All P files are
// open from the start, under temporary names; a range's table is filtered (-remove-ambig-features: a per-feature filter, so per range it
// is the same filter), then every rank's key records are made on the GPU as the bytes of its file (mcq_table_shard_records), copied to
// a pinned block and appended (mcq_shard_writer_*).  The files get their names after the last range: a run that fails leaves none.
// Host memory: one rank's records of one range.  The keys of a file come range by range, in ascending feature order inside a range.
int build_in_ranges(const BuildOptions& o, const mcq_build_desc& d, uint32_t n_ranges, const std::vector<mcq_taxon_rec>& targets,
                    const mcq_taxdump* dump, uint64_t n_bases, Phases& phase) {
    const uint32_t nt = d.n_targets;
    RangeBuild build;
    if (mcq_range_build_create(&d, n_ranges, &build.h) || mcq_range_build_info(build.h, &n_ranges, nullptr, nullptr)) return build_fail();
    std::vector<uint32_t> windows(nt);
    if (mcq_range_build_tgt_windows(build.h, windows.data())) return build_fail();
    const std::vector<mcq_taxon_rec> taxa = taxon_list(targets, dump, {});
    std::vector<uint32_t> tgt_key;
    const bool ambig = ambig_on(o, taxa, nt);
    if (ambig && !ambig_keys(o, taxa, nt, tgt_key)) return host_fail();
    phase("windows");

    const mcq_shard_params sp = shard_params(o);
    OutFiles files_out(true);
    ShardWriters writers;
    writers.w.assign(o.P, nullptr);
    {
        for (uint32_t r = 0; r < o.P; ++r) {
            std::vector<mcq_taxon_rec> mine = taxa;
            for (uint32_t t = r; t < nt; t += o.P) mine[nt - 1 - t].windows = windows[t];                    // `windows` is set for the targets the rank owns
            const std::string path = files_out.add(o.db + "_" + std::to_string(r));                          // src/mode_build.cpp:1079-1082
            if (mcq_shard_writer_open(path.c_str(), &sp, mine.data(), mine.size(), nt, &writers.w[r])) return host_fail();
        }
    }
    DeviceBuf<unsigned char> d_rec; PinnedBuf<unsigned char> h_rec;
    uint64_t keys_total = 0, locs_total = 0, keys_before = 0, removed_total = 0;
    double t_build = 0, t_ambig = 0, t_records = 0, t_write = 0;
    auto seconds = [](std::chrono::steady_clock::time_point a) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - a).count(); };
    for (uint32_t range = 0; range < n_ranges; ++range) {
        auto t0 = std::chrono::steady_clock::now();
        Table table;
        if (mcq_range_build_next(build.h, &table.h)) return build_fail();
        if (!table.h) { std::fprintf(stderr, "ABORT: the build ended after %u of %u ranges\n", range, n_ranges); return 1; }
        t_build += seconds(t0); t0 = std::chrono::steady_clock::now();
        if (ambig) {
            uint64_t before = 0, removed = 0;
            Table kept;
            if (mcq_table_info(table.h, &before, nullptr, nullptr, nullptr, nullptr, nullptr) ||
                mcq_table_remove_ambiguous(table.h, tgt_key.data(), nt, (uint32_t)o.max_ambig, 0, &kept.h, &removed)) return build_fail();
            table.reset();
            std::swap(table.h, kept.h);
            keys_before += before; removed_total += removed;
            t_ambig += seconds(t0);
        }
        for (uint32_t r = 0; r < o.P; ++r) {
            t0 = std::chrono::steady_clock::now();
            uint64_t nb = 0, nk = 0, nl = 0;
            if (mcq_table_shard_records(table.h, o.P, r, nullptr, 0, &nb, &nk, &nl)) return build_fail();
            if (!d_rec.grow(nb) || !h_rec.grow(nb)) return 1;
            if (nb) {
                if (mcq_table_shard_records(table.h, o.P, r, d_rec.p, d_rec.cap, &nb, &nk, &nl)) return build_fail();
                MCQ_HIP(hipMemcpy(h_rec.p, d_rec.p, nb, hipMemcpyDeviceToHost), return 1);
            }
            t_records += seconds(t0); t0 = std::chrono::steady_clock::now();
            if (mcq_shard_writer_append(writers.w[r], h_rec.p, nb, nk, nl)) return host_fail();
            t_write += seconds(t0);
            keys_total += nk; locs_total += nl;
        }
    }
    const auto t0 = std::chrono::steady_clock::now();
    if (!writers.close()) return host_fail();
    t_write += seconds(t0);
    if (phase.on) {
        const struct { const char* name; double t; } rows[] = {{"sketch + sort (ranges)", t_build}, {"remove ambiguous features", t_ambig},
                                                                 {"key records", t_records}, {"write", t_write}};
        for (const auto& x : rows) std::fprintf(stderr, "[mcq_build_cli] %-28s %8.3f s\n", x.name, x.t);
    }
    if (!files_out.commit()) return 1;
    if (ambig) std::fputs(ambig_text(o, removed_total, keys_before).c_str(), stdout);
    std::printf("%u targets, %llu bases -> %u files %s_0 .. _%u: %llu keys, %llu locations", nt, (unsigned long long)n_bases, o.P, o.db.c_str(),
                o.P - 1, (unsigned long long)keys_total, (unsigned long long)locs_total);
    if (phase.on) std::printf(" (%u ranges)", n_ranges);
    std::printf("\n");
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    BuildOptions o;
    if (!parse(argc, argv, o)) return 2;
    Phases phase;
    MCQ_HIP(hipSetDevice(o.device), return 1);
    // ---- 0. -modify: the database that is there -- its sketch parameters and bucket limit are the run's (get_build_options_from_db,
    // src/mode_build.cpp:1117-1136); an option that asks for another sketch ends the run here, where the reference goes on with the
    // database's value in silence
    RefDb old;
    mcq_refdb_info old_info; std::memset(&old_info, 0, sizeof(old_info));
    if (o.modify) {
        if (o.db.size() < 3 || o.db.compare(o.db.size() - 3, 3, ".db") != 0) { std::fprintf(stderr, "ABORT: -modify: the database name must end in .db (%s)\n", o.db.c_str()); return 1; }
        if (mcq_refdb_open_meta(o.db.substr(0, o.db.size() - 3).c_str(), o.P, &old.h) || mcq_refdb_get_info(old.h, &old_info)) return host_fail();
        const struct { const char* name; bool set; int asked; uint32_t has; } sk[] = {
            {"-kmerlen", o.set_kmerlen, o.kmerlen, old_info.k}, {"-sketchlen", o.set_sketchlen, o.sketchlen, old_info.sketch_size},
            {"-winlen", o.set_winlen, o.winlen, old_info.winlen}, {"-winstride", o.set_winstride, o.winstride, old_info.winstride}};
        for (const auto& x : sk)
            if (x.set && (int64_t)x.asked != (int64_t)x.has) {
                std::fprintf(stderr, "ABORT: %s %d differs from the database's %u: -modify sketches with the database's parameters\n", x.name, x.asked, x.has);
                return 1;
            }
        o.kmerlen = (int)old_info.k; o.sketchlen = (int)old_info.sketch_size; o.winlen = (int)old_info.winlen; o.winstride = (int)old_info.winstride;
        if (!o.set_max_locs) o.max_locs = (int)std::min<uint32_t>(std::max<uint32_t>(old_info.max_locs_per_feature, 1), 254);
    }
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
    if (!o.taxonomy.empty() && mcq_taxdump_read(o.taxonomy.c_str(), &tax.h)) return host_fail();      // (optional with -modify)

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
    const uint64_t io_bytes = std::min<uint64_t>(o.read_buffer, 16u << 20);
    if (o.modify ? mcq_genome_reader_open_after(paths.data(), (uint32_t)paths.size(), io_bytes, old.h, &reader.h)
                 : mcq_genome_reader_open(paths.data(), (uint32_t)paths.size(), io_bytes, &reader.h)) return host_fail();
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
    // targets: the database's (-modify), then the ones read now, with the ids that go on behind them
    const uint32_t n_old = old_info.n_targets, n_new = mcq_genome_reader_n_targets(reader.h);
    if ((uint64_t)n_old + n_new >= 0xFFFFFFFFull) { std::fprintf(stderr, "ABORT: more targets than a 32-bit target id holds\n"); return 1; }
    const uint32_t nt = n_old + n_new;
    if (nt < 1 || (!o.modify && n_new < 1)) { std::fprintf(stderr, "ABORT: no reference sequence found in the genome files\n"); return 1; }
    std::vector<mcq_taxon_rec> targets(nt), old_taxa(old_info.n_taxa);
    if (o.modify) {
        if (mcq_refdb_taxa(old.h, old_taxa.data())) return host_fail();
        std::vector<bool> seen(n_old, false);
        for (const mcq_taxon_rec& x : old_taxa)
            if (x.id < 0 && (uint64_t)(-x.id - 1) < n_old) { targets[(size_t)(-x.id - 1)] = x; targets[(size_t)(-x.id - 1)].windows = 0; seen[(size_t)(-x.id - 1)] = true; }
        for (uint32_t t = 0; t < n_old; ++t)
            if (!seen[t]) { std::fprintf(stderr, "ABORT: the database holds no taxon for its target %u\n", t); return 1; }
    }
    std::vector<uint64_t> seq_off((size_t)n_new + 1, 0);
    for (uint32_t t = 0; t < n_new; ++t) {
        uint64_t len = 0;
        if (mcq_genome_reader_target(reader.h, t, &targets[n_old + t], &len)) return host_fail();
        seq_off[t + 1] = seq_off[t] + len;
    }
    DeviceBuf<uint64_t> d_seq_off;
    if (!d_seq_off.grow((uint64_t)n_new + 1)) return 1;
    MCQ_HIP(hipMemcpy(d_seq_off.p, seq_off.data(), ((size_t)n_new + 1) * 8, hipMemcpyHostToDevice), return 1);
    stage[0] = PinnedBuf<char>(); stage[1] = PinnedBuf<char>();              // (the read buffers are not needed any more)
    phase("read");

    // ---- 2. the union of the P rank tables
    Table table;
    if (o.modify) {
        // what the files hold goes to the extender file by file, chunk by chunk (mcq_shard_stream_*), then the new sequences
        std::vector<uint32_t> old_windows(n_old);
        if (mcq_refdb_tgt_windows(old.h, old_windows.data())) return host_fail();
        mcq_table_extend_desc d; std::memset(&d, 0, sizeof(d));
        d.k = old_info.k; d.sketch_size = old_info.sketch_size; d.winlen = old_info.winlen; d.winstride = old_info.winstride;
        d.n_ranks = o.P; d.max_locs = (uint32_t)o.max_locs; d.flags = o.remove_overpopulated ? MCQ_BUILD_REMOVE_OVERPOPULATED : 0; d.device = o.device;
        d.n_old_targets = n_old; d.old_tgt_windows = old_windows.data(); d.expected_old_locations = old_info.n_locs;
        Extender ext;
        if (mcq_table_extend_create(&d, &ext.h)) { std::fprintf(stderr, "ABORT: %s\n", mcq_build_last_error()); return 1; }
        uint64_t largest = 0;
        for (uint32_t r = 0; r < o.P; ++r) { uint64_t nl = 0; if (mcq_refdb_file_stats(old.h, r, nullptr, nullptr, &nl)) return host_fail(); largest = std::max(largest, nl); }
        const uint64_t chunk = std::min<uint64_t>(largest + 255, 1u << 22);           // (a chunk takes whole key records: at most 255 locations each)
        PinnedBuf<uint32_t> cf, ct, cw;
        if (!cf.grow(chunk) || !ct.grow(chunk) || !cw.grow(chunk)) return 1;
        for (uint32_t r = 0; r < o.P; ++r) {
            ShardStream in;
            if (mcq_shard_stream_open(old.h, r, &in.h)) return host_fail();
            for (;;) {
                uint64_t n = 0;
                if (mcq_shard_stream_next(in.h, cf.p, ct.p, cw.p, chunk, &n)) return host_fail();
                if (!n) break;
                if (mcq_table_extend_add(ext.h, cf.p, ct.p, cw.p, n, 0)) { std::fprintf(stderr, "ABORT: %s_%u: %s\n", o.db.c_str(), r, mcq_build_last_error()); return 1; }
            }
        }
        phase("old locations");
        if (mcq_table_extend_finish(ext.h, d_bases.p, d_seq_off.p, n_new, MCQ_DEVICE_PTRS, &table.h)) { std::fprintf(stderr, "ABORT: %s\n", mcq_build_last_error()); return 1; }
        ext.h = nullptr;                                                         // (finish has released it)
    } else {
        mcq_build_desc d; std::memset(&d, 0, sizeof(d));
        d.k = (uint32_t)o.kmerlen; d.sketch_size = (uint32_t)o.sketchlen; d.winlen = (uint32_t)o.winlen; d.winstride = (uint32_t)o.winstride;
        d.n_targets = nt; d.bases = d_bases.p; d.seq_off = d_seq_off.p; d.emulate_ranks = o.P; d.max_locs = (uint32_t)o.max_locs;
        d.flags = MCQ_DEVICE_PTRS | (o.remove_overpopulated ? MCQ_BUILD_REMOVE_OVERPOPULATED : 0); d.device = o.device;
        // in feature ranges when asked to (-ranges N), or when the one-piece temporaries (about 60 B per feature slot) would not leave
        // room for the table: mcq_db_build's test, with the sequences on the device; the library then derives the number of ranges
        bool in_ranges = o.ranges > 0;
        if (!in_ranges) {
            size_t mem_free = 0, mem_total = 0;
            MCQ_HIP(hipMemGetInfo(&mem_free, &mem_total), return 1);
            const uint64_t slots = n_bases / (uint64_t)o.winstride * (uint64_t)o.sketchlen;
            in_ranges = slots * 60 > mem_free / 2;
        }
        if (in_ranges) return build_in_ranges(o, d, (uint32_t)o.ranges, targets, tax.h, n_bases, phase);
        if (mcq_build_table(&d, &table.h)) { std::fprintf(stderr, "ABORT: %s\n", mcq_build_last_error()); return 1; }
    }
    d_bases = DeviceBuf<char>();
    std::vector<uint32_t> windows(nt);
    if (mcq_table_tgt_windows(table.h, windows.data())) { std::fprintf(stderr, "ABORT: %s\n", mcq_build_last_error()); return 1; }
    phase("sketch + sort");

    const std::vector<mcq_taxon_rec> taxa = taxon_list(targets, tax.h, old_taxa);

    // ---- 2b. -remove-ambig-features: once, on the union table
    std::string ambig_line;
    if (ambig_on(o, taxa, nt)) {
        std::vector<uint32_t> tgt_key;
        if (!ambig_keys(o, taxa, nt, tgt_key)) return host_fail();
        uint64_t keys_before = 0, removed = 0;
        Table kept;
        if (mcq_table_info(table.h, &keys_before, nullptr, nullptr, nullptr, nullptr, nullptr) ||
            mcq_table_remove_ambiguous(table.h, tgt_key.data(), nt, (uint32_t)o.max_ambig, 0, &kept.h, &removed)) {
            std::fprintf(stderr, "ABORT: %s\n", mcq_build_last_error()); return 1;
        }
        table.reset();                                                       // (the unfiltered table goes before the rank split)
        std::swap(table.h, kept.h);
        ambig_line = ambig_text(o, removed, keys_before);
        phase("remove ambiguous features");
    }

    // ---- 3. rank by rank: split on the device, copy, write
    const std::string& out_db = o.out_db.empty() ? o.db : o.out_db;
    OutFiles files_out(o.modify);
    mcq_shard_params sp = shard_params(o);
    if (o.modify) { sp.q_sketch_size = old_info.q_sketch_size; sp.q_winlen = old_info.q_winlen; sp.q_winstride = old_info.q_winstride; }     // (the query sketcher stays the database's)
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
            R.path = files_out.add(out_db + "_" + std::to_string(r));      // src/mode_build.cpp:1079-1082
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
    if (!files_out.commit()) return 1;
    if (o.modify) std::printf("%u sequences added to %u, %llu skipped (their names were taken)\n", n_new, n_old, (unsigned long long)mcq_genome_reader_n_skipped(reader.h));
    std::fputs(ambig_line.c_str(), stdout);
    std::printf("%u targets, %llu bases -> %u files %s_0 .. _%u: %llu keys, %llu locations\n", nt, (unsigned long long)n_bases, o.P, out_db.c_str(),
                o.P - 1, (unsigned long long)keys_total, (unsigned long long)locs_total);
    return 0;
}
