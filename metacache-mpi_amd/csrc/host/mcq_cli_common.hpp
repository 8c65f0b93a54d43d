#pragma once
// mcq_cli_common.hpp -- what mcq_query_cli (one GPU) and mcq_query_mpi (one process per GPU under mpiexec) share: the
// options, the opening of the database and the writers of the reference's -out file.
//
// mcq_query_cli -- stand-in for `mpiexec -n P metacache query <db> r1.fq r2.fq -pairfiles ...`
// (src/mode_query.cpp:404-458) around the engine: reads the reference's shard files, runs the per-read path on
// the GPU through the C ABI, classifies on the host and writes what the reference writes to its -out file:
//   * the parameter lines                      show_query_parameters    src/printing.cpp:40-113
//   * "# TABLE_LAYOUT: ..."                    show_query_mapping_header src/classification.cpp:486-512, printing.cpp:243-300
//   * "# <file1> + <file2>"                    src/querying.h:1337
//   * one mapping line per read (pair)         show_query_mapping       src/classification.cpp:583-632
//         taxon formats (rank:name default, -taxids, -taxids-only, -omit-ranks, -lineage)  show_taxon / show_lineage /
//         show_no_taxon src/printing.cpp:117-201, :305-330;  -tophits list  show_matches src/printing.cpp:333-360
//   * -abundances / -abundance-per R tables   show_abundances / show_abundance_estimates src/printing.cpp:474-517,
//                                              estimate_abundance src/classification.cpp:362-428 (mcq_refdb_abundance_text)
//         after the mapping lines, into the -out file or the -abundances FILE (src/mode_query.cpp:59-117); the counts come
//         from the device (mcq_classify), checked against the host classification's total
//   * -hits-per-seq [FILE] (mcq_query_cli only)  show_matches_per_targets src/printing.cpp:437-469 (mcq_hits_table_text) after the
//         mapping lines and in front of the abundance tables (src/classification.cpp:847-862), into the -out file or FILE; the
//         query_id column of the TABLE_LAYOUT and of every mapping line, two parameter lines
//   * -queryids                                the query_id column of the TABLE_LAYOUT and of every mapping line (showQueryIds,
//         src/query_options.cpp:249-250, :308: -hits-per-seq sets the same flag)
//   * -locations                               the candidate_locations column behind top_hits: show_candidate_ranges
//         src/printing.cpp:422-432, `[w * win_beg,w * win_end + winlen] ` per candidate; after a fold (n_ranks > 1) the candidates
//         carry (0,0) and every entry is `[0,<winlen>] `, as in the reference's MPI program
//   * -allhits (mcq_query_cli only)             the all_hits column in front of top_hits: show_matches over match locations
//         src/printing.cpp:365-416, one `name/win:count,` (-lowest sequence) or `ancestorname:count,` per distinct (target, window)
//         of the read, from mcq_all_hits on the GPU; sets the map view mode to `all` (src/query_options.cpp:293-297); with -exclude
//         the entries on the read's own clade are left out on the host
//   * -align (mcq_query_cli only)               show_alignment src/classification.cpp:437-477 behind the classification column of a
//         classified read whose first candidate is a sequence (mcq_align on the GPU, mcq_align_subjects.hpp), one parameter line
//         (src/printing.cpp:91-93); -align-candidate-range, written into no output, aligns against the candidate's real window range
//         where the fold has zeroed it
//   * the summary                              show_summary             src/printing.cpp:622-641,
//                                              show_taxon_statistics    src/printing.cpp:522-600 (mcq_eval_stats_text)
//   * -exclude RANK / -ground-truth / -precision (mcq_query_cli only; get_evaluation_options, src/query_options.cpp:190-213):
//         the read's truth from its whole header (mcq_refdb_ground_truth, against the whole database), the "Clade Exclusion on
//         Rank" parameter line (src/printing.cpp:75-78, which ends without a newline), the truth_ column of the TABLE_LAYOUT and
//         of every mapping line (src/classification.cpp:499-502, :611-614), assign_known_correct and the "ground truth" blocks of
//         the summary.  The truth stays with the read up to its evaluation; the reference's MPI program loses it on rank 0
//         (DESIGN.md section 16).  -taxon-coverage is rejected; mcq_query_mpi rejects all of them.
// After sorting, the file equals the reference's byte for byte except for the measured values of the "# time:" and
// "# speed:" lines (tests/test_gpu_cli.py).  Not reproduced: the reference prints nothing for a thread's chunk in which
// no read was classified (src/querying.h:1091, :1129).
//
// usage: mcq_query_cli <dbprefix> <n_ranks> <file|directory>... [-pairfiles | -pairseq] [-splitout PREFIX] [-lowest R] [-highest R]
//            [-maxcand N] [-hitmin N] [-hitdiff X] [-insertsize N] [-threads N] [-tophits] [-taxids] [-taxids-only] [-omit-ranks]
//            [-lineage] [-mapped-only] [-nomap] [-noquirks] [-abundances [FILE]] [-abundance-per R] [-out FILE] [-batch N]
//            [-batch-bases N] [-read-chunk BYTES] [-reader gpu|host] [-exclude RANK] [-ground-truth] [-precision] [-hits-per-seq [FILE]]
//            [-align] [-align-candidate-range] [-queryids] [-locations] [-allhits] [-winlen N] [-winstride N] [-sketchlen N]
//            [-max-locations-per-feature N] [-remove-overpopulated-features] [-help]
// (inputs: every argument up to the first option; a directory stands for the files in it (files_in_directory below).  -pairseq
//  without -pairfiles comes first: every file is interleaved pairs, also the two of `r1 r2` and the one of `r1 -`.  Without it,
//  `r1 r2` alone is one pair of files in the given order and `r1 -` one single-end file.  Otherwise -pairfiles sorts the names and pairs
//  consecutive ones (src/mode_query.cpp:409-411, src/querying.h:1329-1340; an odd count is an error), -pairseq takes every file
//  as interleaved pairs (sequence_pair_reader::next, src/sequence_io.cpp:442-462), and without either every file is single-end,
//  in the given order.  Each unit's mapping lines follow its "# f1 + f2" / "# f1" line; statistics and abundances add up over
//  all units.  -splitout PREFIX (-split-out): one output per unit instead, PREFIX_<name1>[_<name2>].txt, each with its own
//  head, summary and abundance tables, src/mode_query.cpp:170-229; -out FILE, if given, is the prefix: src/query_options.cpp:343-351;
//  -list-inputs (written into no output): print the pairing mode and one line per unit -- its "f1 + f2" / "f1" text, under -splitout a
//  tab and its output file -- and leave before the database is opened;
//  -batch / -batch-bases: queries / bases per batch; the reads go through in batches, see mcq_read_batches.hpp;
//  -read-chunk / -reader (mcq_query_cli only, written into no output): bytes per read() of each file, default 8 MiB, and
//  who parses the chunks -- the GPU (mcq_reads_prepare; a chunk not in the strict form goes to the host) or always the host;
//  -abundances [FILE] / -abundance-per R (aliases -abundances-per, -abundance_per, -abundances_per): src/query_options.cpp:310-323)
#include <dirent.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <initializer_list>
#include <iostream>
#include <string>
#include <vector>

#include "../../../include/mcq.h"
#include "../../../include/mcq_host.h"
#include "../../../include/mcq_open.hpp"
#include "mcq_read_unit.hpp"

// How a taxon is written (the reference's taxon_print_mode, src/query_options.h:68-71; output of src/printing.cpp:117-176,
// :243-300) as two independent choices: an optional "<rank>:" prefix, and one of three bodies -- name, id, name(id).
struct Mode {
    bool rank_prefix; int body;                          // body: 0 = name, 1 = id, 2 = name(id)
    static constexpr Mode make(bool show_ranks, bool taxids, bool taxids_only) { return Mode{show_ranks, taxids_only ? 1 : (taxids ? 2 : 0)}; }
    bool ids_only() const { return body == 1; }
};

struct Options {
    std::string prefix, outfile;
    std::vector<ReadUnit> units;         // the inputs, in the order they are read and written (make_units)
    enum Pairing { NONE, FILES, SEQUENCES } pairing = NONE;   // the reference's pairing_mode (src/query_options.cpp:82-97)
    bool split = false;                  // -splitout: one output per unit
    bool list_inputs = false;            // -list-inputs: print the units and leave
    uint32_t P = 1;                      // ranks of the reference build / run whose results are reproduced
    uint32_t lowest = MCQ_RANK_SEQUENCE, highest = MCQ_RANK_DOMAIN, maxcand = 2, hitmin = 0, threads = 1;
    float hitdiff = 1.0f; uint64_t insertsize = 0; bool quirks = true;
    bool show_ranks = true, taxids = false, taxids_only = false, lineage = false, tophits = false, mapped_only = false, nomap = false;
    bool abundances = false;             // -abundances [FILE]: the plain per-taxon table
    std::string abundance_file;          // ... its FILE (cleared when it names the -out file: src/query_options.cpp:355)
    uint32_t abundance_rank = MCQ_RANK_NONE;   // -abundance-per R: the estimate to rank R (< root)
    bool tax_counts() const { return abundances || abundance_rank != MCQ_RANK_NONE; }
    bool align = false;                  // -align: the alignment block behind the line of a read classified to a sequence
    bool align_range = false;            // -align-candidate-range: align against the candidate's real window range, not the folded (0,0)
    bool query_ids = false;              // -queryids, and set by -hits-per-seq: the query_id column (showQueryIds)
    bool locations = false;              // -locations: the candidate_locations column
    bool allhits = false;                // -allhits: the all_hits column (mcq_query_cli)
    bool hits_per_seq = false;           // -hits-per-seq [FILE]: the per-reference window hit lists, and the query_id column
    std::string hits_file;               // ... its FILE (cleared when it names the -out file: src/query_options.cpp:353)
    bool coverage = false;               // -coverage [FILE]: the report of window coverage per reference sequence (mcq_query_cli)
    std::string coverage_file;           // ... its FILE (cleared when it names the -out file)
    double cov_percentile = -1;          // -cov-percentile P (0..100; below 0: not given): two passes, the least covered sequences removed
    bool cov_cut() const { return cov_percentile >= 0; }
    bool cov_on() const { return coverage || cov_cut(); }
    uint32_t exclude_rank = MCQ_RANK_NONE;     // -exclude R (< root): drop the hits on the read's own clade at R
    bool ground_truth = false, precision = false;   // -ground-truth: the truth_ column; -precision: the evaluation statistics
    bool wants_truth() const { return ground_truth || precision || exclude_rank != MCQ_RANK_NONE; }   // prepare_evaluation, src/classification.cpp:172-177
    std::string transport = "rccl";      // mcq_query_mpi: rccl | mpi (blocks through the host and MPI_Alltoallv)
    uint64_t batch = 1u << 19, batch_bases = 256u << 20;   // mcq_query_mpi: queries / bases per rank and batch
    uint64_t read_chunk = 8u << 20;      // mcq_query_cli: bytes per file and chunk (-read-chunk)
    bool host_reader = false;            // mcq_query_cli: -reader host
    mcq_query_tuning tuning;             // -winlen, -winstride, -sketchlen, -max-locations-per-feature, -remove-overpopulated-features
    bool paired() const { return pairing != NONE; }
};

// an option under any of its spellings (the reference's args.get / args.contains take a list of them, e.g. src/mode_build.cpp:113-122)
static inline bool opt_named(const std::string& a, std::initializer_list<const char*> names) {
    for (const char* n : names) if (a == n) return true;
    return false;
}

// The files a directory stands for: files_in_directory (src/filesys_utility.cpp:32-73), which sequence_filenames
// (src/args_handling.cpp:50-90) applies to every input name -- every entry but "." and "..", a subdirectory (10 levels) replaced
// by what it holds, an entry that holds nothing (a file, an empty directory) by its own path.  The reference keeps readdir's
// order, which no two file systems share; here the entries of a directory go in the order of their names.
static std::vector<std::string> files_in_directory(std::string dir, int recurse = 10) {
    if (!dir.empty() && (dir.back() == '/' || dir.back() == '\\')) dir.pop_back();
    std::vector<std::string> files, names;
    if (DIR* d = opendir(dir.c_str())) {
        while (struct dirent* e = readdir(d))
            if (std::strcmp(e->d_name, ".") != 0 && std::strcmp(e->d_name, "..") != 0) names.push_back(e->d_name);
        closedir(d);
    }
    std::sort(names.begin(), names.end());
    for (const std::string& n : names) {
        std::vector<std::string> below;
        if (recurse > 0) below = files_in_directory(dir + "/" + n, recurse - 1);
        if (below.empty()) files.push_back(dir + "/" + n);
        else files.insert(files.end(), below.begin(), below.end());
    }
    return files;
}

// The input names of the command line -> the units, in the order they are read.  false (reported): no input, or an odd
// number of files to pair.
static bool make_units(const std::vector<std::string>& named, bool pairfiles, bool pairseq, Options& o) {
    o.units.clear(); o.pairing = Options::NONE;
    auto unit = [&](const std::string& a, const std::string& b, bool inter) { ReadUnit u; u.f1 = a; u.f2 = b; u.interleaved = inter; o.units.push_back(u); };
    bool expanded = false;
    std::vector<std::string> files;
    for (const std::string& n : named) {
        if (n == "-" && named.size() == 2 && &n == &named[1]) continue;                 // `r1 -`
        const std::vector<std::string> in = files_in_directory(n);
        if (in.empty()) files.push_back(n); else { files.insert(files.end(), in.begin(), in.end()); expanded = true; }
    }
    if (files.empty()) { std::fprintf(stderr, "ABORT: no read files given\n"); return false; }
    pairseq = pairseq && !pairfiles;                                                    // -pairfiles comes first: src/query_options.cpp:83-97
    const bool two_named = named.size() == 2 && files.size() == 2 && !expanded && !pairseq;   // `r1 r2`: one pair, in the given order
    if ((pairfiles && files.size() > 1) || two_named) {
        o.pairing = Options::FILES;
        if (!two_named) std::sort(files.begin(), files.end());                          // src/mode_query.cpp:409-411
        if (files.size() & 1) { std::fprintf(stderr, "ABORT: -pairfiles needs an even number of read files, %zu were given\n", files.size()); return false; }
        for (size_t i = 0; i < files.size(); i += 2) unit(files[i], files[i + 1], false);
    } else if (pairseq) {
        o.pairing = Options::SEQUENCES;
        for (const std::string& f : files) unit(f, "", true);
    } else
        for (const std::string& f : files) unit(f, "", false);
    return true;
}

// -help of mcq_query_cli and mcq_query_mpi
static const char* const kQueryUsage =
    "usage: mcq_query_cli <dbprefix> <n_ranks> <file|directory>... [-pairfiles | -pairseq] [-splitout PREFIX] [options]\n"
    "       mcq_query_cli <dbprefix> <n_ranks> <r1> <r2|-> [options]\n"
    "       mpiexec -n N mcq_query_mpi <dbprefix> <n_ranks> <file|directory>... [options] [-transport rccl|mpi]\n"
    "classification:  -lowest R  -highest R  -maxcand N  -hitmin N  -hitdiff X  -insertsize N  -noquirks\n"
    "output:          -out FILE  -splitout PREFIX  -tophits  -taxids  -taxids-only  -omit-ranks  -lineage  -mapped-only  -nomap\n"
    "                 -abundances [FILE]  -abundance-per R  -list-inputs\n"
    "running:         -threads N  -batch N  -batch-bases N  -read-chunk BYTES  -reader gpu|host\n"
    "evaluation (mcq_query_cli only; mcq_query_mpi rejects these three and names mcq_query_cli):\n"
    "  -exclude RANK    clade exclusion: a read whose header names its ground truth (accession, or taxid|N) loses every\n"
    "                   database hit on the truth's clade at RANK before its candidates are made; a truth without an\n"
    "                   ancestor at RANK loses the hits on targets that have none either\n"
    "  -ground-truth    (-ground_truth, -groundtruth) a truth_ column in front of the classification\n"
    "  -precision       known / correct / precision / sensitivity per rank in the summary\n"
    "                   The truth is resolved against the whole database and kept up to the evaluation (the reference's\n"
    "                   MPI program resolves it per shard and evaluates without it).\n"
    "where the reads land:\n"
    "  -hits-per-seq [FILE]  (mcq_query_cli only; mcq_query_mpi rejects it and names mcq_query_cli; aliases -hitsperseq, -hits_per_seq,\n"
    "                   -hits-per-sequence, ...) after the mapping lines, or into FILE: for every reference sequence that is a\n"
    "                   candidate of some read the reads that hit it, as queryid/window:hits/window:hits...; a query_id column in\n"
    "                   front of every mapping line.  Rows in ascending target order.  Host memory grows with the input (one\n"
    "                   entry per read and candidate is kept until the end, as in the reference).  A read with more than %u\n"
    "                   distinct (sequence, window) pairs on its candidates ends the run with an ABORT line that names it.\n"
    "coverage (mcq_query_cli only; mcq_query_mpi rejects both and names mcq_query_cli; not options of the reference):\n"
    "  -coverage [FILE]  after the mapping lines and the -hits-per-seq table, in front of the abundance tables, or into FILE: for every\n"
    "                   reference sequence that is a candidate of some read its windows, the windows hit by at least one read, that\n"
    "                   fraction, the reads that had it as a candidate and their hits -- added up on the GPU, nothing per read is kept.\n"
    "                   Candidates are taken at sequence level whatever -lowest says (up to 16 per read).  A read beyond the\n"
    "                   capacity of -hits-per-seq adds nothing and is counted in a # line of the report.  With -splitout the coverage\n"
    "                   is taken over all units together and written once: into FILE, else to stdout behind the last unit's run.\n"
    "  -cov-percentile P  (0..100) two passes over the input: the first only gathers the coverage; then the floor(H * P / 100) of the\n"
    "                   H hit sequences with the least fraction of windows covered (ties: the lower target id first) are removed,\n"
    "                   and the second pass is the ordinary run in which a removed sequence can be no candidate of any read.  The\n"
    "                   last column of the -coverage report shows the cut.  Not together with -exclude.\n"
    "alignment:\n"
    "  -align           (mcq_query_cli only; mcq_query_mpi rejects it and names mcq_query_cli; aliases -alignment, -showalignment) with\n"
    "                   -lowest sequence: behind the line of a read classified to a sequence, its semi-global alignment to the top\n"
    "                   candidate's window range (score, source file and record, range, the two aligned strings), computed on the GPU.\n"
    "                   A mate of more than 2048 bases or a window range of more than 4096 bases ends the run with an ABORT line\n"
    "                   that names the read.  The genome files the database names are read once at the start, relative to the\n"
    "                   working directory, and stay in host memory: it grows with the genomes.  A file that cannot be read is\n"
    "                   reported once and its sequences get no alignment.  Above -lowest sequence only the parameter line is written.\n"
    "  -align-candidate-range  (written into no output) with n_ranks > 1 the merged candidates carry no positions and -align aligns\n"
    "                   to window 0 of the target, as the reference's MPI program does; this option aligns to the candidate's real\n"
    "                   window range instead\n"
    "more columns:\n"
    "  -queryids        (aliases -query-ids, -query_ids, -queryid, -query-id, -query_id) a query_id column in front of every mapping\n"
    "                   line: the 1-based number of the read (pair)\n"
    "  -locations       a candidate_locations column behind top_hits: `[begin,end] ` in bases of the target for every candidate; with\n"
    "                   n_ranks > 1 the merged candidates carry no positions and every entry is `[0,<window length>] `\n"
    "  -allhits         (mcq_query_cli only; mcq_query_mpi rejects it and names mcq_query_cli; alias -all-hits) an all_hits column in\n"
    "                   front of top_hits: every (sequence, window) the read hits with its number of hits, as name/window:hits, with\n"
    "                   -lowest sequence, else as ancestorname:hits, -- computed on the GPU.  Every read is shown (also with -nomap or\n"
    "                   -mapped-only, unless -nomap -tophits).  With -exclude RANK the hits on the read's own clade are left out.  A\n"
    "                   batch whose hits need more than 2 GiB, or a read with more locations than the workspace takes, ends the run\n"
    "                   with an ABORT line.  Three batches are in flight: up to 6 GiB on the device and 6 GiB of pinned host memory.\n"
    "database query options (both programs; get_database_query_options of the reference; written into no output line):\n"
    "  -winlen N  -winstride N  -sketchlen N   sketch the READS with another window length, window stride or sketch size than the\n"
    "                   database was built with.  -winlen without -winstride sets the stride to N as well; values below 1 are ignored.\n"
    "                   The engine's limits: a window of k to 128 bases, a sketch of at most 32 features; a value outside them ends\n"
    "                   the run with an ABORT line before the database is read.\n"
    "  -max-locations-per-feature N  (-max_locations_per_feature) shrink every bucket -- the locations of one feature on one rank of\n"
    "                   the build -- to its first N locations, on the GPU while the shard files are streamed.  As in the reference: N\n"
    "                   of 1 or less is ignored without the next option; N is taken as an 8-bit bucket size (300 means 44, 256\n"
    "                   means 1); 254 and 255 mean the largest bucket and change nothing; so does an N at or above the database's\n"
    "                   own limit.\n"
    "  -remove-overpopulated-features  (-remove_overpopulated_features) drop every feature of a rank whose bucket there holds more\n"
    "                   than N - 1 locations (253 without N or with N of 254 and more; at most the database's limit - 1; not applied\n"
    "                   when that is 0), then shrink to N as above: N = 1 removes nothing and leaves one location per bucket.\n"
    "                   Either of the two loads the database by the streaming route whatever its size; the numbers of buckets shrunk\n"
    "                   and removed are printed on stderr.\n"
    "  -max-load-fac X  is not read: it sizes the reference's hash table and changes no result.\n"
    "rejected:        -taxon-coverage (both programs): the coverage statistics are not reproduced\n";

static bool parse_options(int argc, char** argv, Options& o) {
    for (int a = 1; a < argc; ++a) if (std::string(argv[a]) == "-help" || std::string(argv[a]) == "--help" || std::string(argv[a]) == "-h") { std::printf(kQueryUsage, (unsigned)MCQ_TARGET_HITS_MAX_KEYS); return false; }   // (the text's one %u: the kernel's key capacity)
    std::vector<std::string> named;                      // argv[3 ..] up to the first option
    int i = 3;
    for (; i < argc && !(argv[i][0] == '-' && argv[i][1] != '\0'); ++i) named.push_back(argv[i]);
    if (argc < 4 || named.empty()) {
        std::fprintf(stderr, "usage: %s <dbprefix> <n_ranks> <file|directory>... [-pairfiles | -pairseq] [-splitout PREFIX] [options]\n"
                             "       %s <dbprefix> <n_ranks> <r1> <r2|-> [options]\n", argv[0], argv[0]);
        return false;
    }
    o.prefix = argv[1]; o.P = (uint32_t)std::atoi(argv[2]);
    bool pairfiles = false, pairseq = false; std::string split_prefix;
    for (; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() -> const char* { return (i + 1 < argc) ? argv[++i] : ""; };
        if (a == "-lowest") { uint32_t r = mcq_rank_from_name(next()); if (r < MCQ_RANK_ROOT) o.lowest = r; }
        else if (a == "-highest") { uint32_t r = mcq_rank_from_name(next()); if (r <= MCQ_RANK_ROOT) o.highest = r; }
        else if (a == "-maxcand" || a == "-max-cand") o.maxcand = (uint32_t)std::atoi(next());
        else if (a == "-hitmin") o.hitmin = (uint32_t)std::atoi(next());
        else if (a == "-hitdiff") { o.hitdiff = (float)std::atof(next()); if (o.hitdiff > 1) o.hitdiff *= 0.01; }   // src/query_options.cpp:167-169
        else if (a == "-insertsize") o.insertsize = std::strtoull(next(), nullptr, 10);
        else if (a == "-threads") o.threads = (uint32_t)std::atoi(next());
        else if (a == "-tophits" || a == "-top-hits") o.tophits = true;
        else if (a == "-taxids" || a == "-taxid") o.taxids = true;
        else if (a == "-taxids-only" || a == "-taxidsonly" || a == "-taxid-only") o.taxids_only = true;
        else if (a == "-omit-ranks" || a == "-omitranks") o.show_ranks = false;
        else if (a == "-lineage") o.lineage = true;
        else if (a == "-mapped-only" || a == "-mappedonly") o.mapped_only = true;
        else if (a == "-nomap" || a == "-no-map") o.nomap = true;
        else if (a == "-noquirks") o.quirks = false;
        else if (opt_named(a, {"-paired_files", "-paired-files", "-pair_files", "-pair-files", "-pairfiles"})) pairfiles = true;   // src/query_options.cpp:83-84
        else if (opt_named(a, {"-paired_sequences", "-paired-sequences", "-pair_sequences", "-pair-sequences", "-pair_sequ", "-pair-sequ",
                               "-pair_seq", "-pair-seq", "-pairsequ", "-pairseq", "-paired"})) pairseq = true;                      // :90-94
        else if (a == "-list-inputs") o.list_inputs = true;
        else if (a == "-splitout" || a == "-split-out") { o.split = true; if (i + 1 < argc && argv[i + 1][0] != '-') split_prefix = argv[++i]; }
        else if (a == "-transport") o.transport = next();
        else if (a == "-batch") o.batch = std::max<uint64_t>(1, std::strtoull(next(), nullptr, 10));
        else if (a == "-batch-bases") o.batch_bases = std::max<uint64_t>(1024, std::strtoull(next(), nullptr, 10));
        else if (a == "-out") o.outfile = next();
        else if (a == "-read-chunk") o.read_chunk = std::max<uint64_t>(1, std::strtoull(next(), nullptr, 10));
        else if (a == "-reader") o.host_reader = std::string(next()) == "host";
        else if (a == "-abundances") {                                       // the FILE is the next token unless it is an option
            o.abundances = true;
            if (i + 1 < argc && argv[i + 1][0] != '-') o.abundance_file = argv[++i];
        }
        else if (a == "-abundance-per" || a == "-abundances-per" || a == "-abundance_per" || a == "-abundances_per") {
            const uint32_t r = mcq_rank_from_name(next()); if (r < MCQ_RANK_ROOT) o.abundance_rank = r;
        }
        else if (opt_named(a, {"-hits-per-seq", "-hitsperseq", "-hits_per_seq", "-hits-per-sequence", "-hitspersequence", "-hits_per_sequence"})) {   // src/query_options.cpp:299-306
            o.hits_per_seq = true; o.query_ids = true;                       // src/query_options.cpp:308
            if (i + 1 < argc && argv[i + 1][0] != '-') o.hits_file = argv[++i];
        }
        else if (a == "-coverage") {                                         // the FILE is the next token unless it is an option
            o.coverage = true;
            if (i + 1 < argc && argv[i + 1][0] != '-') o.coverage_file = argv[++i];
        }
        else if (a == "-cov-percentile" || a == "-cov_percentile") {
            char* end = nullptr; const char* v = next();
            const double P = std::strtod(v, &end);
            if (end == v || *end != '\0' || !(P >= 0.0 && P <= 100.0)) {
                std::fprintf(stderr, "ABORT: -cov-percentile takes a number from 0 to 100, not '%s'\n", v);
                return false;
            }
            o.cov_percentile = P;
        }
        else if (opt_named(a, {"-align", "-alignment", "-showalignment"})) o.align = true;                                      // src/query_options.cpp:329-331
        else if (a == "-align-candidate-range") o.align_range = true;
        else if (opt_named(a, {"-queryids", "-query-ids", "-query_ids", "-queryid", "-query-id", "-query_id"})) o.query_ids = true;   // src/query_options.cpp:249-250
        else if (a == "-locations") o.locations = true;                                                                         // :257
        else if (a == "-allhits" || a == "-all-hits") o.allhits = true;                                                         // :262-263
        else if (a == "-exclude") { const uint32_t r = mcq_rank_from_name(next()); if (r < MCQ_RANK_ROOT) o.exclude_rank = r; }   // src/query_options.cpp:205-210
        else if (opt_named(a, {"-ground-truth", "-ground_truth", "-groundtruth"})) o.ground_truth = true;                       // :196-198
        else if (a == "-precision") o.precision = true;                                                                         // :203
        else if (a == "-max-locations-per-feature" || a == "-max_locations_per_feature") o.tuning.max_locs = std::atoi(next());   // src/query_options.cpp:47-49
        else if (a == "-remove-overpopulated-features" || a == "-remove_overpopulated_features") o.tuning.remove_overpopulated = true;   // :51-53
        else if (a == "-sketchlen") o.tuning.sketchlen = std::atoi(next());                                                     // :56
        else if (a == "-winlen") o.tuning.winlen = std::atoi(next());                                                           // :57
        else if (a == "-winstride") o.tuning.winstride = std::max(0, std::atoi(next()));                                        // :58 (given: -winlen does not set it; below 1: not applied)
        else if (a == "-taxon-coverage") {                                                                                      // :201
            std::fprintf(stderr, "ABORT: -taxon-coverage is not supported: the coverage statistics (a scan over all taxa per read) are not reproduced; "
                                 "-precision alone gives the other statistics\n");
            return false;
        }
    }
    if (o.split && o.outfile.empty()) o.outfile = split_prefix;              // src/query_options.cpp:346-351
    if (o.abundance_file == o.outfile) o.abundance_file.clear();
    if (o.cov_cut() && o.exclude_rank != MCQ_RANK_NONE) {                   // (both need the workspace's one exclusion table)
        std::fprintf(stderr, "ABORT: -cov-percentile and -exclude cannot be combined: both use the one exclusion table of the workspace\n");
        return false;
    }
    if (o.coverage_file == o.outfile) o.coverage_file.clear();
    if (o.hits_file == o.outfile) o.hits_file.clear();                       // src/query_options.cpp:353
    if (!make_units(named, pairfiles, pairseq, o)) return false;
    if (o.lowest > o.highest) o.lowest = o.highest;
    if (o.nomap && o.tophits) { o.nomap = false; o.mapped_only = true; }   // "showing hits changes the mapping mode", src/query_options.cpp:293-297
    else if (o.allhits) { o.nomap = false; o.mapped_only = false; }        // ... -allhits shows every read
    return true;
}

struct Out {
    mcq_refdb* db; const Options& p; Mode mode;
    const char* comment = "# "; const char* none = "--"; const char* col = "\t|\t";
    uint64_t tgt_stride = 0, tgt_winlen = 0;             // -locations: the database's target window stride and window size

    // one taxon column entry: [prefix ':'] body, the body built from a name text and an id text
    template <class Name, class Id>
    void entry(std::ostream& os, const char* prefix, const Name& name, const Id& id) const {
        if (mode.rank_prefix) os << prefix << ':';
        if (mode.body != 1) os << name;
        if (mode.body == 2) os << '(';
        if (mode.body != 0) os << id;
        if (mode.body == 2) os << ')';
    }
    void taxon(std::ostream& os, uint32_t key) const {
        entry(os, mcq_rank_name(mcq_refdb_taxon_rank(db, key)), mcq_refdb_taxon_name(db, key), mcq_refdb_taxon_id(db, key));
    }
    void no_taxon(std::ostream& os, uint32_t rank) const { entry(os, mcq_rank_name(rank), none, 0); }
    // classification column: show_taxon(os, db, opt, tax), src/printing.cpp:305-330 (collapseUnclassified is on)
    void best(std::ostream& os, uint32_t key) const {
        if (key == MCQ_NO_TAXON || mcq_refdb_taxon_rank(db, key) > p.highest) {
            if (mode.ids_only() && !mode.rank_prefix) os << 0; else os << none;
            return;
        }
        const uint32_t tr = mcq_refdb_taxon_rank(db, key);
        const uint32_t rmin = p.lowest < tr ? tr : p.lowest, rmax = p.lineage ? p.highest : rmin;
        for (uint32_t r = rmin; r <= rmax; ++r) {                           // show_lineage, src/printing.cpp:181-201
            const uint32_t a = mcq_refdb_ancestor(db, key, r);
            if (a != MCQ_NO_TAXON) taxon(os, a); else no_taxon(os, r);
            if (r < rmax) os << ',';
        }
    }
    // the TABLE_LAYOUT line's taxon column: one entry per rank shown, every word behind `pre` (show_taxon_header, src/printing.cpp:240-300)
    void header_taxon(std::ostream& os, const std::string& pre = "") const {
        const uint32_t rmax = p.lineage ? p.highest : p.lowest;
        for (uint32_t r = p.lowest; r <= rmax; ++r) {
            entry(os, (pre + (p.lowest == rmax ? "rank" : mcq_rank_name(r))).c_str(), pre + "taxname", pre + "taxid");
            if (r < rmax) os << ',';
        }
    }
};

static Out make_out(mcq_refdb* rdb, const Options& p) {
    Out o{rdb, p, Mode::make(p.show_ranks, p.taxids, p.taxids_only)};   // -taxids-only wins over -taxids (src/query_options.cpp:262-274)
    mcq_refdb_info info; mcq_refdb_get_info(rdb, &info);
    o.tgt_stride = info.winstride; o.tgt_winlen = info.winlen;
    return o;
}

// show_query_parameters (src/printing.cpp:40-113) + show_query_mapping_header (src/classification.cpp:486-512)
static void write_head(std::ostream& os, const Out& o, uint32_t hitmin, bool layout = true) {   // layout false: the head of a merge, which prints no TABLE_LAYOUT line
    const Options& p = o.p; const char* cm = o.comment;
    if (!p.nomap) {
        os << cm << "Reporting per-read mappings (non-mapping lines start with '" << cm << "').\n";
        if (p.lineage) os << cm << "The complete lineage will be reported starting with the lowest match.\n";
        else os << cm << "Only the lowest matching rank will be reported.\n";
    } else os << cm << "Per-Read mappings will not be shown.\n";
    os << cm << "Classification will be constrained to ranks from '" << mcq_rank_name(p.lowest) << "' to '" << mcq_rank_name(p.highest) << "'.\n";
    os << cm << "Classification hit threshold is " << hitmin << " per query\n";
    os << cm << "At maximum " << p.maxcand << " classification candidates will be considered per query.\n";
    if (p.exclude_rank != MCQ_RANK_NONE) os << cm << "Clade Exclusion on Rank: " << mcq_rank_name(p.exclude_rank);   // (no newline: src/printing.cpp:75-78)
    if (p.pairing == Options::FILES) os << cm << "File based paired-end mode:\n" << cm << "  Reads from two consecutive files will be interleaved.\n"
                                        << cm << "  Max insert size considered " << p.insertsize << ".\n";
    else if (p.pairing == Options::SEQUENCES) os << cm << "Per file paired-end mode:\n" << cm << "  Reads from two consecutive sequences in each file will be paired up.\n"
                                                 << cm << "  Max insert size considered " << p.insertsize << ".\n";
    if (p.align) os << cm << "Query sequences will be aligned to best candidate target => SLOW!\n";   // src/printing.cpp:91-93
    if (p.hits_per_seq)                                                     // (both lines hang on -hits-per-seq in the reference: the second one is its quirk, :95-103)
        os << cm << "A list of hits per reference sequence will be generated after the read mapping.\n"
           << cm << "A list of absolute and relative abundances per taxon will be generated after the read mapping.\n";
    if (p.coverage) os << cm << "A list of window coverage per reference sequence will be generated after the read mapping.\n";
    if (p.cov_cut()) os << cm << "Reference sequences below coverage percentile " << p.cov_percentile << " were removed before the read mapping.\n";
    if (p.abundance_rank != MCQ_RANK_NONE)
        os << cm << "A list of absolute and relative abundances for each '" << mcq_rank_name(p.abundance_rank)
           << "' will be generated after the read mapping.\n";
    os << cm << "Using " << p.threads << " threads\n";
    if (!p.nomap && layout) {
        os << cm << "TABLE_LAYOUT: ";
        if (p.query_ids) os << "query_id" << o.col;                          // showQueryIds, src/query_options.cpp:308, src/classification.cpp:495
        os << "query_header" << o.col;
        if (p.ground_truth) { o.header_taxon(os, "truth_"); os << o.col; }
        if (p.allhits) os << "all_hits" << o.col;                            // src/classification.cpp:504-506
        if (p.tophits) os << "top_hits" << o.col;
        if (p.locations) os << "candidate_locations" << o.col;
        o.header_taxon(os);
        os << '\n';
    }
}
// the line in front of a unit's mapping lines (showInfo, src/querying.h:1336-1340)
static void write_unit_line(std::ostream& os, const Out& o, const ReadUnit& u) { os << o.comment << u.display() << '\n'; }

// -splitout: the options of the run over `u` alone, its outputs named as src/mode_query.cpp:176-228 names them
static std::string extract_filename(const std::string& path) { return path.substr(path.find_last_of("/\\") + 1); }   // src/filesys_utility.cpp:94-101
static Options split_options(const Options& p, const ReadUnit& u) {
    Options s = p;
    s.units.assign(1, u); s.split = false;
    const std::string tail = "_" + extract_filename(u.f1) + (u.f2.empty() ? std::string() : "_" + extract_filename(u.f2)) + ".txt";
    if (!p.outfile.empty()) s.outfile = p.outfile + tail;
    if (!p.abundance_file.empty()) s.abundance_file = p.abundance_file + tail;
    if (!p.hits_file.empty()) s.hits_file = p.hits_file + tail;             // src/mode_query.cpp:186-190, :213-218
    s.coverage = false; s.coverage_file.clear();                            // (the report is written once, over all units together: mcq_query_cli's main)
    return s;
}
// -list-inputs
static void list_inputs(std::ostream& os, const Options& p) {
    static const char* mode[] = {"none", "files", "sequences"};
    os << "pairing: " << mode[p.pairing] << '\n';
    for (const ReadUnit& u : p.units) {
        os << u.display();
        if (p.split) os << '\t' << split_options(p, u).outfile;
        os << '\n';
    }
}
// every file of every unit opens: asked before the first output is written, whichever run reads the file
static bool inputs_readable(const Options& p) {
    for (const ReadUnit& u : p.units)
        for (const std::string* f : {&u.f1, &u.f2})
            if (!f->empty() && !std::ifstream(*f).good()) { std::fprintf(stderr, "FAIL: can't open file %s\n", f->c_str()); return false; }
    return true;
}
// the runs a command line asks for: one over all units, or (-splitout) one per unit
static std::vector<Options> output_runs(const Options& p) {
    std::vector<Options> runs;
    if (!p.split) runs.push_back(p);
    else for (const ReadUnit& u : p.units) runs.push_back(split_options(p, u));
    return runs;
}

// one query: classification (src/classification.cpp:235-265), statistics (classification_statistics::assign,
// src/classification_statistics.h:69-78) and its mapping line (show_query_mapping, src/classification.cpp:583-632)
// (token: the header up to its first ' ', what the line prints; truth: the read's ground truth or MCQ_NO_TAXON, for the truth_
//  column and, with `ev`, evaluate_classification's assign_known_correct, src/classification.cpp:329-353)
// -align: what show_alignment (src/classification.cpp:437-477) prints of a read, or nothing (length 0)
// -allhits: a read's entries (mcq_all_hits) and what turns them into the column.  tgt_key[t]: the taxon whose name stands for target t
// (its ancestor at -lowest, or the sequence itself: mcq_refdb_tgt2tax).  tgt_clade / query_clade (-exclude): an entry on a target
// whose clade key is the read's is left out, as remove_hits_on_rank drops its matches (src/classification.cpp:141-157)
struct AllHits {
    const mcq_hit* e = nullptr; uint32_t n = 0;
    const uint32_t* tgt_key = nullptr;
    const uint32_t* tgt_clade = nullptr; uint32_t query_clade = 0;
};
// show_matches over match locations, src/printing.cpp:365-416
static void write_all_hits(std::ostream& os, const Out& o, const AllHits& h) {
    const bool seq = o.p.lowest == MCQ_RANK_SEQUENCE;
    for (uint32_t i = 0; i < h.n; ++i) {
        const mcq_hit& m = h.e[i];
        if (h.tgt_clade && h.tgt_clade[m.tgt] == h.query_clade) continue;
        os << mcq_refdb_taxon_name(o.db, h.tgt_key[m.tgt]);
        if (seq) os << '/' << (int)m.win;
        os << ':' << (int)m.hits << ',';
    }
}
struct AlignBlock {
    int32_t score = 0; uint32_t length = 0;              // length: of the two aligned strings; 0 = no block
    const char* file = ""; uint64_t index = 0;           // the target's source
    uint64_t range_beg = 0, range_end = 0;               // w * beg, w * end + w
    const char* query = nullptr; const char* target = nullptr;
};
static void write_query(std::ostream& os, const Out& o, uint32_t hitmin, const char* token, size_t token_len,
                        const mcq_cand* cands, uint32_t ncand, uint64_t* assigned /* [MCQ_RANK_NONE + 1] */,
                        uint32_t truth = MCQ_NO_TAXON, mcq_eval_stats* ev = nullptr, uint64_t query_id = 0, const AlignBlock* al = nullptr,
                        const AllHits* all = nullptr) {
    mcq_refdb* rdb = o.db; const Options& p = o.p;
    const uint32_t best = mcq_refdb_classify(rdb, reinterpret_cast<const uint32_t*>(cands), ncand, hitmin, p.hitdiff, p.highest);
    if (best == MCQ_NO_TAXON) ++assigned[MCQ_RANK_NONE];
    else for (uint32_t r = mcq_refdb_taxon_rank(rdb, best); r <= MCQ_RANK_ROOT; ++r) ++assigned[r];
    if (ev) mcq_eval_stats_assign_known_correct(ev, mcq_refdb_taxon_rank(rdb, best), mcq_refdb_taxon_rank(rdb, truth),
                                                mcq_refdb_taxon_rank(rdb, mcq_refdb_ranked_lca(rdb, best, truth)));
    if (p.nomap || (p.mapped_only && best == MCQ_NO_TAXON)) return;
    if (p.query_ids) os << query_id << o.col;                                // showQueryIds, src/classification.cpp:537
    os.write(token, (std::streamsize)token_len) << o.col;
    if (p.ground_truth) { o.best(os, truth); os << o.col; }                  // show_taxon(os, db, opt, query.groundTruth), :611-614
    if (p.allhits) { if (all) write_all_hits(os, o, *all); os << o.col; }    // src/classification.cpp:555-558
    if (p.tophits) {                                                         // show_matches, src/printing.cpp:333-360
        for (uint32_t i = 0; i < ncand && cands[i].hits > 0; ++i) {
            const mcq_cand& c = cands[i];
            if (i) os << ',';
            const uint32_t key = c.tax;
            if (p.lowest == MCQ_RANK_SEQUENCE) os << mcq_refdb_taxon_name(rdb, key);
            else {
                const uint32_t a = mcq_refdb_taxon_rank(rdb, key) < p.lowest ? mcq_refdb_ancestor(rdb, key, p.lowest) : key;
                if (a != MCQ_NO_TAXON) os << mcq_refdb_taxon_id(rdb, a); else os << mcq_refdb_taxon_name(rdb, key);
            }
            os << ':' << c.hits;
        }
        os << o.col;
    }
    if (p.locations) {                                                       // show_candidate_ranges, src/printing.cpp:422-432
        for (uint32_t i = 0; i < ncand && cands[i].hits > 0; ++i)
            os << '[' << o.tgt_stride * cands[i].win_beg << ',' << o.tgt_stride * cands[i].win_end + o.tgt_winlen << "] ";
        os << o.col;
    }
    o.best(os, best);
    if (al && al->length && best != MCQ_NO_TAXON) {                          // opt.showAlignment && cls.best, src/classification.cpp:627-629
        os << '\n' << o.comment << "  score  " << al->score << "  aligned to " << al->file << " #" << al->index
           << " in range [" << al->range_beg << ',' << al->range_end << "]\n" << o.comment << "  query  ";
        os.write(al->query, al->length) << '\n' << o.comment << "  target ";
        os.write(al->target, al->length);
    }
    os << '\n';
}
static void write_query(std::ostream& os, const Out& o, uint32_t hitmin, const std::string& header,
                        const mcq_cand* cands, uint32_t ncand, uint64_t* assigned, uint64_t query_id = 0) {
    write_query(os, o, hitmin, header.data(), std::min(header.size(), header.find(' ')), cands, ncand, assigned, MCQ_NO_TAXON, nullptr, query_id);
}

// show_summary (src/printing.cpp:622-641) + show_taxon_statistics (:522-555)
static void write_summary(std::ostream& os, const Out& o, const uint64_t* assigned, double ms, const mcq_eval_stats* ev = nullptr) {
    const Options& p = o.p; const char* cm = o.comment;
    const uint64_t total = assigned[MCQ_RANK_ROOT] + assigned[MCQ_RANK_NONE];
    const uint64_t num_queries = p.paired() ? 2 * total : total;             // paired reads count twice (:626-627)
    os << cm << "queries: " << num_queries << '\n'
       << cm << "time:    " << (long long)ms << " ms\n"
       << cm << "speed:   " << num_queries / (ms / 60000.0) << " queries/min\n";
    if (total > 0) {
        mcq_eval_stats st; std::memset(&st, 0, sizeof(st));                  // without -precision: the assignments alone
        if (ev) st = *ev; else std::copy(assigned, assigned + MCQ_RANK_NONE + 1, st.assigned);
        std::string text((size_t)mcq_eval_stats_text(&st, cm, nullptr, 0) + 1, '\0');
        mcq_eval_stats_text(&st, cm, &text[0], text.size());
        text.pop_back();
        os << text;
    } else std::cerr << cm << "No valid query sequences found.\n";
}

// the taxonomy of the database on `device` for mcq_classify (the ranked lineages mcq_refdb_classify works on)
static mcq_taxonomy* make_taxonomy(mcq_refdb* rdb, int device) {
    mcq_refdb_info info; mcq_refdb_get_info(rdb, &info);
    std::vector<uint32_t> lin((size_t)info.n_taxa * 21); std::vector<uint8_t> rank(info.n_taxa);
    mcq_taxonomy* tx = nullptr;
    if (mcq_refdb_lineages(rdb, lin.data(), rank.data())) { std::fprintf(stderr, "ABORT: %s\n", mcq_host_last_error()); return nullptr; }
    if (mcq_taxonomy_create(lin.data(), rank.data(), info.n_taxa, device, &tx)) { std::fprintf(stderr, "ABORT: %s\n", mcq_last_error()); return nullptr; }
    return tx;
}
static mcq_query_opts query_opts(const Options& p) {
    mcq_query_opts qo; qo.max_cand = p.maxcand; qo.emulate_ranks = p.P; qo.insert_size_max = p.insertsize; qo.flags = p.quirks ? MCQ_QUIRK_SEQ_DROP : 0;
    return qo;
}
static mcq_classify_opts classify_opts(const Options& p, uint32_t hitmin) {
    mcq_classify_opts co; co.hits_min = hitmin; co.hits_diff_fraction = p.hitdiff; co.highest_rank = p.highest; co.flags = 0;
    return co;
}

// where the mapping lines go: the -out file (`file`, opened here) if one was named, else stdout
static std::ostream& open_out(const Options& p, std::ofstream& file) {
    if (!p.outfile.empty()) file.open(p.outfile);
    return p.outfile.empty() ? std::cout : file;
}

// counts += the per-taxon counts that ws has gathered since it was made ([n_taxa + 1])
static bool add_taxon_counts(mcq_ws* ws, std::vector<uint64_t>& counts) {
    std::vector<uint64_t> c(counts.size(), 0);
    if (mcq_ws_taxon_counts(ws, c.data(), 0)) { std::fprintf(stderr, "ABORT: %s\n", mcq_last_error()); return false; }
    for (size_t i = 0; i < c.size(); ++i) counts[i] += c[i];
    return true;
}

// the abundance tables (src/classification.cpp:744-757) from the device's counts ([n_taxa + 1], the last slot the unclassified
// queries), after checking them against the host classification's statistics.  They go to the -abundances FILE if one was
// named, else to `os` (the -out file or stdout): src/mode_query.cpp:59-117.  false = mismatch or write error (reported).
static bool write_abundances(std::ostream& os, mcq_refdb* rdb, const Options& p, const std::vector<uint64_t>& counts, const uint64_t* assigned) {
    mcq_refdb_info info; mcq_refdb_get_info(rdb, &info);
    uint64_t classified = 0;
    for (uint32_t t = 0; t < info.n_taxa; ++t) classified += counts[t];
    if (classified != assigned[MCQ_RANK_ROOT] || counts[info.n_taxa] != assigned[MCQ_RANK_NONE]) {
        std::fprintf(stderr, "ABORT: the device classified %llu queries (%llu not), the host %llu (%llu not)\n", (unsigned long long)classified,
                     (unsigned long long)counts[info.n_taxa], (unsigned long long)assigned[MCQ_RANK_ROOT], (unsigned long long)assigned[MCQ_RANK_NONE]);
        return false;
    }
    const uint64_t total = assigned[MCQ_RANK_ROOT] + assigned[MCQ_RANK_NONE];      // statistics.total()
    std::ofstream fab;
    if (!p.abundance_file.empty()) {
        fab.open(p.abundance_file);
        if (!fab.good()) { std::fprintf(stderr, "ABORT: Could not write to file %s\n", p.abundance_file.c_str()); return false; }
        std::cout << "Per-Taxon mappings will be written to file: " << p.abundance_file << std::endl;
    }
    std::ostream& ao = p.abundance_file.empty() ? os : fab;
    auto table = [&](uint32_t rank) -> bool {           // rank MCQ_RANK_NONE: the plain table, else the estimate to it
        const int64_t n = mcq_refdb_abundance_text(rdb, counts.data(), total, rank, nullptr, 0);
        if (n < 0) { std::fprintf(stderr, "ABORT: %s\n", mcq_host_last_error()); return false; }
        std::string text((size_t)n + 1, '\0');
        mcq_refdb_abundance_text(rdb, counts.data(), total, rank, &text[0], text.size());
        text.resize((size_t)n);
        ao << text;
        return true;
    };
    if (p.abundances && !table(MCQ_RANK_NONE)) return false;
    if (p.abundance_rank != MCQ_RANK_NONE && !table(p.abundance_rank)) return false;
    return ao.good();
}

// The reference's shard files -> the queryable handle of shard `shard_id` of `n_shards` (include/mcq_open.hpp: the host-side union
// for small databases, the streaming route -- heads on the host, tables merged on the GPU -- from MCQ_STREAM_LOAD_MIN_MB, default
// 1024, MB of shard files on)
struct Database {
    mcq_refdb* rdb = nullptr; mcq_db* edb = nullptr; std::vector<uint32_t> t2t; uint32_t hitmin = 0;     // hitmin: -hitmin or its default
    mcq_db* seq_edb = nullptr; bool streamed = false;    // -coverage / -cov-percentile above -lowest sequence: the same table with sequence-level keys
    ~Database() { mcq_db_destroy(seq_edb); mcq_db_destroy(edb); mcq_refdb_close(rdb); }
};
static bool open_database(const Options& p, Database& db, uint32_t n_shards, uint32_t shard_id, int device) {
    std::string err; bool& streamed = db.streamed;
    if (mcq_open_refdb(p.prefix, p.P, mcq_stream_load_min_bytes(), &db.rdb, &streamed, err, p.tuning)) { std::fprintf(stderr, "ABORT: %s\n", err.c_str()); return false; }
    mcq_refdb_info info; mcq_refdb_get_info(db.rdb, &info);
    db.hitmin = p.hitmin < 1 ? mcq_default_hits_min(info.sketch_size) : p.hitmin;
    db.t2t.resize(info.n_targets);
    if (mcq_refdb_tgt2tax(db.rdb, p.lowest, db.t2t.data())) { std::fprintf(stderr, "ABORT: %s\n", mcq_host_last_error()); return false; }
    uint64_t n_shrunk = 0, n_removed = 0;
    if (mcq_make_db(db.rdb, streamed, db.t2t.data(), n_shards, shard_id, device, &db.edb, err, p.tuning, &n_shrunk, &n_removed)) { std::fprintf(stderr, "ABORT: %s\n", err.c_str()); return false; }
    if (p.tuning.max_locs > 1 || p.tuning.remove_overpopulated)
        std::fprintf(stderr, "bucket rule: %llu buckets shrunk, %llu removed\n", (unsigned long long)n_shrunk, (unsigned long long)n_removed);
    return true;
}
// the table of an opened database once more, its candidates at sequence level whatever -lowest says (mcq_query_cli's coverage)
static bool open_seq_twin(const Options& p, Database& db) {
    std::string err;
    std::vector<uint32_t> t2t(db.t2t.size());
    if (mcq_refdb_tgt2tax(db.rdb, MCQ_RANK_SEQUENCE, t2t.data())) { std::fprintf(stderr, "ABORT: %s\n", mcq_host_last_error()); return false; }
    if (mcq_make_db(db.rdb, db.streamed, t2t.data(), 1, 0, 0, &db.seq_edb, err, p.tuning)) { std::fprintf(stderr, "ABORT: %s\n", err.c_str()); return false; }
    return true;
}
