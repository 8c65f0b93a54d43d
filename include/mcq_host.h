/* mcq_host.h -- host-side companions of the query engine (C ABI, no GPU needed).
 *
 * Rows f1 and f3 of SURVEY.md section 8: reading the reference's database shard files
 * and the final per-read classification.  Each entry point names the reference code it
 * stands in for (paths relative to the reference root).
 *
 *   mcq_refdb_open      sketch_database::read            src/sketch_database.h:858-952
 *                       hash_multimap::deserialize        src/hash_multimap.h:923-964
 *                       taxon / taxonomy read_binary       src/taxonomy.h:312-335, :660-676
 *   mcq_refdb_tgt2tax   db.ancestor(taxon_of_target, r)   src/sketch_database.h:146, :717-720
 *                       as used by candidates insert()    src/candidates.h:242-245
 *   mcq_refdb_classify  classify()                        src/classification.cpp:235-265
 *                       ranked_lca()                      src/taxonomy.h:531-537
 *   mcq_rank_from_name  taxonomy::rank_from_name          src/taxonomy.h:173-213
 *   mcq_refdb_write_shard  sketch_database::write         src/sketch_database.h:959-998
 *   mcq_refdb_open_meta + mcq_shard_stream_*   the same reader, streaming (no host-side table)
 *   mcq_taxdump_read    make_taxonomic_hierarchy         src/taxonomy_io.cpp:56-185
 *   mcq_target_name / mcq_target_parent_taxid   extract_accession_string / extract_taxon_id   src/sequence_io.cpp:705-748
 *   mcq_genome_files    sequence_filenames               src/args_handling.cpp:50-90, src/filesys_utility.cpp:32-73
 *   mcq_genome_reader_* fasta_reader + add_targets_to_database   src/sequence_io.cpp:121-170, src/mode_build.cpp:559-647
 *   mcq_genome_reader_open_after + mcq_refdb_taxa   the same on a database that was read (`modify`)   src/mode_build.cpp:1117-1136
 *
 * A taxon *key* is the index of the taxon in the database's taxon list; bit 31 marks a
 * sequence-level taxon (rank Sequence), 0xFFFFFFFF is "no taxon".  These are the keys
 * mcq_db_desc.tgt2tax carries and mcq_cand.tax returns.
 */
#ifndef MCQ_HOST_H
#define MCQ_HOST_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct mcq_refdb mcq_refdb;

typedef struct {
    uint32_t k, sketch_size, winlen, winstride;        /* target sketching parameters      */
    uint32_t q_sketch_size, q_winlen, q_winstride;      /* query sketching parameters       */
    uint32_t max_locs_per_feature;
    uint32_t n_ranks;                                    /* shard files read                 */
    uint32_t n_targets, n_taxa;
    uint64_t n_keys, n_locs;                             /* of the union table               */
} mcq_refdb_info;

#define MCQ_NO_TAXON 0xFFFFFFFFu
#define MCQ_RANK_SEQUENCE 0u
#define MCQ_RANK_SPECIES 4u
#define MCQ_RANK_DOMAIN 19u
#define MCQ_RANK_ROOT 20u
#define MCQ_RANK_NONE 21u

/* ---- writing a shard file the reference can read (sketch_database::write src/sketch_database.h:959-998,
 * hash_multimap::serialize src/hash_multimap.h:972-1029, taxon write_binary src/taxonomy.h:326-335) ------
 * One file = one rank: its parameters, the whole taxon list (sequence-level taxa have id -(target+1);
 * `windows` is non-zero only for the targets this rank owns) and this rank's table.  keys / list_off /
 * locs as in mcq_db_desc ((tgt << 32) | win, lists sorted, at most 255 entries each), host memory.
 * Keys are written in the order given (the reference's reader inserts them one by one, any order works). */
typedef struct {
    int64_t id, parent;
    uint8_t rank;               /* MCQ_RANK_* / taxonomy::rank, 21 = none */
    const char* name;
    const char* file;           /* source file name of a sequence-level taxon, "" otherwise */
    uint64_t index;             /* source.index */
    uint64_t windows;           /* source.windows */
} mcq_taxon_rec;
typedef struct {
    uint64_t k, sketch_size, winlen, winstride;         /* target sketcher            */
    uint64_t q_k, q_sketch_size, q_winlen, q_winstride; /* query sketcher             */
    uint64_t max_locs_per_feature;
} mcq_shard_params;
int mcq_refdb_write_shard(const char* path, const mcq_shard_params* params, const mcq_taxon_rec* taxa, uint64_t n_taxa,
                          uint32_t n_targets, const uint32_t* keys, const uint64_t* list_off, const uint64_t* locs,
                          uint64_t n_keys);
/* The same file written in blocks, for a table that is never in host memory as a whole (mcq_build_cli -ranges): open writes the head
 * of mcq_refdb_write_shard and two zero counts; append takes host bytes that hold whole key records (`u32 key, u8 n, u64 n, u32 tgt[n],
 * u64 n, u32 win[n]`, 21 + 8 n bytes each: what mcq_table_shard_records of include/mcq.h makes on the GPU) with their numbers of keys
 * and locations -- n_bytes must be 21 n_keys + 8 n_locs, an empty block is allowed --; close patches the two counts and closes (a
 * null handle is allowed; the handle is gone after close, whatever it returns).  Given the same records in the same order the file
 * is byte-identical to mcq_refdb_write_shard's.  Errors (text: mcq_host_last_error): a file that cannot be opened, a write error.   */
typedef struct mcq_shard_writer mcq_shard_writer;
int mcq_shard_writer_open(const char* path, const mcq_shard_params* params, const mcq_taxon_rec* taxa, uint64_t n_taxa,
                          uint32_t n_targets, mcq_shard_writer** out);
int mcq_shard_writer_append(mcq_shard_writer* w, const void* records, uint64_t n_bytes, uint64_t n_keys, uint64_t n_locs);
int mcq_shard_writer_close(mcq_shard_writer* w);

/* reads <prefix>.db_0 .. <prefix>.db_<n_ranks-1> and unions their tables */
int mcq_refdb_open(const char* prefix, uint32_t n_ranks, mcq_refdb** out);
int mcq_refdb_close(mcq_refdb* db);
int mcq_refdb_get_info(const mcq_refdb* db, mcq_refdb_info* out);

/* ---- the streaming route: shard files of any size (RefSeq scale: >= 1.5e10 locations) without a host-side union ----------
 * mcq_refdb_open_meta reads only the head of every shard file -- parameters, taxa, target count (sketch_database::read up to
 * the feature store, src/sketch_database.h:858-930) -- so that the taxon functions and classify work; info.n_keys stays 0,
 * the table accessors return nothing.  mcq_shard_stream_* hands the key records of one file out in file order as chunks of
 * (feature, target, window) triples (hash_multimap::deserialize, src/hash_multimap.h:923-964: per key {u32 key, u8 n, u64 n,
 * u32 tgt[n], u64 n, u32 win[n]}), whole key records per chunk; mcq_refdb_tgt_windows gives the windows of every target (the
 * taxon `windows` field of its owning rank) -- what turns (target, window) into a global window index.  The consumer is
 * mcq_parts_builder_* of include/mcq.h: the ranks are merged per feature-hash range ON THE GPU.  Host memory: one 16 MB read
 * buffer per open stream + the caller's chunk.                                                                            */
int mcq_refdb_open_meta(const char* prefix, uint32_t n_ranks, mcq_refdb** out);
int mcq_refdb_tgt_windows(const mcq_refdb* db, uint32_t* out /* [n_targets] */);
int mcq_refdb_file_stats(const mcq_refdb* db, uint32_t rank, uint64_t* bytes, uint64_t* n_keys, uint64_t* n_locs);
typedef struct mcq_shard_stream mcq_shard_stream;
int mcq_shard_stream_open(const mcq_refdb* db /* from mcq_refdb_open_meta */, uint32_t rank, mcq_shard_stream** out);
/* up to `cap` (>= 255) locations into feat / tgt / win; *n = 0 when the file is exhausted */
int mcq_shard_stream_next(mcq_shard_stream* s, uint32_t* feat, uint32_t* tgt, uint32_t* win, uint64_t cap, uint64_t* n);
int mcq_shard_stream_close(mcq_shard_stream* s);

/* union table in the layout mcq_db_desc wants; valid until mcq_refdb_close */
const uint32_t* mcq_refdb_keys(const mcq_refdb* db);
const uint64_t* mcq_refdb_list_off(const mcq_refdb* db);
const uint64_t* mcq_refdb_locs(const mcq_refdb* db);

/* taxon key per target for candidate merging below `merge_below_rank` */
int mcq_refdb_tgt2tax(const mcq_refdb* db, uint32_t merge_below_rank, uint32_t* out /* [n_targets] */);

int64_t mcq_refdb_taxon_id(const mcq_refdb* db, uint32_t key);       /* 0 for MCQ_NO_TAXON        */
uint32_t mcq_refdb_taxon_rank(const mcq_refdb* db, uint32_t key);
const char* mcq_refdb_taxon_name(const mcq_refdb* db, uint32_t key);
/* the rest of a taxon record as the shard file holds it (src/taxonomy.h:312-335): parent id, and the source of a sequence-level
 * taxon -- file name, index of the record in that file (from 1), windows (non-zero on the rank that owns the target; the
 * handle keeps the taxa of rank 0's file)                                                                             */
int64_t mcq_refdb_taxon_parent(const mcq_refdb* db, uint32_t key);
const char* mcq_refdb_taxon_file(const mcq_refdb* db, uint32_t key);
uint64_t mcq_refdb_taxon_index(const mcq_refdb* db, uint32_t key);
uint64_t mcq_refdb_taxon_windows(const mcq_refdb* db, uint32_t key);
/* taxon index at `rank` in the ranked lineage of `key`, MCQ_NO_TAXON if none */
uint32_t mcq_refdb_ancestor(const mcq_refdb* db, uint32_t key, uint32_t rank);

/* ---- ground truth and clade exclusion (`-ground-truth`, `-precision`, `-exclude RANK` of the reference's query mode) ----
 * mcq_refdb_ground_truth: the taxon a read's header names, as ground_truth (src/classification.cpp:111-131) resolves it -- the
 * first that succeeds of 1. the sequence-level taxon named by the header's accession.version (extract_ncbi_accession_version_number,
 * src/sequence_io.cpp:600-642), 2. the first one whose name goes on from the header's accession without version
 * (taxon_with_similar_name, src/sketch_database.h:631-639; the two-letter prefixes of src/sequence_io.cpp:43-58), 3. the taxon
 * with the id behind "taxid" + one separator character (:724-748), 4. the sequence-level taxon named by the whole header --
 * and then its next ranked ancestor (src/sketch_database.h:724-737: of a sequence-level taxon the first ranked taxon above
 * it).  Returns the taxon index or MCQ_NO_TAXON.  Resolved against the WHOLE database: the handle holds every target's taxon
 * (each rank of the reference's MPI program asks its own shard).
 * mcq_refdb_clade_keys: per target the key of its ancestor at `rank` -- db.ancestor(hit.tax, rank) of remove_hits_on_rank
 * (src/classification.cpp:141-157) -- or MCQ_CLADE_NONE of include/mcq.h (= MCQ_NO_TAXON) where it has none: what
 * mcq_ws_set_exclusion takes.  mcq_refdb_taxon_clade: the same for a read's truth: its ancestor at `rank`, MCQ_CLADE_NONE if
 * it has none (the truth sits above `rank`), MCQ_CLADE_KEEP_ALL (0xFFFFFFFE) for truth == MCQ_NO_TAXON: one entry of
 * mcq_ws_set_query_clades.                                                                                          */
uint32_t mcq_refdb_ground_truth(const mcq_refdb* db, const char* header, uint64_t len);
int mcq_refdb_clade_keys(const mcq_refdb* db, uint32_t rank, uint32_t* out /* [n_targets] */);
uint32_t mcq_refdb_taxon_clade(const mcq_refdb* db, uint32_t truth, uint32_t rank);
/* mcq_refdb_clade_keys without a database: the keys of targets 0 .. n_targets-1 from the taxon list a build is about to write
 * (mcq_refdb_write_shard: sequence-level taxa, id -(target + 1), then the dump's) -- the values mcq_refdb_clade_keys returns on the
 * written files: index into `taxa` of the ancestor at exactly `rank`, or MCQ_CLADE_NONE.  What mcq_table_remove_ambiguous
 * (include/mcq.h) takes for -remove-ambig-features RANK; for rank sequence the caller passes the target ids themselves.       */
int mcq_taxa_clade_keys(const mcq_taxon_rec* taxa, uint64_t n_taxa, uint32_t n_targets, uint32_t rank, uint32_t* out /* [n_targets] */);

/* ---- evaluation statistics (`-precision`): classification_statistics (src/classification_statistics.h:40-235) restated
 * type for type.  The four arrays are indexed by rank, [MCQ_RANK_NONE] counting the queries without: assigned[r] = queries
 * classified at rank r or below it, known[r] = queries whose truth is known at r or below, correct[r] = of those the ones whose
 * classification is right from r up, wrong[r] = known wrong assignments at r.
 * mcq_eval_stats_assign is assign (:70-78); mcq_eval_stats_assign_known_correct is assign_known_correct (:91-120) with the rank
 * of the classification, of the truth, and of their ranked LCA (mcq_refdb_ranked_lca; MCQ_RANK_NONE where there is none):
 * evaluate_classification (src/classification.cpp:329-353).  The accessors with a rank are known(r), correct(r), wrong(r),
 * assigned(r); the reference's forms without one are the value at MCQ_RANK_ROOT, unknown() / unassigned() the value at
 * MCQ_RANK_NONE, total() = assigned(root) + unassigned().  The rates and precision(r) = correct / (correct + wrong),
 * sensitivity(r) = correct / known are doubles, 0 over an empty denominator (:201-224).
 * mcq_eval_stats_text: show_taxon_statistics (src/printing.cpp:522-600) in ostream default formatting, every line behind
 * `prefix`: the "unclassified" / "classified" block, and once a truth is known the "ground truth ..." blocks.  The coverage
 * block (:601-611, -taxon-coverage) is not reproduced.  Text to buf as mcq_refdb_abundance_text does; returns its length. */
typedef struct { uint64_t assigned[22], known[22], correct[22], wrong[22]; } mcq_eval_stats;
void mcq_eval_stats_assign(mcq_eval_stats* s, uint32_t assigned);
void mcq_eval_stats_assign_known_correct(mcq_eval_stats* s, uint32_t assigned, uint32_t known, uint32_t correct);
void mcq_eval_stats_add(mcq_eval_stats* into, const mcq_eval_stats* from);
uint64_t mcq_eval_stats_total(const mcq_eval_stats* s);
uint64_t mcq_eval_stats_assigned(const mcq_eval_stats* s, uint32_t rank);
uint64_t mcq_eval_stats_known(const mcq_eval_stats* s, uint32_t rank);
uint64_t mcq_eval_stats_unknown(const mcq_eval_stats* s);
uint64_t mcq_eval_stats_correct(const mcq_eval_stats* s, uint32_t rank);
uint64_t mcq_eval_stats_wrong(const mcq_eval_stats* s, uint32_t rank);
double mcq_eval_stats_known_rate(const mcq_eval_stats* s, uint32_t rank);
double mcq_eval_stats_unknown_rate(const mcq_eval_stats* s);
double mcq_eval_stats_classification_rate(const mcq_eval_stats* s, uint32_t rank);
double mcq_eval_stats_unclassified_rate(const mcq_eval_stats* s);
double mcq_eval_stats_precision(const mcq_eval_stats* s, uint32_t rank);
double mcq_eval_stats_sensitivity(const mcq_eval_stats* s, uint32_t rank);
int64_t mcq_eval_stats_text(const mcq_eval_stats* s, const char* prefix, char* buf, size_t cap);
/* ranked_lca (src/taxonomy.h:531-537): the first rank at which both ranked lineages hold the same taxon; MCQ_NO_TAXON if
 * either key is MCQ_NO_TAXON (src/sketch_database.h:751-753) or they share none */
uint32_t mcq_refdb_ranked_lca(const mcq_refdb* db, uint32_t a, uint32_t b);

/* cands: n x {tax key, hits, (2 ignored words)} as mcq_query returns them.
 * hits_diff_fraction as the reference stores it (-hitdiff 80 -> 0.8f).
 * Returns the taxon index of the classification or MCQ_NO_TAXON.                      */
uint32_t mcq_refdb_classify(const mcq_refdb* db, const uint32_t* cands, uint32_t n,
                            uint32_t hits_min, float hits_diff_fraction, uint32_t highest_rank);

/* the ranked lineages classify works on, for the device (mcq_taxonomy_create of include/mcq.h): lineage[t * 21 + r] =
 * taxon index at rank r in the lineage of taxon t (the taxon itself included) or MCQ_NO_TAXON, rank[t] = its rank.
 * lineage holds n_taxa x 21 u32, rank n_taxa bytes.                                                                */
int mcq_refdb_lineages(const mcq_refdb* db, uint32_t* lineage, uint8_t* rank);

/* The reference's abundance tables (show_abundances / show_abundance_estimates, src/printing.cpp:474-517) from the
 * number of classified queries per taxon: counts[n_taxa], indexed by taxon index (bit 31 of the keys stripped);
 * total = queries processed, classified or not (the denominator of the percentages).  est_rank = MCQ_RANK_NONE: the
 * plain table ("# query summary: ..."); a rank below root: estimate_abundance (src/classification.cpp:362-428) to that
 * rank first ("# estimated abundance ...").  The text, its comment line included, goes to buf (NUL-terminated, cut
 * to cap - 1 bytes); returns its length (call with cap = 0 to learn it), negative on error.
 * Counts are exact u64 and become float once, here; the reference adds floats, which differs past 2^24 on one taxon
 * (DESIGN.md section 12).                                                                                          */
int64_t mcq_refdb_abundance_text(const mcq_refdb* db, const uint64_t* counts, uint64_t total, uint32_t est_rank,
                                 char* buf, size_t cap);

/* ---- the table of `-hits-per-seq`: matches_per_target (src/matches_per_target.h:43-188) and show_matches_per_targets
 * (src/printing.cpp:437-469).  For every reference sequence that is a candidate of some read the reads that hit it, and for each
 * read the windows of the read's candidate range on it with a hit count per window.  The ranges and counts come from
 * mcq_target_hits of include/mcq.h; this is the accumulator and the writer.
 * mcq_hits_table_add: one read on one target -- query id, target, the range [win_beg, win_beg + n_win) and counts[n_win].  Windows
 * with a count of 0 are dropped (the reference's vector holds only windows with a match); a range without any is not an entry.
 * mcq_hits_table_merge: matches_per_target::merge -- moves every entry of `from` into `into` (per-thread accumulators).
 * mcq_hits_table_text: sort_match_lists (:172-184: a target's entries by first window, then last window, then query id), then the
 * block of show_matches_per_targets: the three lines behind `comment` and one row per target -- show_taxon of the target (the
 * reference's src/printing.cpp:305-330 with the taxon print mode below), `column`, windows_in_sequence (the `windows` field of the
 * target's taxon on the rank that owns it), `column`, qid/win:hits/win:hits...,qid/...  Text to buf as mcq_refdb_abundance_text
 * does; returns its length (cap = 0: only that), negative on error.
 * ROW ORDER: ascending target id.  The reference iterates an unordered_map keyed by taxon pointers, so its row order is not
 * defined by its inputs; a comparison sorts the rows.
 * mcq_taxon_print: how a taxon is written (taxon_print_mode, src/query_options.h:68-71): show_ranks = the "<rank>:" prefix, body
 * 0 name / 1 id / 2 name(id); lineage != 0: every rank from max(lowest_rank, the taxon's) to highest_rank, else that one rank. */
typedef struct mcq_hits_table mcq_hits_table;
typedef struct { uint32_t show_ranks, body, lineage, lowest_rank, highest_rank; } mcq_taxon_print;
int mcq_hits_table_create(mcq_hits_table** out);
int mcq_hits_table_add(mcq_hits_table* t, uint64_t query_id, uint32_t target, uint32_t win_beg, uint32_t n_win, const uint32_t* counts);
int mcq_hits_table_merge(mcq_hits_table* into, mcq_hits_table* from);
uint64_t mcq_hits_table_targets(const mcq_hits_table* t);
uint64_t mcq_hits_table_entries(const mcq_hits_table* t);
int64_t mcq_hits_table_text(mcq_hits_table* t, const mcq_refdb* db, const char* comment, const char* column,
                            const mcq_taxon_print* mode, char* buf, size_t cap);
/* The same block handed to `sink` piece by piece -- the three head lines, then one piece per row -- so that a table that has grown
 * with the input is formatted once and never held as one text (mcq_query_cli writes it this way; mcq_hits_table_text with its
 * length-first convention formats twice).  sink returns 0 to go on; anything else ends the call with an error.  The lists are
 * sorted once: a later call without an add or merge in between does not sort again.                                        */
typedef int (*mcq_text_sink)(void* user, const char* data, size_t n);
int mcq_hits_table_write(mcq_hits_table* t, const mcq_refdb* db, const char* comment, const char* column,
                         const mcq_taxon_print* mode, mcq_text_sink sink, void* user);
int mcq_hits_table_free(mcq_hits_table* t);
/* the sequence-level taxon key (bit 31 set) of a target, MCQ_NO_TAXON if it has none; and the way back for the device: out[n_taxa],
 * target id of every taxon index that is a target's sequence-level taxon, MCQ_NO_TAXON for the others (mcq_target_slots) */
uint32_t mcq_refdb_target_key(const mcq_refdb* db, uint32_t target);
int mcq_refdb_tax2tgt(const mcq_refdb* db, uint32_t* out /* [n_taxa] */);

/* ---- coverage of reference sequences: the cut of `-cov-percentile` and the report of `-coverage` over what mcq_coverage_read of
 * include/mcq.h returns (cov[n_targets]) and the targets' windows (windows[n_targets]: mcq_refdb_seq_windows, the windows_in_sequence
 * of the -hits-per-seq table as 32-bit numbers).
 * mcq_coverage_cut -- the rule is this project's own: the hit targets are those with windows_covered > 0, H of them.  They are ordered
 * by breadth windows_covered / windows ascending, compared exactly by cross-multiplication in 64 bits (a before b iff a.covered *
 * b.windows < b.covered * a.windows), never as floats; ties go by ascending target id.  The first K = floor(H * percentile / 100) of
 * them get removed[t] = 1, every other target 0.  Percentile 0 removes nothing, 100 removes all hit targets; a target without a covered
 * window is never removed.  percentile outside [0, 100]: an error.
 * mcq_coverage_text / mcq_coverage_write -- the report block as mcq_hits_table_text / mcq_hits_table_write give theirs: behind `comment`
 * the line `--- coverage of reference sequences ---`, one line each for reads_skipped and out_of_range if not 0 (queries that were
 * beyond mcq_target_hits' capacity; ranges mcq_coverage_add refused), and the TABLE_LAYOUT line naming the columns sequence,
 * windows_in_sequence, windows_covered, coverage, queries, hits, kept; then one row per target with queries > 0 in ascending target
 * id: show_taxon of the target under `mode` as in the -hits-per-seq table, windows[t], windows_covered, the fraction with six
 * decimals (0.000000 for a target without windows), queries, hits, and `kept` or `removed` (removed == NULL: all kept).           */
#ifndef MCQ_TARGET_COVERAGE_DEFINED
#define MCQ_TARGET_COVERAGE_DEFINED
typedef struct { uint64_t hits; uint64_t queries; uint32_t windows_covered; uint32_t reserved; } mcq_target_coverage;   /* as in include/mcq.h */
#endif
int mcq_refdb_seq_windows(const mcq_refdb* db, uint32_t* out /* [n_targets] */);
int mcq_coverage_cut(const mcq_target_coverage* cov, const uint32_t* windows, uint32_t n_targets, double percentile, uint8_t* removed /* [n_targets] */);
int64_t mcq_coverage_text(const mcq_refdb* db, const mcq_target_coverage* cov, const uint32_t* windows, uint32_t n_targets,
                          const uint8_t* removed, uint64_t reads_skipped, uint64_t out_of_range, const char* comment, const char* column,
                          const mcq_taxon_print* mode, char* buf, size_t cap);
int mcq_coverage_write(const mcq_refdb* db, const mcq_target_coverage* cov, const uint32_t* windows, uint32_t n_targets,
                       const uint8_t* removed, uint64_t reads_skipped, uint64_t out_of_range, const char* comment, const char* column,
                       const mcq_taxon_print* mode, mcq_text_sink sink, void* user);

/* ---- read files in chunks (mcq_query_cli's input stage) -------------------------------------------------------------
 * mcq_read_stream_fill puts into buf (cap bytes) first the bytes that the last fill left unconsumed, then read()s of the
 * file until buf holds `want` bytes (want <= cap) or the file ends: *len bytes, *eof = 1 when buf[0 .. *len) runs to the end
 * of the file.  mcq_read_stream_consume(s, n) marks the first n bytes of the last fill as used; the rest stays in that
 * buffer, which must stay valid until the next fill moves it to the front of the buffer given then (it may be the same
 * buffer).  Host memory: none besides the caller's buffers.                                                           */
typedef struct mcq_read_stream mcq_read_stream;
int mcq_read_stream_open(const char* path, mcq_read_stream** out);
int mcq_read_stream_fill(mcq_read_stream* s, char* buf, uint64_t cap, uint64_t want, uint64_t* len, int32_t* eof);
int mcq_read_stream_consume(mcq_read_stream* s, uint64_t n_bytes);
int mcq_read_stream_close(mcq_read_stream* s);

/* One chunk of read text per file (text2 NULL: single-end), each starting at a record, parsed exactly as
 * `metacache query` reads it with std::getline (src/sequence_io.cpp:122-285): '@' starts a record of header, sequence,
 * '+' and quality lines; '>' starts a record whose following lines are joined; empty lines are skipped; other lines are
 * appended to the record before them; a '\r' stays in its line.  A record is taken only once it is complete in its chunk
 * (the next record has begun, or the chunk ends the file: flags MCQ_READS_EOF1 / _EOF2).  Records are taken in order while
 * n < max_queries and the bases stay <= max_bases (a first query larger than that is taken alone); with two texts n is at
 * most the smaller complete-record count.  Output, in the form mcq_reads_prepare (include/mcq.h) writes on the device:
 *   bases      the sequences back to back (capacity len1 + len2), mates of query q as sequences 2q, 2q+1
 *   seq_off    [n_seqs + 1] offsets into bases (capacity 2 * max_queries + 1)
 *   hdr        [2 * n] (begin, end) byte range in text1 of query q's header up to its first ' ' (what the -out file prints)
 *   info       [MCQ_READS_INFO_WORDS]: n queries, bases, bytes of text1 / text2 used (the rest is carried to the next
 *              chunk), status (always 0 here), complete records found in text1 / text2 (at most max_queries)
 * Flag MCQ_READS_INTERLEAVED (text2 NULL): records 2r, 2r+1 of text1 are the mates of one query, as sequence_pair_reader::next
 * pairs them under -pairseq (src/sequence_io.cpp:442-462: first = reader1_->next(), second = reader1_->next(), the second an
 * empty sequence once the file has run out).  Output in the paired form; a query is complete once both its records are (a
 * chunk that ends between two mates takes neither, the cut falls in front of the first mate); a last record without a mate,
 * in a chunk that ends the file, is a query with an empty second mate; max_queries / max_bases count pairs and the bases
 * of both mates; info[MCQ_READS_COMPLETE1] counts complete queries, _CUT2 and _COMPLETE2 are 0.                        */
#ifndef MCQ_READS_CONSTANTS             /* (the same in include/mcq.h) */
#define MCQ_READS_CONSTANTS
enum { MCQ_READS_EOF1 = 1u, MCQ_READS_EOF2 = 2u,
       MCQ_READS_INTERLEAVED = 4u };   /* text2 NULL: records 2q, 2q+1 of text1 are the mates of query q (see above) */
enum { MCQ_READS_N = 0, MCQ_READS_BASES = 1, MCQ_READS_CUT1 = 2, MCQ_READS_CUT2 = 3, MCQ_READS_STATUS = 4,
       MCQ_READS_COMPLETE1 = 5, MCQ_READS_COMPLETE2 = 6, MCQ_READS_INFO_WORDS = 8 };
enum { MCQ_READS_NOT_STRICT = 1u };   /* info[MCQ_READS_STATUS] of the device step: parse this chunk on the host */
#endif
int mcq_reads_parse(const char* text1, uint64_t len1, const char* text2, uint64_t len2, uint32_t flags,
                    uint64_t max_queries, uint64_t max_bases, char* bases, uint64_t* seq_off, uint64_t* hdr, uint64_t* info);

/* ---- the inputs of a build (mcq_build_cli): taxonomy dump, genome files, targets ---------------------------------------
 * mcq_taxdump_read: nodes.dmp, names.dmp (scientific names) and, if there, merged.dmp of `dir`, as make_taxonomic_hierarchy
 * (src/taxonomy_io.cpp:56-185) reads them: every old id of merged.dmp becomes a taxon of rank none below its new id and is
 * replaced by it in nodes.dmp; of several records with one id the first stays; taxon 1 gets rank root.  The records come in
 * the order the reference writes them (ascending id; the sequence-level taxa, id -(target + 1), go before them).  `name`
 * points into the handle; file is "", index and windows 0.                                                              */
typedef struct mcq_taxdump mcq_taxdump;
int mcq_taxdump_read(const char* dir, mcq_taxdump** out);
uint64_t mcq_taxdump_count(const mcq_taxdump* t);
const mcq_taxon_rec* mcq_taxdump_taxa(const mcq_taxdump* t);
int mcq_taxdump_free(mcq_taxdump* t);
/* name of the sequence-level taxon of a sequence with this header (the '>' line without the '>'): accession.version, else
 * accession, else the gi number, else the whole header (src/sequence_io.cpp:705-719, src/mode_build.cpp:591-596).  Written to
 * buf (NUL-terminated, cut to cap - 1 bytes); returns the length.  mcq_target_parent_taxid: the N of "taxid|N" in the header,
 * 0 if there is none (src/sequence_io.cpp:724-748) -- the parent a target gets when no mapping file names one (mapping files:
 * mcq_seq2tax_* and mcq_accmap_host below).                                                                             */
int64_t mcq_target_name(const char* header, uint64_t len, char* buf, size_t cap);
int64_t mcq_target_parent_taxid(const char* header, uint64_t len);
/* the files named by the arguments of a build, every directory expanded (recursively, 10 levels), then sorted: the order in
 * which the reference reads them (src/args_handling.cpp:50-90, src/filesys_utility.cpp:32-73, src/mode_build.cpp:570-575)   */
typedef struct mcq_file_list mcq_file_list;
int mcq_genome_files(const char* const* args, uint32_t n_args, mcq_file_list** out);
uint32_t mcq_file_list_count(const mcq_file_list* l);
const char* mcq_file_list_get(const mcq_file_list* l, uint32_t i);
int mcq_file_list_free(mcq_file_list* l);
/* Multi-line FASTA files read in order through one buffer of io_bytes.  mcq_genome_reader_next appends up to `cap` bases to
 * `bases`: the sequences of the targets back to back, in target order, a sequence going on in the next call when the buffer is
 * full (*done = 1: all files are read).  A target is a record with sequence text whose name is not taken yet (target ids
 * count only those); mcq_genome_reader_target gives target t's taxon record (id -(t + 1), parent from the header, rank
 * sequence, name, file, index of the record in its file from 1; windows 0: the build counts them) and its length so far,
 * for every target begun.  Lines are joined by dropping the '\n' only.  A file that does not start with '>' and a record
 * without sequence text end the reading of that file, as they do in the reference.  The extension decides how the reference
 * reads a file, its first character only without a known one (src/sequence_io.cpp:534-571): FASTA text under a FASTQ
 * extension is left as its FASTQ reader leaves it, a file or directory that cannot be read is passed over; a file the
 * reference would read as FASTQ is an error.
 * Host memory: io_bytes, one header line, and name + file + length per target.                                        */
typedef struct mcq_genome_reader mcq_genome_reader;
int mcq_genome_reader_open(const char* const* files, uint32_t n_files, uint64_t io_bytes, mcq_genome_reader** out);
int mcq_genome_reader_next(mcq_genome_reader* r, char* bases, uint64_t cap, uint64_t* n_bases, int32_t* done);
uint32_t mcq_genome_reader_n_targets(const mcq_genome_reader* r);
int mcq_genome_reader_target(const mcq_genome_reader* r, uint32_t target, mcq_taxon_rec* rec, uint64_t* length);
int mcq_genome_reader_close(mcq_genome_reader* r);
/* The reader for sequences that are ADDED to a database (`modify`: add_to_database on a database that was read,
 * src/mode_build.cpp:1117-1136): the names of the database's sequence-level taxa are taken before the first file is read
 * (name2tax_, src/sketch_database.h:533-534, :938-943), and the target ids go on behind the database's: target i of this reader
 * (i from 0, as mcq_genome_reader_target counts them) has the id n_old + i and the taxon id -(n_old + i + 1), n_old =
 * info.n_targets of `existing` (from either opener; only read during this call).  mcq_genome_reader_n_skipped: records with
 * sequence text that were passed over so far because their name was taken, by the database or earlier in this run.        */
int mcq_genome_reader_open_after(const char* const* files, uint32_t n_files, uint64_t io_bytes, const mcq_refdb* existing,
                                 mcq_genome_reader** out);
uint64_t mcq_genome_reader_n_skipped(const mcq_genome_reader* r);
/* every taxon record of an opened database in file order, as rank 0's file holds it (`windows` of a sequence-level taxon is
 * non-zero only for the targets rank 0 owns; mcq_refdb_tgt_windows has every target's): out[n_taxa]; name and file point into
 * the handle.  What a `modify` carries forward into the files it writes.                                                  */
int mcq_refdb_taxa(const mcq_refdb* db, mcq_taxon_rec* out /* [n_taxa] */);

/* ---- mapping files: which taxon a sequence belongs to when its header does not say -----------------------------------
 * Pre-mapping (make_sequence_to_taxon_id_map and find_taxon_id, src/taxonomy_io.cpp:190-310, src/mode_build.cpp:531-550):
 * mcq_seq2tax_read reads <dir>/assembly_summary.txt, if it opens, for every distinct directory of the genome FILES (what is in
 * front of a name's last '/' or '\\'; in std::set order).  mcq_seq2tax_add_file reads one file of that kind into the map
 * (*opened = 0 and nothing read if it does not open).  A file is read as the reference reads it: up to 10 leading '#' lines, of
 * which the last is the header row (else the first line is); the header's first word is dropped, the others count from 0;
 * `taxid` names taxcol, `accession.version` / `assembly_accession` keycol; a line is keycol TABs passed, a word (the key), taxcol
 * TABs passed, an integer; without a taxid column the whole file is read again as key TAB taxid.  The first entry of a key
 * stays.  mcq_seq2tax_find: the exact key, else the first key greater than `name` if it begins with it, else 0.  Entries come in
 * key order.
 * mcq_genome_reader_open_mapped: mcq_genome_reader_open (existing = NULL) or _open_after with the map (NULL: none; copied).  A
 * target's parent then is the map's entry for its name, else for the accession string of its FILE's name
 * (extract_accession_string, no fall-back to the whole name), else the N of taxid|N in its header, else 0
 * (src/mode_build.cpp:591-604).                                                                                            */
typedef struct mcq_seq2tax mcq_seq2tax;
int mcq_seq2tax_create(mcq_seq2tax** out);
int mcq_seq2tax_add_file(mcq_seq2tax* m, const char* path, int32_t* opened);
int mcq_seq2tax_read(const char* const* genome_files, uint32_t n_files, mcq_seq2tax** out);
uint64_t mcq_seq2tax_count(const mcq_seq2tax* m);
int mcq_seq2tax_entry(mcq_seq2tax* m, uint64_t i, const char** key, int64_t* taxid);
int64_t mcq_seq2tax_find(const mcq_seq2tax* m, const char* name, uint64_t len);
int mcq_seq2tax_free(mcq_seq2tax* m);
int mcq_genome_reader_open_mapped(const char* const* files, uint32_t n_files, uint64_t io_bytes, const mcq_refdb* existing,
                                  const mcq_seq2tax* seq2tax, mcq_genome_reader** out);
/* Post-mapping (try_to_rank_unranked_targets, src/mode_build.cpp:493-522, :248-312).  mcq_taxmap_files: the files in the order
 * they are read: `postmap` (-taxpostmap; NULL or "": none), then nucl_gb, nucl_wgs, nucl_est, nucl_gss .accession2taxid of
 * `taxdir` (named whether they exist or not; a file that does not open is passed over by the caller), then every other file below
 * taxdir whose path contains ".accession2taxid" (src/args_handling.cpp:122-145).  DIVERGENCES: those last ones come in name order
 * (the reference: readdir's order); taxdir NULL or "" names no file but `postmap` (the reference looks in the working directory).
 * mcq_accmap_host: the reference's parser of one such text: the first line is passed over unread (skip_first_line != 0; 0 for
 * text that goes on in the middle of a file), then `acc accver taxid gi` are read as blank-separated words that may run across
 * lines, taxid as an unsigned 64-bit number; the text ends at the first record that does not parse, or when no target is left
 * unranked.  names_blob / name_off / name_target: the sorted names as mcq_accmap_create (include/mcq.h) takes them.  A record's
 * target (the one named accver, else the first name greater than acc that begins with it, else the one named gi) gets
 * parent[t] = taxid and unranked[t] = 0 if unranked[t] was set; other entries of `parent` stay.  *n_records (may be NULL): records
 * read.  The fall-back of mcq_accmap_chunk for text that is not strict, and the CPU yardstick.                               */
int mcq_taxmap_files(const char* taxdir, const char* postmap, mcq_file_list** out);
int mcq_accmap_host(const char* text, uint64_t n_bytes, int32_t skip_first_line, const char* names_blob, const uint64_t* name_off,
                    uint64_t n_names, const uint32_t* name_target, uint8_t* unranked /* [n_targets] in, out */,
                    int64_t* parent /* [n_targets] in, out */, uint32_t n_targets, uint64_t* n_records);
/* mcq_accmap_host_rule: the same parser -- words across lines, num_get's number, the end at the first record that does not parse or
 * when nothing is left unranked, the first line passed over on request -- under a rule of mcq_accmap_create_rule (include/mcq.h):
 * 0 is mcq_accmap_host; under 1 / 2 / 3 a record's target is the one named exactly by its acc / accver / gi word and no other, what
 * read_mappings_from_file of the reference's `annotate` enters into its map (src/mode_annotate.cpp:181-229; an id keeps its first
 * taxid).  The fall-back of a handle with that rule for text that is not strict, and the CPU yardstick.
 * For a caller that streams a file through a buffer: *n_consumed (may be NULL) = the bytes of text up to the end of the last whole
 * record (the end of the first line passed over if there is none); *stopped (may be NULL) = 0 when the reading ended because the
 * text ran out, inside a record or between two -- the caller goes on with text + *n_consumed and what follows --, 1 when it ended
 * for good: a taxid that does not parse, or nothing left unranked.  Text that is not the end of its file should end behind a white
 * space byte, so that its last word is whole.                                                                                   */
int mcq_accmap_host_rule(const char* text, uint64_t n_bytes, int32_t skip_first_line, const char* names_blob, const uint64_t* name_off,
                         uint64_t n_names, const uint32_t* name_target, uint8_t* unranked /* [n_targets] in, out */,
                         int64_t* parent /* [n_targets] in, out */, uint32_t n_targets, uint32_t rule, uint64_t* n_records,
                         uint64_t* n_consumed, int32_t* stopped);

/* ---- annotate: taxid|N written into the headers of a genome file (mcq_annotate_cli; src/mode_annotate.cpp:238-311) -----
 * mcq_annotate_id: the id of a header LINE -- the whole line with its '>' or '@', as annotate_with_taxid hands it to the extractors
 * (src/sequence_io.cpp:576-700) -- of id_type 1 (acc: extract_ncbi_accession_number), 2 (accver: ..._version_number) or 3 (gi:
 * extract_genbank_identifier): the values of MCQ_ACCMAP_RULE_ACC / _ACCVER / _GI.  So a header without a known prefix but with a
 * '.' before byte 25 gives, under accver, an id that begins with '>' and that no mapping line names.  Written to buf
 * (NUL-terminated, cut to cap - 1 bytes); returns the length (0: no id), -1 on an error.
 * mcq_annotate_rewrite: the line as annotate writes it.  An old taxid is cut first: from the first "taxid" -- if value_sep occurs
 * from 4 bytes behind its start on -- through the first field_sep behind that value separator, else through the next value_sep, else
 * to the end of the line.  Then, if has_id, "taxid" value_sep N field_sep goes in ONE byte behind the start of the first field_sep
 * (also when field_sep is longer than one byte: the reference's ipos + 1), or field_sep "taxid" value_sep N field_sep is appended
 * when there is none.  Without an id the line only loses its old taxid.  The separators must not be empty.  Written to buf as
 * above (the new line is at most len + 25 + 2 x strlen(field_sep) + strlen(value_sep) bytes); returns its length, -1 on an error. */
int64_t mcq_annotate_id(const char* line, uint64_t len, uint32_t id_type, char* buf, size_t cap);
int64_t mcq_annotate_rewrite(const char* line, uint64_t len, int32_t has_id, uint64_t taxid, const char* field_sep,
                             const char* value_sep, char* buf, size_t cap);

/* ---- merging query result files: the host side of the reference's `merge` mode (the device side: mcq_merge_* of include/mcq.h) ----
 * mcq_refdb_from_taxdump: a database that is a taxonomy alone -- the taxa of a dump in its order, no target, no table; the taxon
 * functions above (id, name, rank, ancestor, lineages, classify, abundance text, statistics) work on it unchanged.
 * mcq_refdb_taxid_table: the taxon ids of a database strictly ascending with the taxon index taxon_with_id gives for each (of two
 * taxa with one id the one the id map holds): what mcq_merge_create takes.  ids / index: [n_taxa]; *n_ids: how many were written.
 * mcq_results_properties: get_results_file_properties (src/mode_merge.cpp:131-200) -- only '#' lines up to one that begins with
 * "# Classification" (which must not hold "sequence"), then only '#' lines up to "# TABLE_LAYOUT:", whose first column must be
 * query_id; *tophits_column = the number of '|' in front of the column named top_hits (it must be 2 or more: behind the query
 * header); *results_begin = the byte at which the first line that does not begin with '#' begins (the file's size if there is
 * none); *n_lines = the number of lines from there on that do not begin with '#' (an empty line counts).  Every rejection is an
 * error whose text names the file.
 * mcq_merge_host: read_results (src/mode_merge.cpp:209-264) over text that holds whole lines of a results file: lines that begin
 * with '#' are skipped; of the others the unsigned id is read (white space in front of it skipped, line ends included), the
 * stream goes behind the next '|', the header is the next blank-delimited token, the stream goes behind tophits_column - 1 more
 * '|' and behind the next TAB, and until the next character is a TAB it reads taxid (signed 64-bit), goes behind ':', reads hits
 * (unsigned 64-bit) and one character.  Line l of the output names query line_query[l] (0-based: id - 1), holds the items
 * [item_off[l], item_off[l + 1]) of taxid / hits and its header token at header_off[l] = text_offset + its place in text, header_len[l]
 * bytes: the arrays of mcq_merge_lines.  item_off holds line_cap + 1 words; the number of '\n' + 1 and the number of ':' bound the
 * lines and the items.  Ids may repeat: the caller cuts its mcq_merge_lines calls there.
 * DIVERGENCES, all errors whose text is `file_name: line N: ...` (N = first_line_no + the line's index in text): where the
 * reference's stream goes bad inside a line the reference never returns (its loop waits for a TAB); id 0 (the reference takes it
 * for id 1) and an id beyond n_queries (the reference writes past its vectors); a '|' inside the header token (the reference
 * parses such a line in two ways, depending on whether it knows the query's header already); hits of 2^32 or more.              */
int mcq_refdb_from_taxdump(const mcq_taxdump* dump, mcq_refdb** out);
int mcq_refdb_taxid_table(const mcq_refdb* db, int64_t* ids, uint32_t* index, uint64_t* n_ids);
int mcq_results_properties(const char* path, uint32_t* tophits_column, uint64_t* results_begin, uint64_t* n_lines);
int mcq_merge_host(const char* text, uint64_t n_bytes, uint32_t tophits_column, uint64_t n_queries, const char* file_name,
                   uint64_t first_line_no, uint64_t text_offset, uint32_t* line_query, uint64_t* item_off, int64_t* taxid,
                   uint32_t* hits, uint64_t* header_off, uint32_t* header_len, uint64_t line_cap, uint64_t item_cap,
                   uint64_t* n_lines, uint64_t* n_items);

/* default of -hitmin when unset: src/mode_query.cpp:247-259 */
uint32_t mcq_default_hits_min(uint32_t sketch_size);
uint32_t mcq_rank_from_name(const char* name);
const char* mcq_rank_name(uint32_t rank);
const char* mcq_host_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
