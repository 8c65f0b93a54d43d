/* mcq.h -- C ABI of the MI355X query-path engine for MetaCache-MPI.
 *
 * This is the drop-in boundary.  The reference has no
 * plugin/FFI API; the seam is the per-read body + candidate merge inside
 * query_batched_parallel2 (reference src/querying.h:792-825 and :867-1073), i.e.
 *
 *   database::accumulate_matches(seq, res, offsets)     src/sketch_database.h:826-833
 *     -> sketcher::operator()(first,last)               src/hash_dna.h:113-152
 *     -> hash_multimap::find(key)                       src/hash_multimap.h:778-789
 *   merge_sort(a, offsets, b)                           src/querying.h:88-106
 *   classification_candidates{db, matches, rules}       src/candidates.h:207-219
 *   classification_candidates::insert(cand, db, rules)  src/candidates.h:236-285
 *   MPI tree merge of (qid,taxid,hits) triplets         src/querying.h:867-1073
 *
 * Each entry point below says which of these it replaces.  Plain pointers and
 * sizes only; 0 = success, negative = error (mcq_last_error() gives the text);
 * nothing throws across the boundary.  All buffers are caller-owned.
 *
 * Vocabulary: a *sequence* is one read (or mate); a *query* is one read or one
 * read pair; a *location* is (target id, window id) packed as (tgt << 32) | win;
 * a *feature* is one 32-bit min-hash value of a window sketch.
 */
#ifndef MCQ_H
#define MCQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mcq_db mcq_db;   /* GPU-resident feature -> locations multimap (one shard) */
typedef struct mcq_ws mcq_ws;   /* per-caller workspace; one per concurrent mcq_query     */

enum {
    MCQ_OK = 0,
    MCQ_E_ARG = -1,        /* bad argument                                            */
    MCQ_E_HIP = -2,        /* HIP runtime error                                       */
    MCQ_E_CAPACITY = -3,   /* a query exceeded the workspace's per-query capacity     */
    MCQ_E_UNSUPPORTED = -4 /* parameter outside what the kernels are built for        */
};

/* flags */
enum {
    MCQ_DEVICE_PTRS = 1u,       /* the pointers in this struct are device pointers     */
    MCQ_QUIRK_SEQ_DROP = 2u,    /* emulate the reference's u32 wire format: a sequence-
                                   level taxon (key bit 31 set) sent by a non-root rank
                                   is dropped (src/querying.h:958, :983-985)            */
    MCQ_BATCH_RANGES = 8u,      /* mcq_batch.flags (device pointers only): seq_off holds 2*n_seqs
                                   (begin,end) byte ranges into `bases` instead of n_seqs+1 offsets:
                                   the sequences may sit anywhere in the buffer, e.g. inside raw
                                   FASTQ text indexed by mcq_fastq_index                          */
    MCQ_BATCH_PACKED = 0x10u,   /* mcq_batch.flags: `bases` is not ASCII but the packed form mcq_pack_bases writes (3 bits per
                                   base instead of 8: what a host that keeps its reads packed sends over PCIe): u32 words of
                                   2-bit codes, 16 bases per word, first base in the top bits (A/a 0, C/c 1, G/g 2, T/t 3), one
                                   zero pad word, then u32 words of ambiguity bits, 32 bases per word, first base in the top bit
                                   (1 = not ACGT: src/dna_encoding.h:326-336), one zero pad word.  seq_off stays in bases;
                                   mcq_batch.n_bases = seq_off[n_seqs].  Not with MCQ_BATCH_RANGES                        */
    MCQ_FORCE_BLOCK_PATH = 0x100u, /* test hook: every query takes the workgroup path    */
    MCQ_FORCE_RAW_SORT = 0x400u,   /* test hook: the wave path sorts the raw match list instead of
                                      de-duplicating it first (the path of > 256 distinct keys / 64-bit keys) */
    MCQ_NO_WAVE16 = 0x800u,        /* test hook: queries of 513..1024 locations take the workgroup path
                                      instead of the second wave stage                     */
    MCQ_NO_TWO_CLASS = 0x4000u,    /* test hook: long match lists are sorted whole instead of taking the two-class tail
                                      (light / heavy locations: DESIGN.md section 4); same results either way            */
    MCQ_FOLD_BY_LISTS = 0x8000u,   /* test hook: emulate_ranks > 1 builds the P bounded lists and folds them level by level (the form
                                      MCQ_QUIRK_SEQ_DROP needs on a table with sequence-level taxa) instead of the one selection
                                      in the order (hits, rank, position) that gives the same list        */
    MCQ_FORCE_LEAN_WAVE = 0x20000u, /* test hook / A-B: the first wave stage in its lean form: it answers the
                                      reads of at most 256 locations and queues every other one for the later stages.  Only where that form exists (a table of the default sketch geometry -- k 16, sketch 16, windows
                                      128 / 113, DESIGN.md section 17 --, 32-bit location words, P x M within a wave's
                                      lanes, not with another MCQ_FORCE_* / MCQ_NO_WAVE16 hook): MCQ_E_UNSUPPORTED otherwise   */
    MCQ_FORCE_FULL_WAVE = 0x40000u, /* test hook / A-B: the first wave stage in its full form, whatever the batch before it
                                      suggests.  Same results with either flag and with neither                      */
    MCQ_BUILD_REMOVE_OVERPOPULATED = 0x1000u, /* mcq_build_desc.flags: the build option
                                   -remove-overpopulated-features (src/mode_build.cpp:847-1074): a feature whose
                                   per-rank location counts (after the per-rank limit) sum to more than
                                   max_locs - 1 is removed from every rank                                  */
    MCQ_DB_LOCS_64 = 0x200u,    /* mcq_db_desc.flags: keep 64-bit locations in HBM even when
                                   (tgt,win) would fit a 32-bit form                     */
    MCQ_DB_LOCS_GW = 0x2000u,   /* mcq_db_desc.flags: 32-bit locations in the global-window form (first window of the
                                   target + window) even when the two bit fields would fit 32 bits.  Without either
                                   flag the handle picks: bit fields (tgt << wb) | win if they fit 32 bits, else the
                                   global-window form if the table has fewer than 2^32 - 1 windows (any table the
                                   reference can hold below ~485 Gbp, src/config.h:54-67), else 64-bit words  */
    MCQ_DB_SLOTS_16 = 0x4000u,  /* mcq_db_desc.flags: 16-B slots, every list behind the slot array           */
    MCQ_DB_BUCKETS_64 = 0x8000u /* mcq_db_desc.flags: 64-B buckets, lists of up to 14 (7) locations inside them.
                                   Without either flag the layout follows the table: buckets while the mean list has
                                   at most 4 locations, slots beyond                  */
};

/* Database description = the union of the reference's P shard tables
 * (hash_multimap contents, src/hash_multimap.h:923-964) plus the metadata the
 * candidate step needs.  keys are unique; list i = locs[list_off[i] .. list_off[i+1])
 * sorted ascending by (tgt,win).  tgt2tax[t] is the taxon key insert() works on for
 * target t: db.ancestor(taxon_of_target(t), mergeBelow) if it exists, else a key with
 * bit 31 set that is unique to the target (src/candidates.h:242-245).  Keys are opaque
 * to the engine except bit 31.
 * n_shards/shard_id: this handle stores only keys with mcq_owner(key, n_shards) ==
 * shard_id (the caller may pass all keys; foreign ones are skipped).               */
typedef struct {
    /* Limits narrower than the reference's, by construction of the kernels (MCQ_E_UNSUPPORTED beyond them):
     * k <= 16 is the reference's own limit for 32-bit k-mers (src/config.h:47); winlen <= 128 (`-winlen` is free in
     * the reference, src/mode_build.cpp:67; one wave holds a window as 2 bases per lane) and sketch_size <= 32 (the
     * selection network sorts 64 candidates) cover its defaults (128 / 16) and every shipped script.              */
    uint32_t k;               /* k-mer length, 1..16 (src/hash_dna.h:75)              */
    uint32_t sketch_size;     /* s, 1..32 (src/mode_build.cpp:66)                     */
    uint32_t winlen;          /* query window length, k..128 (src/sketch_database.h:256) */
    uint32_t winstride;       /* query window stride                                  */
    uint32_t tgt_winstride;   /* target window stride (range width, classification.cpp:217) */
    uint32_t n_targets;
    uint64_t n_keys;
    uint64_t n_locs;
    const uint32_t* keys;       /* [n_keys]                                           */
    const uint64_t* list_off;   /* [n_keys + 1]                                       */
    const uint64_t* locs;       /* [n_locs]  (tgt << 32) | win                        */
    const uint32_t* tgt2tax;    /* [n_targets]                                        */
    uint32_t n_shards;          /* >= 1                                               */
    uint32_t shard_id;
    uint32_t flags;             /* MCQ_DEVICE_PTRS, MCQ_DB_LOCS_64 / _GW, MCQ_DB_SLOTS_16 / MCQ_DB_BUCKETS_64 */
    int32_t  device;            /* HIP device ordinal                                 */
    uint32_t loc_win_bits;      /* 0 = derive from the data.  Shards built from different
                                   data must agree on the location format: pass the bit width
                                   of the largest window id of the WHOLE database          */
    const uint32_t* tgt_windows; /* [n_targets] windows of every target (the reference's taxon `windows` field of the
                                   owning rank, src/taxonomy.h:326-335), or NULL = 1 + the largest window id found in
                                   `locs`.  Only the global-window form reads it; shards that are created from
                                   different subsets of the locations must all pass it (same location words everywhere) */
} mcq_db_desc;

/* One batch of sequences: bases[seq_off[i] .. seq_off[i+1]) is sequence i (ASCII,
 * A/C/G/T any case, anything else is ambiguous: src/dna_encoding.h:326-336).
 * paired != 0: sequences 2q and 2q+1 are the mates of query q
 * (sequence_pair_reader::sequence_pair, src/sequence_io.h:204).                     */
typedef struct {
    uint64_t n_seqs;
    const char* bases;
    const uint64_t* seq_off;    /* [n_seqs + 1] */
    uint32_t paired;
    uint32_t flags;             /* MCQ_DEVICE_PTRS, MCQ_BATCH_RANGES, MCQ_BATCH_PACKED */
    uint64_t n_bases;           /* MCQ_BATCH_PACKED with device pointers: bases of the whole batch (locates the planes) */
} mcq_batch;

/* bytes of the packed form of n_bases bases, and the packer: ASCII (host, or device with MCQ_DEVICE_PTRS: then a
 * kernel on `stream`) -> packed buffer of mcq_packed_bytes(n_bases) bytes in the same memory space                  */
uint64_t mcq_packed_bytes(uint64_t n_bases);
int mcq_pack_bases(const char* bases, uint64_t n_bases, void* out, uint32_t flags, void* stream);

/* classification_options / candidate_generation_rules subset that the path uses
 * (src/query_options.h:123-135, src/candidates.h:89-101).                            */
typedef struct {
    uint32_t max_cand;          /* maxNumCandidatesPerQuery, 1..16.  (The reference's `-maxcand 0` = unbounded list,
                                   src/query_options.cpp:176-178, is not offered: past 16 entries its std::sort
                                   is an unstable introsort, so results stop being defined by the inputs.)   */
    uint32_t emulate_ranks;     /* P of the reference run to match (fold order of src/querying.h:867-1073),
                                   1..64; 1 = single list, no fold.  The P lists and their fold are computed as ONE
                                   bounded selection in the order (hits, rank, position) -- the same list,
                                   at the same cost for every P and max_cand (the reference's scripted -n 32 / -n 64 with
                                   -maxcand 4, script/ft/QueryGeneric_FT.sh:115, included).  Only MCQ_QUIRK_SEQ_DROP on a
                                   table with sequence-level taxa carries the lists out: in the lanes of a wave while
                                   pow2ceil(P) x max_cand <= 64, in four registers per lane up to 256 list slots, beyond
                                   that in the LDS of the workgroup kernel (every query, several times slower)          */
    uint64_t insert_size_max;   /* insertSizeMax                                         */
    uint32_t flags;             /* MCQ_QUIRK_SEQ_DROP and the MCQ_FORCE_* (_LEAN_WAVE / _FULL_WAVE included) / MCQ_NO_WAVE16 / MCQ_NO_TWO_CLASS / MCQ_FOLD_BY_LISTS test hooks; any other
                                   bit is rejected with MCQ_E_ARG                         */
} mcq_query_opts;

/* match_candidate (src/candidates.h:66-81) with the taxon as its key.  After a fold
 * (emulate_ranks > 1) window positions are (0,0), as in the reference's wire format. */
typedef struct {
    uint32_t tax;
    uint32_t hits;
    uint32_t win_beg;
    uint32_t win_end;
} mcq_cand;

typedef struct {
    mcq_cand* cands;            /* [n_queries * max_cand]                              */
    uint32_t* n_cand;           /* [n_queries]                                         */
    uint32_t flags;             /* MCQ_DEVICE_PTRS                                     */
} mcq_result;

/* counters of the last mcq_query on a workspace (for the roofline accounting) */
typedef struct {
    uint64_t n_queries;
    uint64_t n_features;        /* sketch features looked up                           */
    uint64_t n_hit_features;    /* features with a non-empty list                      */
    uint64_t n_locations;       /* locations gathered                                  */
    uint64_t n_cands;           /* candidates written                                  */
    uint64_t n_overflow;        /* queries that left the first wave stage (second wave
                                   stage or block-per-query path)                      */
    uint64_t n_two_class;       /* queries answered by the two-class tail (heavy locations sorted, light ones only
                                   as far as they can enter a top list)                */
    uint64_t n_two_class_retry; /* queries that tail could not prove exact and handed on to the exact path */
    uint64_t n_narrow_queued;   /* queries with narrow window ranges (short reads, pairs) counted in the workgroup kernels' queue:
                                   from 4096 on they get the workgroup kernel with the two-class tail (an upper bound: an
                                   entry may be counted twice)                                            */
    uint64_t n_lean_queued;     /* queries the lean first wave stage handed to the second one that the full stage would have
                                   answered itself (not part of n_overflow, which is the same on both routes)         */
} mcq_stats;

/* replaces sketch_database::read -> hash_multimap::deserialize (the table build) */
int mcq_db_create(const mcq_db_desc* desc, mcq_db** out);
int mcq_db_destroy(mcq_db* db);
/* The same for a table that is larger than the memory for its one-piece description (RefSeq scale: 1.7e10 locations are
 * 136 GB as 64-bit words): handed over in parts, e.g. one per feature-hash range (mcq_build_parts makes them) or one per
 * shard file of the reference (src/sketch_database.h:858-999, after mapping (tgt, win) to tgt_windows' prefix sums + win).
 * Device memory only (MCQ_DEVICE_PTRS).  desc->keys / list_off / locs / n_keys / n_locs are ignored, desc->tgt_windows is
 * required: part locations are global-window words, and the handle keeps that form.  A key may appear in one part only. */
typedef struct {
    uint64_t n_keys, n_locs;
    const uint32_t* keys;       /* [n_keys]                                                             */
    const uint32_t* list_len;   /* [n_keys] lengths of the lists, which follow one another in `locs`    */
    const uint32_t* locs;       /* [n_locs] global window indices, every list ascending                 */
} mcq_db_part;
int mcq_db_create_parts(const mcq_db_desc* desc, const mcq_db_part* parts, uint32_t n_parts, mcq_db** out);
/* bytes of HBM held by the handle */
uint64_t mcq_db_bytes(const mcq_db* db);

/* max_queries / max_bases bound one batch; max_locs_per_query bounds the match list
 * of a single query on the block-per-query path (0 = default 1<<18).                 */
int mcq_ws_create(const mcq_db* db, uint64_t max_queries, uint64_t max_bases,
                  uint64_t max_locs_per_query, mcq_ws** out);
int mcq_ws_destroy(mcq_ws* ws);

/* The whole per-read path for one batch: rows 1-11 of SURVEY.md 8a.  Replaces the
 * worker body of query_batched_parallel2 (src/querying.h:792-825) and the MPI tree
 * merge (:867-1073).  stream is a hipStream_t (NULL = default stream).  With device
 * pointers the call only enqueues work; with host pointers it copies in, runs,
 * copies out and synchronises the stream.                                           */
int mcq_query(const mcq_db* db, mcq_ws* ws, const mcq_batch* in, const mcq_query_opts* opt,
              mcq_result* out, void* stream);

/* The same for a caller that streams batch after batch from HOST buffers (pinned memory for full speed): the call
 * returns once the work is enqueued; batch i+1 is copied in and batch i-1 copied out on their own streams while
 * batch i computes (two batches in flight, staging inside the workspace).  *ticket names the call; mcq_ws_wait(ticket)
 * returns when its results are in `out` -- until then `in` and `out` must stay untouched.  Calls complete in order.
 * ASCII bases: bound by PCIe (157 MB per 1 M x 150 bp reads); MCQ_BATCH_PACKED: bound by the kernels.               */
int mcq_query_pipelined(const mcq_db* db, mcq_ws* ws, const mcq_batch* in, const mcq_query_opts* opt,
                        mcq_result* out, uint64_t* ticket);
int mcq_ws_wait(mcq_ws* ws, uint64_t ticket);

/* Waits for the stream, returns MCQ_E_CAPACITY if any query of the last call on ws
 * overflowed the workspace, fills stats (may be NULL).                              */
int mcq_ws_sync(mcq_ws* ws, void* stream, mcq_stats* stats);

/* ---- staged entry points (feature-sharded multi-GPU path) ---------
 * mcq_count_windows: row 1.  win_off[i] = first window of sequence i among the windows of the batch, win_off[n_seqs] =
 *               their number (an empty sequence has one, empty, window).
 * mcq_sketch  : rows 1-5.  win_off comes from mcq_count_windows.  One row of sketch_size features per window:
 *               features[w * sketch_size + i] for i < n_feat[w], ascending; the unused slots of a row are 0xFFFFFFFF.
 *               ASCII batches only (MCQ_BATCH_PACKED is rejected with MCQ_E_ARG).
 * mcq_lookup_*: rows 6-7 on the owning shard (counts, then gather).
 * mcq_assemble / mcq_reduce: rows 8-11 on the home GPU.                              */
int mcq_count_windows(const mcq_db* db, const mcq_batch* in, uint64_t* win_off /* [n_seqs+1] */, void* stream);
int mcq_sketch(const mcq_db* db, const mcq_batch* in, const uint64_t* win_off,
               uint32_t* features, uint32_t* n_feat, void* stream);
/* mcq_lookup_count: list length per feature (0 for absent / foreign / 0xFFFFFFFF); if
 *   list_src is not NULL it also receives where each list starts in the shard, so that
 *   mcq_lookup_gather need not probe again.
 * mcq_lookup_gather: concatenates the lists at out_off[i] in the handle's NATIVE location
 *   width: mcq_db_loc_bytes() = 4 ((tgt << mcq_db_win_bits()) | win, or the global window index: mcq_db_layout_get)
 *   or 8 ((tgt << 32) | win).
 *   The native width is what travels between GPUs.                                     */
int mcq_lookup_count(const mcq_db* db, const uint32_t* features, uint64_t n_features,
                     uint32_t* list_len, uint64_t* list_src, void* stream);
int mcq_lookup_gather(const mcq_db* db, const uint32_t* features, uint64_t n_features,
                      const uint32_t* list_len, const uint64_t* list_src,
                      const uint64_t* out_off /* [n_features+1] */, void* out_locs, void* stream);
uint32_t mcq_db_loc_bytes(const mcq_db* db);
uint32_t mcq_db_win_bits(const mcq_db* db);
/* what a handle was built as (chosen per table by mcq_db_create) */
enum { MCQ_LOC_FIELDS64 = 0, MCQ_LOC_FIELDS32 = 1, MCQ_LOC_GLOBAL_WINDOW = 2 };
typedef struct {
    uint32_t loc_bytes;         /* 4 or 8                                                                */
    uint32_t loc_format;        /* MCQ_LOC_*: (tgt << 32) | win, (tgt << win_bits) | win, or gw_offsets[tgt] + win */
    uint32_t win_bits;
    uint32_t bucket_bytes;      /* 64 (lists of up to 14 / 7 locations inside the bucket) or 16           */
    uint32_t slots_per_key;     /* 4 or 2: load factor <= 0.25 / 0.5                                      */
    uint64_t n_slots, n_keys, n_locs;   /* of this shard                                                  */
    uint64_t n_ext_locs;        /* locations behind the slot array                                        */
    uint64_t n_windows;         /* global-window form: windows of the whole database                      */
    uint64_t bytes;             /* = mcq_db_bytes                                                         */
    const uint32_t* gw_offsets; /* device, [n_targets + 1]; NULL unless MCQ_LOC_GLOBAL_WINDOW             */
} mcq_db_layout;
int mcq_db_layout_get(const mcq_db* db, mcq_db_layout* out);
/* mcq_assemble: home side, after the lists came back.  List i (list_len[i] native-width
 *   locations, consecutive in src_locs) belongs to feature slot src_slot[i] of the batch's
 *   [window][sketch_size] feature array.  Produces the per-query segments mcq_reduce takes:
 *   loc_off[n_queries+1], query_len[n_queries] (sum of the mates' lengths) and dst_locs.   */
int mcq_assemble(const mcq_db* db, uint64_t n_lists, const uint32_t* list_len, const uint32_t* src_slot,
                 uint64_t n_slots, const void* src_locs, const mcq_batch* in, const uint64_t* win_off,
                 uint64_t* loc_off, uint32_t* query_len, void* dst_locs, void* stream);
/* mcq_reduce: rows 8-11 per query from native-width location segments (any order inside). */
int mcq_reduce(const mcq_db* db, mcq_ws* ws, uint64_t n_queries, const uint64_t* loc_off /* [n_queries+1] */,
               const void* locs, const uint32_t* query_len, const mcq_query_opts* opt, mcq_result* out, void* stream);

/* mcq_bucket_features: groups the non-empty features by owning shard.  counts is a device
 *   array of n_shards u64 receiving the per-shard counts; bucketed/src_index receive,
 *   shard after shard, the features and the slot (index into `features`) each came from. */
int mcq_bucket_features(const uint32_t* features, uint64_t n, uint32_t n_shards,
                        uint64_t* counts, uint32_t* bucketed, uint32_t* src_index, void* stream);

/* shard that owns a feature: a range of h2(f) = thomas_mueller_hash(f)
 * (src/hash_int.h:39-45), never of f itself                          */
uint32_t mcq_owner(uint32_t feature, uint32_t n_shards);

/* Per-kernel timing of the path's kernels (HIP events between them on the call's stream), for the
 * roofline line of bench.py.  enable != 0 starts recording.  mcq_ws_kernel_times returns, summed over
 * the batches since enabling, the milliseconds of ms[0] the first wave stage (k_query_wave / k_reduce_wave),
 * ms[1] the second and third wave stages (k_query_wave16 + k_query_wave32 / k_reduce_wave16), ms[2] the workgroup kernels
 * (k_query_block plain + two-class / k_reduce_block), and the number of batches; mcq_ws_kernel_time their total.
 * Both synchronise the recorded events.                                                   */
int mcq_ws_timing(mcq_ws* ws, int enable);
int mcq_ws_kernel_times(mcq_ws* ws, double* ms /* [3] */, uint64_t* n_batches);
int mcq_ws_kernel_time(mcq_ws* ws, double* total_ms, uint64_t* n_batches);

/* ---- feature-sharded multi-GPU path behind one call (csrc/mcq_shard.hip) ----------------------
 * One process per GPU.  Replaces, for a table that is partitioned over n_ranks GPUs, what mcq_query replaces on one:
 * the worker body of query_batched_parallel2 and the MPI tree merge (src/querying.h:792-825, :867-1073).  The table
 * is partitioned by hash range of h2(feature) (mcq_owner) instead of the reference's tgt % P
 * (src/sketch_database.h:540-542); every rank queries its own reads; features travel to their owners and location
 * lists back (two exchanges per batch), the reduce kernels read the received lists in place.  Results equal
 * mcq_query's on the whole table, bit for bit (emulate_ranks reproduces the reference's fold order as there).
 *
 * Transport of the exchanges: RCCL (ncclSend / ncclRecv groups on the call's stream; librccl is loaded at run time)
 * after mcq_shard_comm_rccl, a device copy when n_ranks == 1, or the caller's function (mcq_shard_set_exchange;
 * synchronous: the engine waits for the stream before calling it).
 *
 * All calls are collective: every rank makes the same calls with the same flags in the same order.               */
typedef struct mcq_shard mcq_shard;
#define MCQ_SHARD_UNIQUE_ID_BYTES 128
enum { MCQ_SHARD_EXACT = 1u };   /* mcq_shard_query flags: exchange exact sizes (count exchanges through the host) */

typedef struct {
    uint32_t n_ranks;                  /* 1..32 */
    uint32_t rank;
    uint64_t max_queries;              /* per batch and rank */
    uint64_t max_seqs;                 /* 0 = max_queries (2 x for pairs) */
    uint64_t max_bases;                /* per batch and rank: bounds the number of windows */
    uint64_t max_locs_per_query;       /* as in mcq_ws_create; 0 = default */
    uint64_t max_features_per_peer;    /* capacity of one peer's feature block; 0 = twice the even share of the batch */
    uint64_t max_locations_per_peer;   /* capacity of one peer's location block to start with; 0 = sized by the table: the first
                                          batch of a context runs in the exact mode, its owner-side lookup first counts, and
                                          every rank allocates blocks for the largest count any rank served + 1/8.  An exact
                                          batch that outgrows the blocks allocates larger ones the same way (collectively);
                                          a padded batch that does is reported by mcq_shard_sync as MCQ_E_CAPACITY (never
                                          answered wrongly in silence) and its repeat with MCQ_SHARD_EXACT grows them.
                                          Identical on every rank.                                                          */
} mcq_shard_cfg;

/* moves send_bytes[p] bytes at send_base + send_off[p] to rank p and receives recv_bytes[p] bytes from rank p at
 * recv_base + recv_off[p], p = 0 .. n_ranks-1 (device pointers; own rank included); returns 0 on success, and only
 * when the received bytes are in place                                                                            */
typedef int (*mcq_exchange_fn)(void* user, const void* send_base, const uint64_t* send_off, const uint64_t* send_bytes,
                               void* recv_base, const uint64_t* recv_off, const uint64_t* recv_bytes,
                               uint32_t n_ranks, uint32_t rank);

int mcq_shard_create(const mcq_db* shard /* n_shards = n_ranks, shard_id = rank */, const mcq_shard_cfg* cfg, mcq_shard** out);
int mcq_shard_destroy(mcq_shard* ctx);
/* rank 0 makes the id (ncclGetUniqueId), the launcher carries it to the other ranks (the reference's world would use
 * MPI_Bcast; bench.py a torch.distributed broadcast), every rank passes it to mcq_shard_comm_rccl (ncclCommInitRank) */
int mcq_shard_unique_id(void* out /* MCQ_SHARD_UNIQUE_ID_BYTES */);
int mcq_shard_comm_rccl(mcq_shard* ctx, const void* unique_id);
int mcq_shard_set_exchange(mcq_shard* ctx, mcq_exchange_fn fn, void* user);
/* One batch (device pointers).  Default (padded mode): every block travels at a fixed size learned from the last exact
 * batch (largest count any rank saw, plus a sixteenth), its count inside it: the call only enqueues work, no host
 * round trip.  The first batch of a context, and any batch with MCQ_SHARD_EXACT, exchanges exact sizes after two
 * count exchanges through the host.  `next` (may be NULL): the batch of the following call, resident in device
 * memory and unchanged until that call -- its sketching is enqueued on a second stream now.  The exchanges and the
 * owner-side lookups run on a third stream of the context, the reduce kernels on `stream` behind them: a caller that
 * keeps calling without waiting has the next batch's exchanges and lookups under this batch's reduce kernels.
 * `out` and the statistics are complete when `stream` is (mcq_shard_sync).                                           */
int mcq_shard_query(mcq_shard* ctx, const mcq_batch* in, const mcq_query_opts* opt, mcq_result* out, void* stream,
                    uint32_t flags, const mcq_batch* next);
/* as mcq_ws_sync; MCQ_E_CAPACITY also when a block of the exchange was too small since the last sync (repeat those
 * batches with MCQ_SHARD_EXACT), or when a batch had more windows than cfg.max_bases was given for (no repeat helps:
 * create the context for larger batches).  The flags of a `next` batch's S1 are reported with THAT batch.            */
int mcq_shard_sync(mcq_shard* ctx, void* stream, mcq_stats* stats);
/* block sizes of the padded mode (features / locations per peer); setting them skips the learning batch */
int mcq_shard_set_caps(mcq_shard* ctx, uint64_t features_per_peer, uint64_t locations_per_peer);
int mcq_shard_get_caps(const mcq_shard* ctx, uint64_t* features_per_peer, uint64_t* locations_per_peer);
/* timing of the home side's reduce kernels, as mcq_ws_timing / mcq_ws_kernel_times */
int mcq_shard_timing(mcq_shard* ctx, int enable);
int mcq_shard_kernel_times(mcq_shard* ctx, double* ms /* [3] */, uint64_t* n_batches);
/* ... and of the other stages of a batch (events on the streams they run on; enabled by mcq_shard_timing): ms[0] S1 (window
 * count + sketch + route), ms[1] X1 (feature blocks to their owners), ms[2] S2 (owner-side lookup), ms[3] X2 (list ends and
 * locations back), summed over the n batches harvested so far.  The stages of consecutive batches overlap: the sum of a
 * batch's stages is more than the step time.                                                                          */
int mcq_shard_stage_times(mcq_shard* ctx, double* ms /* [4] */, uint64_t* n_batches);
/* accounting of the exchanges since the context was created: out[0] batches; bytes handed to the transport for OTHER ranks in
 * out[1] X1, out[2] X2 list ends + tile starts, out[3] X2 locations; out[4] bytes of this rank's own blocks; out[5] ranks of
 * the RCCL communicator (0 = another transport); out[6], out[7] block sizes of the padded mode (features / locations per peer) */
int mcq_shard_exchange_bytes(const mcq_shard* ctx, uint64_t* out /* [8] */);

/* ---- row f4: FASTQ ingest on the GPU ------------------------------------------------
 * text: raw FASTQ bytes in DEVICE memory (4 lines per record, as fastq_reader::read_next reads
 * them: src/sequence_io.cpp:251-285).  Writes the (begin,end) byte range of every record's
 * sequence line to seq_ranges[2*r], [2*r+1] (device, capacity 2*max_seqs) and the record count
 * to *n_seqs_out (device).  Feed mcq_query with bases = text, seq_off = seq_ranges,
 * flags = MCQ_DEVICE_PTRS | MCQ_BATCH_RANGES: the bases are read in place, never copied.  */
int mcq_fastq_index(const char* text, uint64_t n_bytes, uint64_t* seq_ranges, uint64_t max_seqs,
                    uint64_t* n_seqs_out, void* stream);
/* the same for FASTA text with every sequence on ONE line (2 lines per record: what read files in FASTA look like; the
 * reference's fasta_reader also joins sequences that span lines, src/sequence_io.cpp:122-200: such files -- genomes --
 * go through a host reader, their bases are not contiguous in the text)                                             */
int mcq_fasta_index(const char* text, uint64_t n_bytes, uint64_t* seq_ranges, uint64_t max_seqs,
                    uint64_t* n_seqs_out, void* stream);

/* ---- reading files: one chunk of read text -> a compacted batch (mcq_query_cli's input stage) -----------------------
 * text1 (and text2 for paired files; NULL: single-end): raw FASTQ or FASTA bytes in DEVICE memory, each chunk starting
 * at a record; flags MCQ_READS_EOF1 / _EOF2: the chunk ends its file.  In one call on `stream`, with no host wait:
 *   bases, seq_off   the sequences compacted as mcq_query takes them with MCQ_DEVICE_PTRS (mates of query q are
 *                    sequences 2q, 2q+1; FASTA lines joined by dropping the '\n' only, a '\r' stays as getline keeps it);
 *                    bases holds len1 + len2 bytes, seq_off 2 * max_queries + 1 entries
 *   hdr              [2q], [2q+1]: byte range in text1 of query q's header after '@' / '>' up to its first ' ' or the line end
 *   info             [MCQ_READS_INFO_WORDS] (device): queries taken, their bases, bytes of text1 / text2 used (the host
 *                    carries the rest into the next chunk), status, complete records found in text1 / text2
 * Records are taken in order while they are complete in the chunk (the next record has begun, or the file ends), n <
 * max_queries, and the bases stay <= max_bases (a first query larger than that is taken alone); with two texts n is at
 * most the smaller complete-record count.  Status MCQ_READS_NOT_STRICT: the chunk is not in the strict form -- FASTQ of
 * 4-line records (line 1 '@', line 3 '+'), or FASTA of '>' header lines and non-empty sequence lines, one format per
 * text -- and the outputs are not to be used: the host parses that chunk (mcq_reads_parse of include/mcq_host.h, the
 * same contract).  scratch: device memory of mcq_reads_scratch_bytes(len1, len2, max_queries) bytes.  Chunks < 4 GiB.
 * Still in the strict form, and read as getline reads them: a FASTQ record whose sequence and quality lines are empty and a
 * FASTA header that the next header or the end of the file follows (a query with no bases), a header with nothing after
 * '@' / '>' or with a ' ' right after it (an empty hdr range), a sequence line that is only "\r" (one base, the '\r'),
 * a text of length 0 (no query).  A FASTQ file that ends inside a record -- fewer than 4 lines, a lone '@' -- is not.
 * Flag MCQ_READS_INTERLEAVED (text2 NULL, len2 0): records 2r, 2r+1 of text1 are the mates of one query, as the reference's
 * sequence_pair_reader::next pairs the records of one file under -pairseq (src/sequence_io.cpp:442-462: two next() of the
 * same reader; the second returns an empty sequence once the file has run out).  The outputs have the paired form (mates
 * of query q are sequences 2q, 2q+1; hdr is the first mate's).  A query is complete once both its records are; a chunk
 * that ends between two mates takes neither and the cut falls in front of the first.  A last record without a mate, in
 * a chunk that ends the file, is a query whose second mate is empty.  max_queries and max_bases count pairs and the
 * bases of both mates; info[MCQ_READS_COMPLETE1] counts complete queries; info[MCQ_READS_CUT2] and _COMPLETE2 are 0.
 * The scratch is mcq_reads_scratch_bytes(len1, 0, max_queries): the record array holds one length per pair.  In this
 * mode a line that ends in '\r' (CRLF text) also makes the chunk MCQ_READS_NOT_STRICT.                             */
#ifndef MCQ_READS_CONSTANTS             /* (the same in include/mcq_host.h) */
#define MCQ_READS_CONSTANTS
enum { MCQ_READS_EOF1 = 1u, MCQ_READS_EOF2 = 2u,
       MCQ_READS_INTERLEAVED = 4u };   /* text2 NULL: records 2q, 2q+1 of text1 are the mates of query q (see above) */
enum { MCQ_READS_N = 0, MCQ_READS_BASES = 1, MCQ_READS_CUT1 = 2, MCQ_READS_CUT2 = 3, MCQ_READS_STATUS = 4,
       MCQ_READS_COMPLETE1 = 5, MCQ_READS_COMPLETE2 = 6, MCQ_READS_INFO_WORDS = 8 };
enum { MCQ_READS_NOT_STRICT = 1u };   /* info[MCQ_READS_STATUS] of the device step: parse this chunk on the host */
#endif
uint64_t mcq_reads_scratch_bytes(uint64_t len1, uint64_t len2, uint64_t max_queries);
int mcq_reads_prepare(const char* text1, uint64_t len1, const char* text2, uint64_t len2, uint32_t flags,
                      uint64_t max_queries, uint64_t max_bases, void* scratch, uint64_t scratch_bytes,
                      char* bases, uint64_t* seq_off, uint64_t* hdr, uint64_t* info, void* stream);

/* ---- row f2: building the table from reference sequences on the GPU -----------------
 * Replaces the build-side loop add_all_window_sketches (src/sketch_database.h:1079-1097) with
 * target t inserted on rank t % P (src/sketch_database.h:540-542): every window of every target is
 * sketched, and per (feature, rank) the first max_locs locations in (target, window) order are
 * kept (src/sketch_database.h:1090-1092, bucket limit 254).  The result is the union of the P rank
 * tables in the layout mcq_db_desc takes.  Target sketching uses (k, sketch_size, winlen,
 * winstride); target t = bases[seq_off[t] .. seq_off[t+1]).                                   */
typedef struct {
    uint32_t k, sketch_size, winlen, winstride;
    uint32_t n_targets;
    const char* bases;            /* host, or device with MCQ_DEVICE_PTRS                     */
    const uint64_t* seq_off;      /* [n_targets+1]                                            */
    const uint32_t* tgt2tax;      /* [n_targets]; only mcq_db_build reads it                  */
    uint32_t emulate_ranks;       /* P of the build being reproduced (0 = 1)                  */
    uint32_t max_locs;            /* per (feature, rank); 0 = 254                             */
    uint32_t n_shards, shard_id;  /* mcq_db_build: as in mcq_db_desc                          */
    uint32_t flags;               /* MCQ_DEVICE_PTRS, MCQ_BUILD_REMOVE_OVERPOPULATED; mcq_db_build: MCQ_DB_LOCS_* and the layout flags too */
    int32_t device;
} mcq_build_desc;

typedef struct mcq_table mcq_table;   /* keys / list_off / locs in device memory */

int mcq_build_table(const mcq_build_desc* desc, mcq_table** out);
/* device pointers into the table (valid until mcq_table_free); any out pointer may be NULL.
 * win_off[n_targets+1] = first global window of every target.                               */
int mcq_table_info(const mcq_table* t, uint64_t* n_keys, uint64_t* n_locs, const uint32_t** keys,
                   const uint64_t** list_off, const uint64_t** locs, const uint64_t** win_off);
int mcq_table_free(mcq_table* t);
/* One reference rank's table out of a union table built with emulate_ranks = n_ranks: rank r of the reference holds the targets
 * with tgt % n_ranks == r (src/sketch_database.h:540-542), so its table is the union table without the other targets' locations
 * and without the keys whose list becomes empty (the per-(feature, rank) limit and -remove-overpopulated-features were applied
 * by the build).  Done on the device (count per key, scans, scatter; lists keep their order); *out is a table of its own --
 * mcq_table_info gives its device arrays (win_off: the union's), mcq_table_free releases it.  A rank without targets gives an
 * empty table (n_keys = 0), not an error.  What mcq_refdb_write_shard (include/mcq_host.h) takes, one rank at a time.        */
int mcq_table_rank_split(const mcq_table* t, uint32_t n_ranks, uint32_t rank, mcq_table** out);
/* -remove-ambig-features on a table (remove_ambiguous_features, src/sketch_database.h:428-470): *out holds every key of t whose
 * list names at most max_keys (1..255) distinct values of tgt_key[target], with its list unchanged; keys and lists keep their order.
 * tgt_key[n_targets] (host, or device with MCQ_DEVICE_PTRS in flags; n_targets must be the table's) are opaque 32-bit words, as in
 * mcq_ws_set_exclusion: the target's ancestor at the rank (mcq_taxa_clade_keys / mcq_refdb_clade_keys of include/mcq_host.h;
 * 0xFFFFFFFF, "none", is a key like any other: two targets without an ancestor count once), or the target id itself for rank sequence.
 * *n_removed = keys dropped.  Done on the device (count per key -- the distinct keys of a list are kept in LDS, max_keys = 1 needs
 * none --, scans, scatter); *out is a table of its own, as after mcq_table_rank_split (win_off: the input's); it may be empty
 * (n_keys = 0), and an empty input gives an empty output.  Device memory at the peak: the input table and the output table (8 B
 * per location and 12 B per key each) plus 24 B per input key of temporaries (and 4 B per target for host keys).
 * MCQ_E_ARG: a null argument, n_targets other than the table's, max_keys outside 1..255 (text: mcq_build_last_error).            */
int mcq_table_remove_ambiguous(const mcq_table* t, const uint32_t* tgt_key /* [n_targets] */, uint32_t n_targets,
                               uint32_t max_keys /* 1..255 */, uint32_t flags /* MCQ_DEVICE_PTRS: tgt_key is on the device */,
                               mcq_table** out, uint64_t* n_removed);
/* windows of every target (the `windows` field of its sequence-level taxon, src/taxonomy.h:326-335) to host memory [n_targets] */
int mcq_table_tgt_windows(const mcq_table* t, uint32_t* out);
/* mcq_build_table + mcq_db_create in one call; the queryable handle is the only thing left in HBM */
int mcq_db_build(const mcq_build_desc* desc, mcq_db** out);
/* The build in parts, for tables whose one-piece temporaries do not fit the GPU (RefSeq scale: ~60 B per feature slot of
 * the sequences; mcq_db_build takes this way by itself then).  The features are cut into ranges of h2(feature) -- sub-ranges
 * of shard `shard_id` of `n_shards` when the table is sharded: only that shard's features are built -- and every range is
 * built on its own from the sequences (device memory only): what stays is the table in the form the query side stores, keys
 * + list lengths + 32-bit global-window words.  Same lists as mcq_build_table (per (feature, rank) limit, rank merge,
 * -remove-overpopulated-features).  The caller may release the sequences before mcq_db_from_parts makes the handle.       */
typedef struct mcq_parts mcq_parts;
int mcq_build_parts(const mcq_build_desc* desc, mcq_parts** out);
int mcq_parts_info(const mcq_parts* parts, uint64_t* n_keys, uint64_t* n_locs, uint64_t* n_windows, uint32_t* n_parts, uint64_t* bytes);
/* tgt2tax: [n_targets] host, or device with MCQ_DEVICE_PTRS in flags; flags also takes MCQ_DB_SLOTS_16 / MCQ_DB_BUCKETS_64 */
int mcq_db_from_parts(const mcq_parts* parts, const uint32_t* tgt2tax, uint32_t n_shards, uint32_t shard_id, uint32_t flags, mcq_db** out);
int mcq_parts_free(mcq_parts* parts);

/* The build in feature ranges that keeps (target, window) lists: the union table of mcq_build_table, one range of it at a time, for
 * sequences whose one-piece temporaries do not fit (what mcq_build_cli -ranges writes shard files from).  Range r holds the features
 * with (h2(feature) * n_ranges) >> 32 == r, the hash of mcq_owner and of mcq_build_parts, whose pass over the sequences this is.
 * create: device pointers only (MCQ_DEVICE_PTRS; bases and seq_off must stay valid until free; n_shards must be 0 or 1); counts the
 *   windows once; n_ranges = 0 derives the count from the free device memory (93 B per feature slot of a range against a third of
 *   it: DESIGN.md section 27).  MCQ_E_UNSUPPORTED: 2^32 - 1 windows or more, more than 2^20 ranges.
 * next: *out = the table of the next range, an ordinary mcq_table (mcq_table_free releases it): exactly the keys of mcq_build_table's
 *   table whose feature falls into the range, in ascending feature order, each with the identical list (per-(feature, rank) limit,
 *   MCQ_BUILD_REMOVE_OVERPOPULATED, (target, window) order); win_off over all targets.  mcq_table_rank_split,
 *   mcq_table_remove_ambiguous, mcq_table_shard_records, mcq_table_tgt_windows and mcq_table_info work on it unchanged.  With
 *   n_ranges = 1 the one table equals mcq_build_table's array for array.  A range without features gives an empty table.  Behind
 *   the last range *out = NULL and MCQ_OK.  Device memory of a call: 44 B per feature slot of the range plus the chunk buffers, then
 *   the table; free the table of a range before the next call unless it is known to fit beside a pass.
 * tgt_windows: windows of every target to host memory [n_targets] (known after create).                                        */
typedef struct mcq_range_build mcq_range_build;
int mcq_range_build_create(const mcq_build_desc* desc, uint32_t n_ranges /* 0 = from the free memory */, mcq_range_build** out);
int mcq_range_build_info(const mcq_range_build* b, uint32_t* n_ranges, uint32_t* next_range, uint64_t* n_windows);
int mcq_range_build_tgt_windows(const mcq_range_build* b, uint32_t* out /* host [n_targets] */);
int mcq_range_build_next(mcq_range_build* b, mcq_table** out);
int mcq_range_build_free(mcq_range_build* b);

/* One reference rank's key records of a table as the bytes of its shard file, made on the device: for every key of t that has at
 * least one location with tgt % n_ranks == rank, in t's key order, the record `u32 key, u8 n, u64 n, u32 tgt[n], u64 n, u32 win[n]`
 * (21 + 8 n bytes, little-endian, no padding; the rank's locations in list order) -- exactly what mcq_refdb_write_shard
 * (include/mcq_host.h) writes behind its two counts for mcq_table_rank_split(t, n_ranks, rank), and what mcq_shard_writer_append
 * takes.  out: device memory of cap_bytes bytes, or NULL to get the three sizes only; *n_bytes, *n_keys, *n_locs are the sizes of
 * the rank's records (set on MCQ_E_CAPACITY too).  A rank that owns no target, and an empty table, give 0 bytes.
 * MCQ_E_CAPACITY: cap_bytes < *n_bytes, nothing is written.  MCQ_E_UNSUPPORTED: a list with more than 255 locations of the rank
 * (the file's count is 8 bits; the build's limit of 254 never makes one).  MCQ_E_ARG: a null argument, rank >= n_ranks.
 * Device memory: 24 B per key of t of temporaries.                                                                            */
int mcq_table_shard_records(const mcq_table* t, uint32_t n_ranks, uint32_t rank, void* out /* device, may be NULL */,
                            uint64_t cap_bytes, uint64_t* n_bytes, uint64_t* n_keys, uint64_t* n_locs);

/* ---- parts from streamed (feature, target, window) triples: a table of any size from the REFERENCE'S OWN shard files --------
 * (row f1 at scale: sketch_database::read + hash_multimap::deserialize, src/sketch_database.h:858-952, src/hash_multimap.h:923-964,
 * without the host-side union of mcq_refdb_open -- 16 B per location and a sort on the host: 240 GB for a RefSeq build.)
 * The host library streams every shard file as chunks of triples (include/mcq_host.h: mcq_refdb_open_meta, mcq_shard_stream_*);
 * mcq_parts_builder_add takes a chunk (host pointers, or device with MCQ_DEVICE_PTRS), turns (target, window) into the global
 * window index of tgt_windows' prefix sums on the GPU and appends the (feature, word) pairs of this shard's features to the buffer
 * of their feature-hash range; mcq_parts_builder_finish sorts every range -- the merge of the reference's P per-rank lists of a
 * feature into (target, window) order -- and leaves the parts mcq_db_from_parts takes (the builder is released).  Chunks may
 * come in any order, from any number of files.  Device memory at the peak: 8 B per location of this shard + ~30 B per location
 * of one range.                                                                                                          */
typedef struct {
    uint32_t k, sketch_size, winlen, winstride;   /* what QUERIES are sketched with (the q_* fields of mcq_refdb_info)      */
    uint32_t tgt_winstride;                       /* window stride of the targets (0 = winstride)                           */
    uint32_t n_targets;
    const uint32_t* tgt_windows;                  /* host [n_targets]: mcq_refdb_tgt_windows                                */
    uint64_t expected_locations;                  /* of the WHOLE table (sum of the shard files' location counts): sizes the ranges */
    uint32_t n_ranges;                            /* 0 = from expected_locations and the free memory                        */
    uint32_t n_shards, shard_id;                  /* as in mcq_db_desc: only this shard's features are kept                 */
    int32_t device;
} mcq_parts_builder_desc;
typedef struct mcq_parts_builder mcq_parts_builder;
int mcq_parts_builder_create(const mcq_parts_builder_desc* desc, mcq_parts_builder** out);
int mcq_parts_builder_add(mcq_parts_builder* b, const uint32_t* feat, const uint32_t* tgt, const uint32_t* win, uint64_t n, uint32_t flags);
int mcq_parts_builder_finish(mcq_parts_builder* b, mcq_parts** out);
int mcq_parts_builder_free(mcq_parts_builder* b);

/* ---- the query-time bucket rules on a chunk of triples (csrc/mcq_bucket_limit.hip) ----------------------
 * `metacache_mpi query -max-locations-per-feature N [-remove-overpopulated-features]` changes every rank's table right after it is
 * read (src/mode_query.cpp:354-377): buckets of more than `remove_above` locations are cleared
 * (remove_features_with_more_locations_than, src/sketch_database.h:381-395), then buckets of more than `keep_first` locations keep
 * their first `keep_first` (max_locations_per_feature, src/sketch_database.h:356-368).  mcq_bucket_limit does that to a chunk as
 * mcq_shard_stream_next (include/mcq_host.h) hands it out -- whole key records of one shard file: a maximal run of equal `feat` is
 * one bucket of one rank; runs of any length are handled.  Removal first, then the shrink.  The triples that stay are compacted to
 * the front of the three arrays in their order, *n_out says how many (what lies behind them is unspecified); *n_shrunk and
 * *n_removed count buckets.  n = 0, or both rules 0: nothing is launched, *n_out = n, the arrays are untouched.
 * Host pointers (flags 0): the call copies in, runs, copies out and returns with the counts set.
 * Device pointers (MCQ_DEVICE_PTRS): the call only enqueues on `stream` (its scratch is stream-ordered too); the three counts are
 * copied to the caller's host words in stream order, so THE CALLER synchronises `stream` before reading them or the arrays.
 * Device memory inside the call: 12 B per triple (+ 12 B with host pointers) and a bit per triple, from the device's stream-ordered
 * pool (hipMallocAsync on `stream`); a pipeline that allocates with hipMalloc / hipFree between such calls should use
 * mcq_bucket_limit_ws below ("Whose scratch").
 * MCQ_E_ARG: a null array with n > 0, a null count, keep_first > 255.  MCQ_E_UNSUPPORTED: 2^40 triples or more.  Text: mcq_last_error. */
int mcq_bucket_limit(uint32_t* feat, uint32_t* tgt, uint32_t* win, uint64_t n,
                     uint32_t keep_first,    /* 0 = no shrink; else 1..255 */
                     uint32_t remove_above,  /* 0 = no removal; else a bucket with more than this many locations goes */
                     uint32_t flags,         /* MCQ_DEVICE_PTRS */
                     int32_t device, void* stream,
                     uint64_t* n_out, uint64_t* n_shrunk, uint64_t* n_removed);
/* The device form with the caller's scratch (device memory of at least mcq_bucket_limit_scratch_bytes(n) bytes, 256-B aligned, free
 * for the call's work on `stream`): nothing is allocated, everything is enqueued.  counts_out: three host words -- triples kept,
 * buckets shrunk, buckets removed -- copied in stream order as above.  What the streaming loader calls per chunk.  */
uint64_t mcq_bucket_limit_scratch_bytes(uint64_t n);
int mcq_bucket_limit_ws(uint32_t* feat, uint32_t* tgt, uint32_t* win, uint64_t n, uint32_t keep_first, uint32_t remove_above,
                        int32_t device, void* stream, void* scratch, uint64_t scratch_bytes, uint64_t* counts_out /* [3] */);
/* The same rules inside the streaming loader: after this call mcq_parts_builder_add applies them to every chunk on the device
 * before its own append (a chunk given as device pointers is copied first: the caller's arrays stay as they are).  This puts one
 * more requirement on the chunks: each holds whole key records of ONE shard file, as mcq_shard_stream_next hands them out (a
 * bucket cut in two by a chunk boundary, or chunks that mix files, would be judged in pieces).  Both 0 switches the rules off.
 * Without the call the builder launches and allocates nothing for them.  MCQ_E_ARG: a null builder, keep_first > 255 (text:
 * mcq_build_last_error).  mcq_parts_builder_bucket_counts: the buckets shrunk and removed over all chunks added so far.     */
int mcq_parts_builder_set_bucket_limit(mcq_parts_builder* b, uint32_t keep_first, uint32_t remove_above);
int mcq_parts_builder_bucket_counts(const mcq_parts_builder* b, uint64_t* n_shrunk, uint64_t* n_removed);

/* ---- content statistics over chunks of triples (csrc/mcq_content_stats.hip) ------------------------------
 * What `metacache_mpi info DB statistics` says about a table's buckets (print_content_properties, src/sketch_database.h:1205-1237)
 * comes from the number of buckets, their largest size and the sums of size, size^2 and size^3 (src/stat_moments.h); the handle
 * gathers these, a histogram of the sizes and the locations of every target over the chunks it is given.  A chunk is whole key records
 * of one shard file, as mcq_shard_stream_next (include/mcq_host.h) hands them out: a maximal run of equal `feat` is one bucket (runs of
 * any length are handled; equal features in two runs that do not touch are two buckets).  `win` is not read and may be null.
 * Host pointers (flags 0) are copied to a staging buffer of the handle first; device pointers (MCQ_DEVICE_PTRS) are read in place.
 * Every call works on the handle's stream (the null stream until mcq_content_stats_set_stream gives another; device arrays must be
 * ready in that stream's order) and returns after the chunk is counted: the totals are integers kept on the host, exact below 2^64
 * (254^3 times any number of buckets a machine holds).  The handle belongs to the device that was current at create; its memory is
 * plain hipMalloc memory that grows with the largest host chunk seen, nothing is allocated per chunk.
 * mcq_content_stats_add: MCQ_E_ARG for a null handle, a null feat or tgt with n > 0, and for a chunk in which a triple names a target
 *   >= n_targets -- the text (mcq_last_error) names the first such triple and its target; that chunk then counts for nothing: totals
 *   and target counts are what they were before the call.  MCQ_E_UNSUPPORTED: 2^40 triples or more.
 * mcq_content_stats_totals: the totals since create or the last reset.  mcq_content_stats_target_locations: locations per target since
 *   create.  mcq_content_stats_reset (between shards) zeroes the totals and KEEPS the target counts: a target's locations are a
 *   property of the whole database, its buckets' statistics one of each shard; a caller that wants fresh target counts makes a new
 *   handle.  mcq_content_stats_free takes a null handle.                                                                          */
typedef struct {
    uint64_t n_buckets, n_locations, sum2, sum3, max_size;
    uint64_t hist[256];         /* hist[s] = buckets of s locations; hist[255] = 255 and more; hist[0] = 0 */
} mcq_content_totals;
typedef struct mcq_content_stats mcq_content_stats;
int mcq_content_stats_create(uint32_t n_targets /* >= 1 */, mcq_content_stats** out);
int mcq_content_stats_set_stream(mcq_content_stats* h, void* stream);
int mcq_content_stats_add(mcq_content_stats* h, const uint32_t* feat, const uint32_t* tgt, const uint32_t* win, uint64_t n,
                          uint32_t flags /* MCQ_DEVICE_PTRS */);
int mcq_content_stats_totals(mcq_content_stats* h, mcq_content_totals* out);
int mcq_content_stats_target_locations(mcq_content_stats* h, uint64_t* out /* [n_targets] */);
int mcq_content_stats_reset(mcq_content_stats* h);
int mcq_content_stats_free(mcq_content_stats* h);

/* ---- extending a table: `metacache_mpi modify DB GENOMES...` (main_mode_build_modify, src/mode_build.cpp:1117-1136) ----------
 * The locations an existing database holds and the sketches of new sequences go through the pipeline of mcq_build_table together.
 * mcq_table_extend_add takes the chunks mcq_shard_stream_next (include/mcq_host.h) hands out, as host pointers or as device
 * pointers with MCQ_DEVICE_PTRS: every (feature, target, window) becomes the pipeline's pair, key = feature * n_ranks +
 * target % n_ranks, value = global window of old_tgt_windows' prefix sums, appended on the device to one buffer in the order
 * given.  Files may come in any order; the chunks of one file keep their order (a (feature, rank) group lies in one file, in one
 * key record).  mcq_table_extend_finish counts the windows of the n_new_targets new sequences and sketches them (mcq_count_windows,
 * mcq_sketch, with the descriptor's parameters: the database's), gives them the target ids n_old_targets, n_old_targets + 1, ...
 * and global windows behind the old ones, puts their pairs BEHIND the old pairs and runs the pipeline: the sort is stable, so per
 * (feature, rank) the old entries come first in their order and the first max_locs stay -- a bucket of the reference that is full
 * takes nothing (add_all_window_sketches, src/sketch_database.h:1079-1097); a max_locs below the database's own shrinks every old
 * bucket to its first max_locs entries (max_locations_per_feature, src/sketch_database.h:356-368); MCQ_BUILD_REMOVE_OVERPOPULATED
 * is applied to old and new together.  *out is a table of n_old_targets + n_new_targets targets, as from mcq_build_table of all
 * of them when the old database was built from the old ones in this order: win_off covers all targets, mcq_table_tgt_windows,
 * mcq_table_rank_split and mcq_table_remove_ambiguous work on it unchanged.  n_new_targets = 0 (bases and seq_off may be NULL)
 * gives the old table back, after the limit and the flag.  finish releases the handle when it succeeds.
 * Limits: the one-piece pipeline only (no build in parts); old + new windows below 2^32 (MCQ_E_UNSUPPORTED); the pair buffer is
 * sized once from expected_old_locations and grows by a sixteenth, by a copy, only when more arrive.  Device memory: 12 B per old
 * location while the chunks are added; in finish 12 B per pair (old locations + new feature slots) twice while the old pairs are
 * copied in front of the new ones, then the pipeline's ~44 B per pair at its peak.
 * MCQ_E_ARG: a null argument, no rank, a triple that names a target or a window the descriptor does not have, an empty feature
 * (0xFFFFFFFF); text in mcq_build_last_error.                                                                               */
typedef struct {
    uint32_t k, sketch_size, winlen, winstride;   /* the database's target sketcher                                         */
    uint32_t n_ranks;                             /* P of the database (0 = 1)                                              */
    uint32_t max_locs;                            /* per (feature, rank); 0 = 254                                           */
    uint32_t flags;                               /* MCQ_BUILD_REMOVE_OVERPOPULATED                                         */
    int32_t device;
    uint32_t n_old_targets;
    const uint32_t* old_tgt_windows;              /* host [n_old_targets]: mcq_refdb_tgt_windows                            */
    uint64_t expected_old_locations;              /* sum of the shard files' location counts: sizes the pair buffer once    */
} mcq_table_extend_desc;
typedef struct mcq_table_extend mcq_table_extend;
int mcq_table_extend_create(const mcq_table_extend_desc* desc, mcq_table_extend** out);
int mcq_table_extend_add(mcq_table_extend* x, const uint32_t* feat, const uint32_t* tgt, const uint32_t* win, uint64_t n, uint32_t flags);
int mcq_table_extend_finish(mcq_table_extend* x, const char* bases, const uint64_t* seq_off /* [n_new_targets + 1] */,
                            uint32_t n_new_targets, uint32_t flags /* MCQ_DEVICE_PTRS: bases and seq_off are on the device */,
                            mcq_table** out);
int mcq_table_extend_free(mcq_table_extend* x);
const char* mcq_build_last_error(void);

/* ---- classification and per-taxon read counts on the device (csrc/mcq_classify.hip) ------------------------------------
 * classify() (src/classification.cpp:235-265, ranked_lca src/taxonomy.h:531-537) of every query's candidate list, as
 * mcq_refdb_classify of include/mcq_host.h computes it, bit for bit, and the count of classified queries per taxon the
 * reference keeps for its abundance tables (++taxCounts[cls.best], src/classification.cpp:712-714).
 * A taxonomy is the ranked-lineage table of the database (mcq_refdb_lineages): lineage[t * 21 + r] = taxon index at rank r
 * in the lineage of taxon t or 0xFFFFFFFF, rank[t] = rank of taxon t (host pointers; copied to `device`).             */
typedef struct mcq_taxonomy mcq_taxonomy;
typedef struct {
    uint32_t hits_min;            /* -hitmin (already defaulted: mcq_default_hits_min)                             */
    float hits_diff_fraction;     /* -hitdiff as the reference stores it (80 -> 0.8f)                              */
    uint32_t highest_rank;        /* -highest (MCQ_RANK_* of include/mcq_host.h)                                   */
    uint32_t flags;               /* 0                                                                             */
} mcq_classify_opts;
int mcq_taxonomy_create(const uint32_t* lineage, const uint8_t* rank, uint32_t n_taxa, int32_t device, mcq_taxonomy** out);
int mcq_taxonomy_destroy(mcq_taxonomy* tx);
/* cands: the device result of mcq_query / mcq_shard_query (flags MCQ_DEVICE_PTRS), n_queries lists of max_cand slots.
 * best (device, may be NULL): per query the taxon index of the classification or 0xFFFFFFFF.  counts (device, may be
 * NULL): [n_taxa + 1] u64, ADDED to: counts[t] += queries classified as taxon t, counts[n_taxa] += unclassified ones.
 * Only enqueues work on `stream`.  Integer counts: the sums do not depend on the order of the adds.                 */
int mcq_classify(const mcq_taxonomy* tx, const mcq_result* cands, uint64_t n_queries, uint32_t max_cand,
                 const mcq_classify_opts* opts, uint32_t* best, uint64_t* counts, void* stream);
/* While a taxonomy is attached (tx != NULL; NULL detaches), every mcq_query / mcq_query_pipelined on the workspace also
 * classifies its batch on the device -- on the batch's stream, before the copy-out -- and adds into the workspace's
 * counts ([n_taxa + 1], zeroed when first attached or attached with another n_taxa).  The taxonomy must outlive the
 * attachment and live on the workspace's device.                                                                     */
int mcq_ws_set_classify(mcq_ws* ws, const mcq_taxonomy* tx, const mcq_classify_opts* opts);
/* waits for the last batch that classified, copies the workspace's counts ([n_taxa + 1] of the taxonomy attached last)
 * to host_out; reset != 0 zeroes them afterwards                                                                      */
int mcq_ws_taxon_counts(mcq_ws* ws, uint64_t* host_out, int reset);

/* ---- clade exclusion: the reference's `-exclude RANK` (prepare_evaluation / remove_hits_on_rank, src/classification.cpp:141-183) ----
 * For a read with a ground truth the reference drops, before the candidates are made, every match on a target whose ancestor
 * at RANK equals the ancestor at RANK of the read's truth.  Either ancestor may be missing, and missing equals missing: a truth
 * above RANK removes the targets that have no ancestor at RANK.  A match goes because of its target alone, so the engine takes
 * the two ancestors as opaque 32-bit keys (mcq_refdb_clade_keys / mcq_refdb_taxon_clade of include/mcq_host.h make them):
 *   tgt_clade[t]    key of target t's ancestor at RANK, MCQ_CLADE_NONE if it has none
 *   query_clade[q]  key of the truth's ancestor at RANK, MCQ_CLADE_NONE if it has none, MCQ_CLADE_KEEP_ALL for a read without
 *                   a ground truth: nothing is excluded for it
 * and retires the excluded targets' candidates before the top lists are built: the same lists as from the match list without
 * those targets' locations (tests/test_gpu_exclusion.py).
 * mcq_ws_set_exclusion attaches the table (copied; host pointer, or device with MCQ_DEVICE_PTRS) to a workspace, NULL detaches;
 * it waits for the device.  While a table is attached, every mcq_query / mcq_query_pipelined on the workspace needs the keys
 * of its batch: mcq_ws_set_query_clades hands them over for the NEXT such call, which consumes them (none handed over, or
 * another count than the batch's queries: MCQ_E_ARG).  A host array is copied by the call; a device array (MCQ_DEVICE_PTRS) is
 * read by that batch's kernels and stays untouched until they are done.  Two pipelined batches in flight each keep their own.
 * Queries under exclusion take the full first wave stage, the second one and the plain workgroup kernel (never the lean stage:
 * MCQ_FORCE_LEAN_WAVE gives MCQ_E_UNSUPPORTED; never the two-class tail, which proves its cut from targets it would then lose).
 * A workspace without a table behaves as ever.  mcq_reduce and mcq_shard_query do not look at it.
 * Not checked: a table given as a device array is not searched for MCQ_CLADE_KEEP_ALL (a host table holding it is MCQ_E_ARG); a
 * target that carried it would be dropped for every read without a truth, so the caller keeps it out.
 * The keys are consumed when the query call takes them, before its kernels are planned: a call that then fails (MCQ_E_UNSUPPORTED
 * of MCQ_FORCE_LEAN_WAVE, a HIP error) has used them up, and the keys are handed over again for the next attempt.  In
 * mcq_query_pipelined such a failure comes after the batch's input copies are queued; they are harmless, the staging set is
 * written again by the next call.  MCQ_QUIRK_SEQ_DROP works as ever: it acts where the emulated ranks' lists are merged, after
 * the excluded targets are gone (tests/test_gpu_exclusion_device.py).                                                      */
static const uint32_t MCQ_CLADE_NONE = 0xFFFFFFFFu;       /* no ancestor at RANK (a target's, or a truth's)      */
static const uint32_t MCQ_CLADE_KEEP_ALL = 0xFFFFFFFEu;   /* query_clade only: no ground truth, exclude nothing */
int mcq_ws_set_exclusion(mcq_ws* ws, const uint32_t* tgt_clade, uint32_t n_targets, uint32_t flags);
int mcq_ws_set_query_clades(mcq_ws* ws, const uint32_t* query_clade, uint64_t n_queries, uint32_t flags);

/* ---- per-target window hit lists: what `-hits-per-seq` prints (csrc/mcq_target_hits.hip) ---------------------------------------
 * matches_per_target::insert (src/matches_per_target.h:111-155) keeps, for a candidate of a read, the windows of the candidate's
 * range with the number of the read's matches on each.  mcq_query gives out no window of a target (after a fold not even the
 * range), so mcq_target_hits works a batch through rows 1-7 once more and keeps only the locations of the targets the caller names:
 *   targets     device, [n_queries * n_slots], n_slots 1..MCQ_TARGET_HITS_MAX_SLOTS; MCQ_TARGET_UNUSED = the slot is unused.  The
 *               targets of a query should differ; a target named twice is answered twice.
 *   out_ranges  device, [n_queries * n_slots]: the read's per-target candidate on that target (for_all_contiguous_window_ranges,
 *               src/candidates.h:118-180: the first strictly best contiguous range of at most numWindows = 2 + max(len1 + len2,
 *               insert_size_max) / target stride windows among all windows of the target the read hits).  n_win = hits = 0 when the
 *               read has no location on the target, when the target does not exist, and for an unused slot (tgt is copied).
 *   out_counts  device, [n_queries * n_slots * range_cap]: counts[i] = the read's matches on (tgt, win_beg + i) for i < n_win, 0 for a
 *               window of the range without a match.  The words from n_win on are left as the caller set them.
 *   status      device, [n_queries]: 0, or MCQ_TARGET_HITS_* bits of a query that exceeded a capacity.  Such a query gets n_win = 0
 *               in ALL its slots and is counted like a query that overflowed the workspace: the next mcq_ws_sync(ws) returns
 *               MCQ_E_CAPACITY.  Nothing is answered wrongly in silence.
 * The capacities: the range width numWindows of the query exceeds range_cap (mcq_target_hits_range_cap gives the width of the
 * longest query of a batch: pass that); the query has more than MCQ_TARGET_HITS_MAX_KEYS distinct (target, window) pairs on its slot
 * targets; a window id inside a target of 2^28 or more, or a sequence of 2^31 bases or more.
 * Batches as mcq_query takes them (ASCII or MCQ_BATCH_PACKED, offsets or MCQ_BATCH_RANGES, paired or not) but device pointers only
 * (MCQ_DEVICE_PTRS); every location form and bucket layout; any sketch geometry the handle accepts.  The call only enqueues work on
 * `stream`.  It does not touch the counters mcq_ws_sync reports except the capacity count.
 * THE CAPACITY COUNT IS THE WORKSPACE'S AND IT STAYS: this call adds to it and never zeroes it (a query enqueued in front of it on
 * the same stream may have counted too, and that must not be lost); only the next mcq_query / mcq_reduce on the workspace zeroes
 * it.  So after one reported query EVERY later mcq_ws_sync on the workspace returns MCQ_E_CAPACITY -- also behind later
 * mcq_target_hits calls whose queries were all answered -- until a query call has run; and a sync that comes after that query call
 * no longer reports it.  A caller that uses this entry point without mcq_query reads status[] (which is exact per call and per
 * query) and treats the sync's code as "some call since the last query reported one".  The text of that error speaks of the
 * workspace's per-query capacity; here it means the capacities above.  A workspace under clade exclusion (mcq_ws_set_exclusion) is not looked at: excluded
 * targets never become candidates, so a caller that names candidates' targets never names one.                                     */
#define MCQ_TARGET_HITS_MAX_SLOTS 16u
#define MCQ_TARGET_HITS_MAX_KEYS 1024u   /* distinct (target, window) pairs of one query over all its slot targets */
#define MCQ_TARGET_UNUSED 0xFFFFFFFFu
enum { MCQ_TARGET_HITS_RANGE = 1u,      /* status: the query's range width exceeds range_cap                          */
       MCQ_TARGET_HITS_KEYS = 2u,       /* ... more than MCQ_TARGET_HITS_MAX_KEYS distinct (target, window) pairs      */
       MCQ_TARGET_HITS_WINDOW = 4u };   /* ... a window id >= 2^28 inside a slot target, or a sequence of >= 2^31 bases */
typedef struct {
    uint32_t tgt;
    uint32_t hits;              /* matches inside the range (match_candidate::hits)  */
    uint32_t win_beg;           /* first window of the range                          */
    uint32_t n_win;             /* its width: win_end = win_beg + n_win - 1; 0 = none */
} mcq_target_range;
/* range width of a query of `longest_query` bases (both mates) = the range_cap a batch whose longest query that is needs */
uint32_t mcq_target_hits_range_cap(const mcq_db* db, uint64_t longest_query, uint64_t insert_size_max);
int mcq_target_hits(const mcq_db* db, mcq_ws* ws, const mcq_batch* in, const uint32_t* targets, uint32_t n_slots,
                    uint64_t insert_size_max, uint32_t range_cap, mcq_target_range* out_ranges, uint32_t* out_counts,
                    uint32_t* status, void* stream);
/* The slot targets of a batch from its device results (mcq_query's `out` with MCQ_DEVICE_PTRS): per query the targets of its
 * sequence-level candidates (key bit 31) with hits >= hits_min, in list order, the other slots MCQ_TARGET_UNUSED -- the candidates
 * matches_per_target::insert takes.  tax2tgt (device, [n_taxa]): target id of taxon index (key & 0x7FFFFFFF), MCQ_TARGET_UNUSED for
 * a taxon that is no target (mcq_refdb_tax2tgt of include/mcq_host.h makes it).  Only enqueues work on `stream`.                  */
int mcq_target_slots(const mcq_result* cands, uint64_t n_queries, uint32_t max_cand, uint32_t hits_min,
                     const uint32_t* tax2tgt, uint32_t n_taxa, uint32_t* targets, uint32_t n_slots, void* stream);

/* ---- read-to-candidate alignment: what `-align` prints (csrc/mcq_align.hip) ------------------------------------------------------
 * make_semi_global_alignment (src/classification.cpp:77-103) of every query of a batch against one subject each: align_semi_global
 * with default_alignment_scheme (src/alignment.h: match +2, mismatch -1, gap -1; row 0 and column 0 are 0 and end the backtrace; a
 * cell takes diag, then above if strictly greater, then left if strictly greater; the end cell is the corner, then the last column at
 * rows 1 .. len_q-1, then the last row at columns 1 .. len_s-1, each only if strictly greater).  Mate 1 is aligned forward and as its
 * reverse complement (reverse_complement, src/dna_encoding.h:146-165: only ACGTacgt change); a second mate that is not empty adds its
 * two scores to the two sums, which are std::size_t there: a negative sum compares as a huge number, and so it does here.  Forward
 * wins only if strictly greater.  What comes back is mate 1's chosen alignment: its score, the orientation, and the two aligned
 * strings in reading order ('_' = gap).  Characters are compared raw: case matters, N equals N.  An empty mate 1 or an empty subject
 * gives score 0 and the one pair '_' / '_'.
 *   in          a batch as mcq_query takes it, device pointers only (MCQ_DEVICE_PTRS), ASCII, offsets or MCQ_BATCH_RANGES, paired or
 *               not.  MCQ_BATCH_PACKED has lost the case of the bases: MCQ_E_UNSUPPORTED.
 *   subjects    device, raw bases; jobs[q] (device, [n_queries]) names query q's slice of it.  on = 0: no alignment for this query.
 *   out         device, [n_queries].  length = bytes of each of the two strings, 0 for a query without `on` and for one beyond a capacity.
 *   out_query, out_subject   device, [n_queries * text_cap]: query q's strings start at q * text_cap.  Only [0, length) is written.
 * The capacities: a mate of more than max_query bases gets MCQ_ALIGN_QUERY_LONG in its status, a subject of more than max_subject bases
 * MCQ_ALIGN_SUBJECT_LONG; such a query gets length 0 and nothing is written into its text slots.  max_query <= MCQ_ALIGN_MAX_QUERY and
 * max_subject <= MCQ_ALIGN_MAX_SUBJECT are the caller's bounds for this call (MCQ_E_ARG beyond), text_cap >= max_query + max_subject and
 * >= 1.  Jobs whose predecessor matrix (2 bits per cell) does not fit a wave's share of LDS keep it in scratch memory of the workspace:
 * 256 MiB, made once by the first call whose bounds allow such a job (that one call allocates; every other call only enqueues work on
 * `stream`); a call that needs it runs with as many waves as areas of max_query x max_subject cells fit into it.  The
 * workspace's counters and its capacity count are not touched: status[] is the only report.                                        */
enum { MCQ_ALIGN_MAX_QUERY = 2048u,      /* bases of one mate                                                    */
       MCQ_ALIGN_MAX_SUBJECT = 4096u };  /* bases of one subject                                                 */
enum { MCQ_ALIGN_QUERY_LONG = 1u,        /* status: a mate has more than max_query bases                         */
       MCQ_ALIGN_SUBJECT_LONG = 2u };    /* ... the subject has more than max_subject bases                      */
typedef struct {
    uint64_t sub_off;           /* first base of the subject in `subjects`                 */
    uint32_t sub_len;
    uint32_t on;                /* 0: no alignment for this query                          */
} mcq_align_job;
typedef struct {
    int32_t score;              /* of mate 1's chosen alignment                            */
    uint32_t length;            /* aligned length L: bytes of each string                  */
    uint32_t reverse;           /* 1: the reverse complement of mate 1 was chosen          */
    uint32_t status;            /* 0 or MCQ_ALIGN_* bits                                    */
} mcq_alignment;
int mcq_align(mcq_ws* ws, const mcq_batch* in, const char* subjects, const mcq_align_job* jobs,
              uint32_t max_query, uint32_t max_subject, mcq_alignment* out,
              char* out_query, char* out_subject, uint32_t text_cap, void* stream);

/* ---- all hits of a read: what `-allhits` prints (csrc/mcq_all_hits.hip) ------------------------------------------------------------
 * A read's sorted match list (what merge_sort returns, src/querying.h:88-106) run-length compressed: one mcq_hit per distinct
 * (target, window) the read hits, in ascending (tgt, win) order, `hits` = how many of the read's locations lie there.  Two calls:
 *   mcq_all_hits_count  sketches and probes every query and leaves in loc_off (device, [n_queries + 1]) the exclusive prefix sums of
 *               the queries' location counts (the sums of the probed list lengths); loc_off[n_queries] is the total.  A query's
 *               location count bounds the number of its entries and is the size of its segment of `hits`.  A query with a sequence
 *               of 2^31 bases or more counts as 0.
 *   mcq_all_hits  writes query q's entries to hits[loc_off[q] .. loc_off[q] + n_hits[q]); their `hits` fields sum to
 *               loc_off[q + 1] - loc_off[q].  hits: device, [cap], 4-byte aligned; n_hits, status: device, [n_queries].
 * mcq_all_hits never writes outside a query's segment nor at `cap` and beyond.  The part of a segment behind the query's entries
 * is working space: what it holds afterwards is undefined.  A query whose status is not 0 gets n_hits = 0 and nothing is written
 * into its segment: MCQ_ALL_HITS_LOCS -- it has more locations than the workspace's max_locs_per_query, or a sequence of 2^31
 * bases or more; MCQ_ALL_HITS_SEGMENT -- its segment in loc_off is not its location count (or loc_off decreases there), or the segment
 * of a query that has locations ends beyond cap.  So a loc_off that mcq_all_hits_count made for this batch on this table and a
 * cap >= loc_off[n_queries] leave only MCQ_ALL_HITS_LOCS to happen.  Nothing is answered wrongly in silence.
 * The kernel tiers by segment size: up to MCQ_ALL_HITS_REG_MAX locations one wavefront sorts in registers, up to
 * MCQ_ALL_HITS_WAVE_MAX one wavefront sorts in LDS, beyond that a workgroup sorts inside the query's own segment.
 * Batches as mcq_target_hits takes them (ASCII or MCQ_BATCH_PACKED, offsets or MCQ_BATCH_RANGES, paired or not; device pointers
 * only: a host batch is MCQ_E_ARG); every location form and bucket layout; any sketch geometry the handle accepts.  Both calls only
 * enqueue work on `stream`.  status[] is the only report: the workspace's counters and its capacity count are not touched.  A
 * workspace under clade exclusion (mcq_ws_set_exclusion) is not looked at: the caller drops the entries of excluded targets.      */
#define MCQ_ALL_HITS_REG_MAX 64u         /* locations of a query sorted in registers                       */
#define MCQ_ALL_HITS_WAVE_MAX 2048u      /* ... sorted in LDS by one wavefront; more: the workgroup tier  */
typedef struct { uint32_t tgt, win, hits; } mcq_hit;                 /* 12 bytes, no padding */
enum { MCQ_ALL_HITS_LOCS = 1u,      /* status: more locations than the workspace's max_locs_per_query, or >= 2^31 bases */
       MCQ_ALL_HITS_SEGMENT = 2u }; /* ... the query's segment in loc_off is not its location count, or ends beyond cap */
int mcq_all_hits_count(const mcq_db* db, mcq_ws* ws, const mcq_batch* in, uint64_t* loc_off /* device [nq+1] */, void* stream);
int mcq_all_hits(const mcq_db* db, mcq_ws* ws, const mcq_batch* in, const uint64_t* loc_off, mcq_hit* hits /* device [cap] */,
                 uint64_t cap, uint32_t* n_hits /* device [nq] */, uint32_t* status /* device [nq] */, void* stream);

/* ---- breadth of coverage per reference sequence: what `-coverage` prints and `-cov-percentile` cuts by (csrc/mcq_coverage.hip) ------
 * A handle on one device that adds up, over all batches of a run, what mcq_target_hits answers: one bit per (target, window) -- set once
 * some query had a match there --, and per target a `queries` and a `hits` counter (u64).  A target's segment of the bitmap starts on a
 * 32-bit word: word_off[t + 1] = word_off[t] + ceil(windows[t] / 32).  Device memory: 4 B per 32 windows and 40 B per target.
 *   create   windows (host, [n_targets], n_targets >= 1): windows of every target (mcq_refdb_tgt_windows); a target may have none.
 *   add      ranges, counts: DEVICE, mcq_target_hits' out_ranges / out_counts as they are ([n_queries * n_slots] and
 *            [n_queries * n_slots * range_cap]; ranges 16-byte aligned).  For every (query, slot) with tgt != MCQ_TARGET_UNUSED and
 *            n_win > 0: window win_beg + i of tgt gets its bit for every i < n_win with counts[i] > 0 (a window of the range with count
 *            0 gets none), queries[tgt] += 1, hits[tgt] += the sum of those counts (the `hits` field of the range is not read).  The
 *            words of counts from n_win on are never read.  A slot with tgt >= n_targets, with win_beg + n_win > windows[tgt], or with
 *            n_win > range_cap is skipped as a whole and counted in out_of_range: the kernel checks this, nothing outside the target's
 *            segment is touched.  Only enqueues work on `stream`.
 *   read     one kernel counts the set bits of every segment, then host_out[t] = {hits, queries, windows_covered} of every target and
 *            *out_of_range (may be NULL) are copied out; waits for `stream`.  All sums are integers: they do not depend on the order
 *            of the adds, nor on how an input was cut into batches.
 *   reset    everything back to zero; only enqueues work on `stream`.
 *   bitmap   for tests: the bitmap as it is, mcq_coverage_bitmap_words() words -- one guard word, the segments, one guard word; the
 *            guards are never addressed and stay 0 -- and (may be NULL) word_off[n_targets + 1], counted from the first segment.  Waits. */
#ifndef MCQ_TARGET_COVERAGE_DEFINED
#define MCQ_TARGET_COVERAGE_DEFINED
typedef struct {
    uint64_t hits;              /* matches of all entries on the target                                     */
    uint64_t queries;           /* (query, slot) entries on the target: reads that had it as a candidate   */
    uint32_t windows_covered;   /* windows of the target with at least one match                           */
    uint32_t reserved;          /* 0                                                                        */
} mcq_target_coverage;
#endif
typedef struct mcq_coverage mcq_coverage;
int mcq_coverage_create(const uint32_t* windows /* host [n_targets] */, uint32_t n_targets, int32_t device, mcq_coverage** out);
int mcq_coverage_add(mcq_coverage* cov, const mcq_target_range* ranges, const uint32_t* counts, uint64_t n_queries, uint32_t n_slots,
                     uint32_t range_cap, void* stream);
int mcq_coverage_read(mcq_coverage* cov, mcq_target_coverage* host_out /* [n_targets] */, uint64_t* out_of_range, void* stream);
int mcq_coverage_reset(mcq_coverage* cov, void* stream);
uint64_t mcq_coverage_bitmap_words(const mcq_coverage* cov);
int mcq_coverage_bitmap(mcq_coverage* cov, uint32_t* host_words, uint64_t* host_word_off, void* stream);
int mcq_coverage_free(mcq_coverage* cov);

/* ---- *.accession2taxid text joined against the names of a database's targets (the post-mapping of a build) -----------
 * What rank_targets_with_mapping_file (src/mode_build.cpp:248-312) does for the targets without a parent, on text of the strict
 * form.  A line `acc TAB accver TAB taxid TAB gi` names one target at most, a function of the line alone: the target named
 * exactly accver; if there is none, the first name strictly greater than acc in byte order if it begins with acc
 * (taxon_with_similar_name, src/sketch_database.h:631-639; a name equal to acc is not found this way); if there is none, the
 * target named exactly gi.  If that target is unranked it takes the taxid of the FIRST line that names it, in the order (file
 * ordinal, line number); a taxid of 0 counts.  A line whose target is ranked does nothing (no falling through to acc or gi).
 * create   names_blob + name_off[n_names + 1]: the sequence-level names of the database back to back, strictly ascending as
 *          std::string compares (unsigned bytes, then length: MCQ_E_ARG otherwise); name_target[k] < n_targets: the target of
 *          name k; unranked[t] != 0: target t has no parent.  Host arrays, copied to `device` by the call.
 * chunk    text: whole lines of ONE file in DEVICE memory (16-B aligned text is read with 16-B loads, any other byte by byte),
 *          n_bytes < 2^32; file_ordinal < 2^23 orders the files, first_line_no (< 2^40) is the number of the chunk's first line
 *          in its file; line i of the chunk has the number first_line_no + i.  Any numbering under which a later line has the
 *          greater number will do, such as the chunk's byte offset in its file (a strict line has at least 8 bytes).
 *          The chunk is STRICT when every line has four non-empty fields of non-blank bytes (none of space, TAB,
 *          LF, VT, FF, CR) split by single TABs, ends in LF (one CR before it is allowed and no part of the fourth field), has
 *          1-19 decimal digits as its third field, and is at most MCQ_ACCMAP_MAX_LINE bytes long with its LF -- then a
 *          token-stream parser sees the same records.  *strict (host) = 1: the chunk is applied when the call returns;
 *          0: it is not strict, and NOTHING in the handle has changed (the caller parses it on the host: mcq_accmap_host of
 *          include/mcq_host.h).  The call waits for `stream`.  Chunks may come in any order: the result depends on their
 *          ordinals and line numbers only.
 * finish   found[t] = 1 and parent[t] = the taxid (the uint64 read, as int64) where a line won target t; 0 and 0 elsewhere.
 *          The handle stays usable.                                                                                        */
#define MCQ_ACCMAP_MAX_LINE 1024
typedef struct mcq_accmap mcq_accmap;
/* The rule by which a strict line names a name.  _TARGETS: the three lookups above (mcq_accmap_create).  _ACC, _ACCVER, _GI: the
 * name that EQUALS the line's first, second or fourth field and nothing else -- no similar-name search, no falling through to
 * another column: the join of the reference's `annotate` (src/mode_annotate.cpp:181-229: one std::map keyed by the chosen column,
 * the first entry of a key stays).  Everything else -- the strict form, unranked[], the first line in (file ordinal, line number)
 * order, a taxid of 0, chunk / finish / free -- is the same under every rule.  An annotate-style caller passes the distinct ids as
 * names, target k = name k, and unranked all 1.                                                                              */
enum { MCQ_ACCMAP_RULE_TARGETS = 0, MCQ_ACCMAP_RULE_ACC = 1, MCQ_ACCMAP_RULE_ACCVER = 2, MCQ_ACCMAP_RULE_GI = 3 };
int mcq_accmap_create_rule(const char* names_blob, const uint64_t* name_off, uint64_t n_names, const uint32_t* name_target,
                           const uint8_t* unranked, uint32_t n_targets, uint32_t rule, int device, mcq_accmap** out);
int mcq_accmap_create(const char* names_blob, const uint64_t* name_off, uint64_t n_names, const uint32_t* name_target,
                      const uint8_t* unranked, uint32_t n_targets, int device, mcq_accmap** out);
int mcq_accmap_chunk(mcq_accmap* h, const char* text, uint64_t n_bytes, uint32_t file_ordinal, uint64_t first_line_no,
                     uint32_t* strict, void* stream);
int mcq_accmap_finish(mcq_accmap* h, int64_t* parent /* host [n_targets] */, uint8_t* found /* host [n_targets] */);
int mcq_accmap_free(mcq_accmap* h);

/* ---- merging query result files: the reference's `merge` mode (csrc/mcq_merge.hip) --------------------------------------
 * What read_results (src/mode_merge.cpp:209-264) does with every mapping line of files written with `-tophits -queryids`, and
 * classify() of the merged lists.  The handle owns per query a candidate list -- a count and max_cand (taxon index, hits) pairs --
 * the reference of its header token (file ordinal, byte offset in the file, length; the first line that brings one sets it) and
 * a count of the items whose taxid the taxonomy does not have (the reference prints `taxid not found` per item).  Every item of a
 * line goes through best_distinct_matches_in_contiguous_window_ranges::insert (src/candidates.h:236-285) on the list of the line's
 * query, in item order: the taxon becomes its ancestor at merge_below_rank if it has one (0: never); a taxon in the list takes
 * more hits and moves ahead of smaller entries, behind equal ones; a new taxon goes in behind equal hits, unless that is the end
 * of a full list.  The insert depends on order: chunks of a file in file order and files in merge order, all on ONE stream.
 * create   tx: the ranked lineages (mcq_taxonomy_create), which must outlive the handle; taxid_sorted / taxid_taxon [n_ids]: the
 *          taxon ids strictly ascending with their taxon indices (host arrays, copied); max_cand 1..16.
 * chunk    text: whole lines of ONE file in DEVICE memory (16-B aligned text is read with 16-B loads), n_bytes < 2^32;
 *          chunk_offset: the byte of the file the chunk begins at (header references); tophits_column >= 2: the number of `|` in
 *          front of the top_hits column.  The chunk is STRICT when every line begins with '#' (skipped), or is: 1-18 digits, the
 *          query id in 1 .. n_queries; `\t|\t`; the header column, beginning with a non-empty token (up to the first blank); the
 *          further columns, each ended by `\t|\t`, and no '|' anywhere else in front of the top_hits column; the top_hits column,
 *          empty or `taxid:hits` items (taxid 1-18 digits, hits 1-9 digits) split by single ',', at most MCQ_MERGE_MAX_ITEMS; a
 *          TAB.  What follows that TAB is not looked at.  A line is at most MCQ_MERGE_MAX_LINE bytes with its LF (the chunk's last
 *          line may lack the LF); no id occurs twice in the chunk; there is no empty line.  *strict (host) = 1: the chunk is
 *          applied when the call returns; 0: it is not strict and NOTHING in the handle has changed (the caller parses it on the
 *          host and hands the lines to mcq_merge_lines).  The call waits for `stream`.
 * lines    lines that are parsed already (host arrays): line l names query line_query[l] (0-based: id - 1) and holds the items
 *          [item_off[l], item_off[l + 1]) of taxid / hits, and its header token at header_off[l] of file file_ordinal, header_len[l]
 *          bytes (0: none).  One call holds a query at most once (MCQ_E_ARG otherwise, and nothing is applied): a caller with a
 *          repeated id cuts the call there.  The same apply kernel as chunk.  The call waits for `stream`.
 * finish   classifies the lists as mcq_classify does candidates: best (device [n_queries], may be NULL), counts (device
 *          [n_taxa + 1], may be NULL, ADDED to).  Only enqueues work on `stream`.  The handle stays usable.
 * lists / headers   copy out to host arrays (any may be NULL): n_cand [n_queries], pairs [n_queries * max_cand * 2] (taxon index,
 *          hits; the slots behind n_cand hold what earlier inserts left), *n_unknown; file / offset / length [n_queries] (length 0:
 *          no header seen).  They wait for the device.                                                                          */
#define MCQ_MERGE_MAX_LINE 4096
#define MCQ_MERGE_MAX_ITEMS 64
typedef struct mcq_merge mcq_merge;
int mcq_merge_create(const mcq_taxonomy* tx, const int64_t* taxid_sorted, const uint32_t* taxid_taxon, uint64_t n_ids,
                     uint64_t n_queries, uint32_t max_cand, uint32_t merge_below_rank, int device, mcq_merge** out);
int mcq_merge_chunk(mcq_merge* h, const char* text, uint64_t n_bytes, uint32_t file_ordinal, uint64_t chunk_offset,
                    uint32_t tophits_column, int32_t* strict, void* stream);
int mcq_merge_lines(mcq_merge* h, const uint32_t* line_query, const uint64_t* item_off /* [n_lines + 1] */, const int64_t* taxid,
                    const uint32_t* hits, const uint64_t* header_off, const uint32_t* header_len, uint64_t n_lines,
                    uint32_t file_ordinal, uint32_t flags /* 0 */, void* stream);
int mcq_merge_finish(mcq_merge* h, const mcq_classify_opts* opts, uint32_t* best, uint64_t* counts, void* stream);
int mcq_merge_lists(mcq_merge* h, uint32_t* n_cand, uint32_t* pairs, uint64_t* n_unknown);
int mcq_merge_headers(mcq_merge* h, uint32_t* file, uint64_t* offset, uint32_t* length);
int mcq_merge_free(mcq_merge* h);

/* ---- debug / parity taps ------------------------------------------------------------
 * Row 5 in isolation is mcq_count_windows + mcq_sketch above (the sketches of every window).
 * Rows 7-8 in isolation: the sorted match list of every query (what merge_sort returns,
 * src/querying.h:88-106): match_off[q..q+1) into matches (capacity cap; pass matches = NULL first to
 * learn the sizes).  path_flags = 0 taps every query on the path it takes in mcq_query (first or second
 * wave stage, workgroup kernel); MCQ_FORCE_BLOCK_PATH / MCQ_FORCE_RAW_SORT / MCQ_NO_WAVE16 tap the path
 * those hooks select.  The taps live in separate instantiations of the kernels.  The batch is a plain
 * ASCII host batch, held to the rules of mcq_query's host batches: seq_off[0] must be 0 (MCQ_E_ARG
 * otherwise), and a packed or ranges batch is refused before anything is copied.                    */
int mcq_debug_matches(const mcq_db* db, mcq_ws* ws, const mcq_batch* in, uint32_t path_flags,
                      uint64_t* match_off /* host [n_queries+1] */, uint64_t* matches /* host */, uint64_t cap);

/* diagnostic builds only (-DMCQ_PHASE_CLOCK): shader clocks per phase of the workgroup kernel of the last synchronised call */
int mcq_debug_phase_clocks(mcq_ws* ws, uint64_t* out /* [22] */);

const char* mcq_last_error(void);
const char* mcq_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MCQ_H */
