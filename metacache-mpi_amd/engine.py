"""ctypes mirror of include/mcq.h.  Names and argument meaning follow the header.

Device buffers are passed as raw pointers (e.g. torch.Tensor.data_ptr()); host
buffers as numpy arrays.  The HIP library is mandatory: there is no fallback.
"""
import ctypes as C
import os

import numpy as np

from .build import lib_path

MCQ_DEVICE_PTRS = 1
MCQ_QUIRK_SEQ_DROP = 2
MCQ_FOLD_BY_LISTS = 0x8000
MCQ_BATCH_RANGES = 8             # seq_off = (begin,end) pairs into `bases` (device pointers only)
MCQ_BATCH_PACKED = 0x10          # bases in the packed form of mcq_pack_bases (3 bits per base)
MCQ_FORCE_BLOCK_PATH = 0x100     # debug: send every query down the block-per-query path
MCQ_DB_LOCS_64 = 0x200           # Database(flags=...): keep 64-bit locations
MCQ_DB_LOCS_GW = 0x2000          # Database(flags=...): 32-bit locations in the global-window form
MCQ_DB_SLOTS_16 = 0x4000         # Database(flags=...): 16-B slots, every list behind the slot array
MCQ_DB_BUCKETS_64 = 0x8000       # Database(flags=...): 64-B buckets with inline lists
MCQ_LOC_FIELDS64, MCQ_LOC_FIELDS32, MCQ_LOC_GLOBAL_WINDOW = 0, 1, 2
MCQ_BUILD_REMOVE_OVERPOPULATED = 0x1000   # Table / Database.build: -remove-overpopulated-features
MCQ_FORCE_RAW_SORT = 0x400       # debug: wave path without the de-duplicating pass
MCQ_NO_WAVE16 = 0x800            # debug: 513..1024 locations take the workgroup path, not the second wave stage
MCQ_NO_TWO_CLASS = 0x4000        # debug: long match lists are sorted whole (no light / heavy split)
MCQ_FORCE_LEAN_WAVE = 0x20000    # debug / A-B: the lean first wave stage (hands every list it does not want to the later stages)
MCQ_FORCE_FULL_WAVE = 0x40000    # debug / A-B: the full first wave stage, whatever the batch before suggests
MCQ_CLADE_NONE = 0xFFFFFFFF      # clade exclusion: no ancestor at the rank (a target's key, or a truth's)
MCQ_CLADE_KEEP_ALL = 0xFFFFFFFE  # clade exclusion, query keys only: no ground truth, nothing is excluded
MCQ_TARGET_HITS_MAX_SLOTS = 16   # mcq_target_hits: slot targets per query
MCQ_TARGET_HITS_MAX_KEYS = 1024  # ... distinct (target, window) pairs of one query over all its slot targets
MCQ_TARGET_UNUSED = 0xFFFFFFFF   # ... an unused slot
MCQ_TARGET_HITS_RANGE, MCQ_TARGET_HITS_KEYS, MCQ_TARGET_HITS_WINDOW = 1, 2, 4    # ... status bits of a query beyond a capacity
MCQ_ALIGN_MAX_QUERY = 2048       # mcq_align: bases of one mate
MCQ_ALIGN_MAX_SUBJECT = 4096     # ... bases of one subject
MCQ_ALIGN_QUERY_LONG, MCQ_ALIGN_SUBJECT_LONG = 1, 2    # ... status bits of a query beyond a capacity
MCQ_ALL_HITS_REG_MAX = 64        # mcq_all_hits: locations of a query sorted in registers
MCQ_ALL_HITS_WAVE_MAX = 2048     # ... sorted in LDS by one wavefront; more: the workgroup tier
MCQ_ALL_HITS_LOCS, MCQ_ALL_HITS_SEGMENT = 1, 2         # ... status bits of a query that was not answered
HIT = np.dtype([("tgt", "<u4"), ("win", "<u4"), ("hits", "<u4")])               # mcq_hit
ALIGN_JOB = np.dtype([("sub_off", "<u8"), ("sub_len", "<u4"), ("on", "<u4")])     # mcq_align_job
ALIGNMENT = np.dtype([("score", "<i4"), ("length", "<u4"), ("reverse", "<u4"), ("status", "<u4")])   # mcq_alignment

MCQ_OK, MCQ_E_ARG, MCQ_E_HIP, MCQ_E_CAPACITY, MCQ_E_UNSUPPORTED = 0, -1, -2, -3, -4


class McqError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("mcq error %d: %s" % (code, msg))
        self.code = code


class DbDesc(C.Structure):
    _fields_ = [("k", C.c_uint32), ("sketch_size", C.c_uint32), ("winlen", C.c_uint32), ("winstride", C.c_uint32),
                ("tgt_winstride", C.c_uint32), ("n_targets", C.c_uint32), ("n_keys", C.c_uint64), ("n_locs", C.c_uint64),
                ("keys", C.c_void_p), ("list_off", C.c_void_p), ("locs", C.c_void_p), ("tgt2tax", C.c_void_p),
                ("n_shards", C.c_uint32), ("shard_id", C.c_uint32), ("flags", C.c_uint32), ("device", C.c_int32),
                ("loc_win_bits", C.c_uint32), ("tgt_windows", C.c_void_p)]


class DbLayout(C.Structure):
    _fields_ = [("loc_bytes", C.c_uint32), ("loc_format", C.c_uint32), ("win_bits", C.c_uint32), ("bucket_bytes", C.c_uint32),
                ("slots_per_key", C.c_uint32), ("n_slots", C.c_uint64), ("n_keys", C.c_uint64), ("n_locs", C.c_uint64),
                ("n_ext_locs", C.c_uint64), ("n_windows", C.c_uint64), ("bytes", C.c_uint64), ("gw_offsets", C.c_void_p)]

    def as_dict(self):
        return {k: (getattr(self, k) or 0) for k, _ in self._fields_}


class BuildDesc(C.Structure):
    _fields_ = [("k", C.c_uint32), ("sketch_size", C.c_uint32), ("winlen", C.c_uint32), ("winstride", C.c_uint32),
                ("n_targets", C.c_uint32), ("bases", C.c_void_p), ("seq_off", C.c_void_p), ("tgt2tax", C.c_void_p),
                ("emulate_ranks", C.c_uint32), ("max_locs", C.c_uint32), ("n_shards", C.c_uint32),
                ("shard_id", C.c_uint32), ("flags", C.c_uint32), ("device", C.c_int32)]


class Batch(C.Structure):
    _fields_ = [("n_seqs", C.c_uint64), ("bases", C.c_void_p), ("seq_off", C.c_void_p),
                ("paired", C.c_uint32), ("flags", C.c_uint32), ("n_bases", C.c_uint64)]


class QueryOpts(C.Structure):
    _fields_ = [("max_cand", C.c_uint32), ("emulate_ranks", C.c_uint32), ("insert_size_max", C.c_uint64),
                ("flags", C.c_uint32)]


class Result(C.Structure):
    _fields_ = [("cands", C.c_void_p), ("n_cand", C.c_void_p), ("flags", C.c_uint32)]


class ClassifyOpts(C.Structure):
    _fields_ = [("hits_min", C.c_uint32), ("hits_diff_fraction", C.c_float), ("highest_rank", C.c_uint32), ("flags", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("n_queries", C.c_uint64), ("n_features", C.c_uint64), ("n_hit_features", C.c_uint64),
                ("n_locations", C.c_uint64), ("n_cands", C.c_uint64), ("n_overflow", C.c_uint64), ("n_two_class", C.c_uint64), ("n_two_class_retry", C.c_uint64), ("n_narrow_queued", C.c_uint64),
                ("n_lean_queued", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class PartsBuilderDesc(C.Structure):
    _fields_ = [("k", C.c_uint32), ("sketch_size", C.c_uint32), ("winlen", C.c_uint32), ("winstride", C.c_uint32),
                ("tgt_winstride", C.c_uint32), ("n_targets", C.c_uint32), ("tgt_windows", C.c_void_p), ("expected_locations", C.c_uint64),
                ("n_ranges", C.c_uint32), ("n_shards", C.c_uint32), ("shard_id", C.c_uint32), ("device", C.c_int32)]


class TableExtendDesc(C.Structure):
    _fields_ = [("k", C.c_uint32), ("sketch_size", C.c_uint32), ("winlen", C.c_uint32), ("winstride", C.c_uint32),
                ("n_ranks", C.c_uint32), ("max_locs", C.c_uint32), ("flags", C.c_uint32), ("device", C.c_int32),
                ("n_old_targets", C.c_uint32), ("old_tgt_windows", C.c_void_p), ("expected_old_locations", C.c_uint64)]


class ContentTotals(C.Structure):
    _fields_ = [("n_buckets", C.c_uint64), ("n_locations", C.c_uint64), ("sum2", C.c_uint64), ("sum3", C.c_uint64),
                ("max_size", C.c_uint64), ("hist", C.c_uint64 * 256)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k, _ in self._fields_[:5]}
        d["hist"] = np.array(self.hist, dtype=np.uint64)
        return d


class ShardCfg(C.Structure):
    _fields_ = [("n_ranks", C.c_uint32), ("rank", C.c_uint32), ("max_queries", C.c_uint64), ("max_seqs", C.c_uint64),
                ("max_bases", C.c_uint64), ("max_locs_per_query", C.c_uint64), ("max_features_per_peer", C.c_uint64),
                ("max_locations_per_peer", C.c_uint64)]


# mcq_exchange_fn
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p,
                          C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint32, C.c_uint32)
MCQ_SHARD_EXACT = 1
MCQ_SHARD_UNIQUE_ID_BYTES = 128

_lib = None


def lib():
    """Loads libmcq_hip.so; raises if it has not been built (no CPU fallback)."""
    global _lib
    if _lib is None:
        p = lib_path()
        if not os.path.exists(p):
            raise ImportError("HIP library %s missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950)" % p)
        L = C.CDLL(p)
        L.mcq_last_error.restype = C.c_char_p
        L.mcq_version.restype = C.c_char_p
        L.mcq_db_create.argtypes = [C.POINTER(DbDesc), C.POINTER(C.c_void_p)]
        L.mcq_db_destroy.argtypes = [C.c_void_p]
        L.mcq_db_bytes.restype = C.c_uint64; L.mcq_db_bytes.argtypes = [C.c_void_p]
        L.mcq_ws_create.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p)]
        L.mcq_ws_destroy.argtypes = [C.c_void_p]
        L.mcq_query.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Batch), C.POINTER(QueryOpts), C.POINTER(Result), C.c_void_p]
        L.mcq_ws_sync.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.mcq_query_pipelined.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Batch), C.POINTER(QueryOpts), C.POINTER(Result), C.POINTER(C.c_uint64)]
        L.mcq_ws_wait.argtypes = [C.c_void_p, C.c_uint64]
        L.mcq_owner.restype = C.c_uint32; L.mcq_owner.argtypes = [C.c_uint32, C.c_uint32]
        L.mcq_debug_matches.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Batch), C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64]
        L.mcq_ws_timing.argtypes = [C.c_void_p, C.c_int]
        L.mcq_ws_kernel_time.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        L.mcq_ws_kernel_times.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        L.mcq_count_windows.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_void_p]
        L.mcq_sketch.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mcq_lookup_count.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mcq_lookup_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mcq_db_loc_bytes.restype = C.c_uint32; L.mcq_db_loc_bytes.argtypes = [C.c_void_p]
        L.mcq_db_win_bits.restype = C.c_uint32; L.mcq_db_win_bits.argtypes = [C.c_void_p]
        L.mcq_db_layout_get.argtypes = [C.c_void_p, C.POINTER(DbLayout)]
        L.mcq_bucket_features.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mcq_assemble.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(Batch),
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mcq_fastq_index.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.mcq_fasta_index.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.mcq_reads_scratch_bytes.restype = C.c_uint64; L.mcq_reads_scratch_bytes.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64]
        L.mcq_reads_prepare.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64,
                                        C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mcq_build_table.argtypes = [C.POINTER(BuildDesc), C.POINTER(C.c_void_p)]
        L.mcq_db_build.argtypes = [C.POINTER(BuildDesc), C.POINTER(C.c_void_p)]
        L.mcq_table_info.argtypes = [C.c_void_p] + [C.c_void_p] * 6
        L.mcq_table_free.argtypes = [C.c_void_p]
        L.mcq_table_rank_split.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
        L.mcq_table_tgt_windows.argtypes = [C.c_void_p, C.c_void_p]
        L.mcq_table_remove_ambiguous.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p),
                                                 C.POINTER(C.c_uint64)]
        L.mcq_build_last_error.restype = C.c_char_p
        L.mcq_build_parts.argtypes = [C.POINTER(BuildDesc), C.POINTER(C.c_void_p)]
        L.mcq_parts_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
        L.mcq_db_from_parts.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
        L.mcq_parts_free.argtypes = [C.c_void_p]
        if hasattr(L, "mcq_parts_builder_create"):          # (an older build of the library under MCQ_HIP_LIB, for same-box A/B runs, lacks the r04 entry points)
            L.mcq_parts_builder_create.argtypes = [C.POINTER(PartsBuilderDesc), C.POINTER(C.c_void_p)]
            L.mcq_parts_builder_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]
            L.mcq_parts_builder_finish.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
            L.mcq_parts_builder_free.argtypes = [C.c_void_p]
        if hasattr(L, "mcq_bucket_limit"):                  # (as above)
            L.mcq_bucket_limit.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32,
                                           C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
            L.mcq_bucket_limit_scratch_bytes.restype = C.c_uint64; L.mcq_bucket_limit_scratch_bytes.argtypes = [C.c_uint64]
            L.mcq_bucket_limit_ws.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int32, C.c_void_p,
                                              C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
            L.mcq_parts_builder_set_bucket_limit.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
            L.mcq_parts_builder_bucket_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        if hasattr(L, "mcq_content_stats_create"):          # (as above)
            L.mcq_content_stats_create.argtypes = [C.c_uint32, C.POINTER(C.c_void_p)]
            L.mcq_content_stats_set_stream.argtypes = [C.c_void_p, C.c_void_p]
            L.mcq_content_stats_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]
            L.mcq_content_stats_totals.argtypes = [C.c_void_p, C.POINTER(ContentTotals)]
            L.mcq_content_stats_target_locations.argtypes = [C.c_void_p, C.c_void_p]
            L.mcq_content_stats_reset.argtypes = [C.c_void_p]
            L.mcq_content_stats_free.argtypes = [C.c_void_p]
        if hasattr(L, "mcq_table_extend_create"):          # (as above: a parent's library in a same-box A/B has none)
            L.mcq_table_extend_create.argtypes = [C.POINTER(TableExtendDesc), C.POINTER(C.c_void_p)]
            L.mcq_table_extend_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]
            L.mcq_table_extend_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
            L.mcq_table_extend_free.argtypes = [C.c_void_p]
        if hasattr(L, "mcq_range_build_create"):            # (as above)
            L.mcq_range_build_create.argtypes = [C.POINTER(BuildDesc), C.c_uint32, C.POINTER(C.c_void_p)]
            L.mcq_range_build_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
            L.mcq_range_build_tgt_windows.argtypes = [C.c_void_p, C.c_void_p]
            L.mcq_range_build_next.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
            L.mcq_range_build_free.argtypes = [C.c_void_p]
            L.mcq_table_shard_records.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                                  C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.mcq_reduce.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.POINTER(QueryOpts), C.POINTER(Result), C.c_void_p]
        L.mcq_packed_bytes.restype = C.c_uint64; L.mcq_packed_bytes.argtypes = [C.c_uint64]
        L.mcq_pack_bases.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p]
        L.mcq_taxonomy_create.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.POINTER(C.c_void_p)]
        L.mcq_taxonomy_destroy.argtypes = [C.c_void_p]
        L.mcq_classify.argtypes = [C.c_void_p, C.POINTER(Result), C.c_uint64, C.c_uint32, C.POINTER(ClassifyOpts), C.c_void_p,
                                   C.c_void_p, C.c_void_p]
        L.mcq_ws_set_classify.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(ClassifyOpts)]
        L.mcq_ws_taxon_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.mcq_ws_set_exclusion.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        L.mcq_ws_set_query_clades.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]
        if hasattr(L, "mcq_target_hits"):           # (an MCQ_HIP_LIB variant built from an older state has none: same-box A/B against a parent)
            L.mcq_target_hits_range_cap.restype = C.c_uint32; L.mcq_target_hits_range_cap.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
            L.mcq_target_hits.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            L.mcq_target_slots.argtypes = [C.POINTER(Result), C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                           C.c_uint32, C.c_void_p]
        if hasattr(L, "mcq_align"):
            L.mcq_align.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        if hasattr(L, "mcq_all_hits"):
            L.mcq_all_hits_count.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_void_p]
            L.mcq_all_hits.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                       C.c_void_p, C.c_void_p]
        if hasattr(L, "mcq_accmap_create"):
            L.mcq_accmap_create.argtypes = [C.c_char_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]
            L.mcq_accmap_create_rule.argtypes = [C.c_char_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int,
                                                 C.POINTER(C.c_void_p)]
            L.mcq_accmap_chunk.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.c_void_p]
            L.mcq_accmap_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
            L.mcq_accmap_free.argtypes = [C.c_void_p]
        if hasattr(L, "mcq_merge_create"):
            L.mcq_merge_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int,
                                           C.POINTER(C.c_void_p)]
            L.mcq_merge_chunk.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(C.c_int32), C.c_void_p]
            L.mcq_merge_lines.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                          C.c_uint32, C.c_uint32, C.c_void_p]
            L.mcq_merge_finish.argtypes = [C.c_void_p, C.POINTER(ClassifyOpts), C.c_void_p, C.c_void_p, C.c_void_p]
            L.mcq_merge_lists.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
            L.mcq_merge_headers.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            L.mcq_merge_free.argtypes = [C.c_void_p]
        if hasattr(L, "mcq_coverage_create"):
            L.mcq_coverage_create.argtypes = [C.c_void_p, C.c_uint32, C.c_int32, C.POINTER(C.c_void_p)]
            L.mcq_coverage_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p]
            L.mcq_coverage_read.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]
            L.mcq_coverage_reset.argtypes = [C.c_void_p, C.c_void_p]
            L.mcq_coverage_bitmap_words.restype = C.c_uint64; L.mcq_coverage_bitmap_words.argtypes = [C.c_void_p]
            L.mcq_coverage_bitmap.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            L.mcq_coverage_free.argtypes = [C.c_void_p]
        L.mcq_shard_create.argtypes = [C.c_void_p, C.POINTER(ShardCfg), C.POINTER(C.c_void_p)]
        L.mcq_shard_destroy.argtypes = [C.c_void_p]
        L.mcq_shard_unique_id.argtypes = [C.c_void_p]
        L.mcq_shard_comm_rccl.argtypes = [C.c_void_p, C.c_void_p]
        L.mcq_shard_set_exchange.argtypes = [C.c_void_p, EXCHANGE_FN, C.c_void_p]
        L.mcq_shard_query.argtypes = [C.c_void_p, C.POINTER(Batch), C.POINTER(QueryOpts), C.POINTER(Result), C.c_void_p,
                                      C.c_uint32, C.POINTER(Batch)]
        L.mcq_shard_sync.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.mcq_shard_set_caps.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
        L.mcq_shard_get_caps.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.mcq_shard_timing.argtypes = [C.c_void_p, C.c_int]
        L.mcq_shard_kernel_times.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        L.mcq_shard_stage_times.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        L.mcq_shard_exchange_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        _lib = L
    return _lib


def _chk(rc):
    if rc != 0:
        raise McqError(rc, lib().mcq_last_error().decode())


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Database:
    """GPU-resident feature -> locations multimap (one shard).  Mirrors the query half
    of the reference's sketch_database: built from the union of its shard tables."""

    def __init__(self, keys, list_off, locs, tgt2tax, k=16, sketch_size=16, winlen=128, winstride=113,
                 tgt_winstride=0, n_shards=1, shard_id=0, device=0, device_ptrs=None, flags=0, loc_win_bits=0, tgt_windows=None):
        """keys/list_off/locs/tgt2tax: numpy arrays (host) -- or, with device_ptrs=dict(
        keys=ptr, list_off=ptr, locs=ptr, tgt2tax=ptr, n_keys=, n_locs=, n_targets=[, tgt_windows=ptr]), raw device pointers.
        tgt_windows (host: numpy u32 [n_targets]): windows per target for the global-window location form."""
        d = DbDesc()
        d.k, d.sketch_size, d.winlen, d.winstride, d.tgt_winstride = k, sketch_size, winlen, winstride, tgt_winstride
        d.n_shards, d.shard_id, d.device = n_shards, shard_id, device
        d.loc_win_bits = loc_win_bits
        if device_ptrs is None:
            self._keep = (np.ascontiguousarray(keys, np.uint32), np.ascontiguousarray(list_off, np.uint64),
                          np.ascontiguousarray(locs, np.uint64), np.ascontiguousarray(tgt2tax, np.uint32))
            kk, oo, ll, tt = self._keep
            assert len(oo) == len(kk) + 1
            d.n_keys, d.n_locs, d.n_targets = len(kk), len(ll), len(tt)
            d.keys, d.list_off, d.locs, d.tgt2tax = _np_ptr(kk), _np_ptr(oo), _np_ptr(ll), _np_ptr(tt)
            if tgt_windows is not None:
                tw = np.ascontiguousarray(tgt_windows, np.uint32)
                assert len(tw) == len(tt)
                self._keep = self._keep + (tw,)
                d.tgt_windows = _np_ptr(tw)
            d.flags = flags
        else:
            p = device_ptrs
            d.n_keys, d.n_locs, d.n_targets = p["n_keys"], p["n_locs"], p["n_targets"]
            d.keys, d.list_off, d.locs, d.tgt2tax = p["keys"], p["list_off"], p["locs"], p["tgt2tax"]
            d.tgt_windows = p.get("tgt_windows")
            d.flags = MCQ_DEVICE_PTRS | flags
        self.k, self.sketch_size, self.winlen, self.winstride = k, sketch_size, winlen, winstride
        self.device = device
        h = C.c_void_p()
        _chk(lib().mcq_db_create(C.byref(d), C.byref(h)))
        self.h = h

    @classmethod
    def build(cls, bases_ptr, seq_off_ptr, tgt2tax_ptr, n_targets, emulate_ranks=1, k=16, sketch_size=16, winlen=128,
              winstride=113, max_locs=0, n_shards=1, shard_id=0, device=0, flags=0, device_ptrs=True):
        """mcq_db_build: reference sequences -> queryable handle, all on the GPU"""
        d = _build_desc(bases_ptr, seq_off_ptr, tgt2tax_ptr, n_targets, emulate_ranks, k, sketch_size, winlen, winstride,
                        max_locs, n_shards, shard_id, device, flags, device_ptrs)
        self = cls.__new__(cls)
        self.k, self.sketch_size, self.winlen, self.winstride, self.device = k, sketch_size, winlen, winstride, device
        h = C.c_void_p()
        rc = lib().mcq_db_build(C.byref(d), C.byref(h))
        if rc != 0:
            raise McqError(rc, (lib().mcq_build_last_error() or b"").decode())
        self.h = h
        return self

    def bytes(self):
        return int(lib().mcq_db_bytes(self.h))

    # ---- staged entry points (device pointers only) -------------------------------
    def count_windows(self, bases_ptr, seq_off_ptr, n_seqs, win_off_ptr, stream=None, flags=0):
        """flags: more batch flags (MCQ_BATCH_RANGES); the same for sketch and assemble"""
        b = Batch(n_seqs, bases_ptr, seq_off_ptr, 0, MCQ_DEVICE_PTRS | flags)
        _chk(lib().mcq_count_windows(self.h, C.byref(b), win_off_ptr, stream))

    def sketch(self, bases_ptr, seq_off_ptr, n_seqs, win_off_ptr, features_ptr, n_feat_ptr, stream=None, flags=0):
        b = Batch(n_seqs, bases_ptr, seq_off_ptr, 0, MCQ_DEVICE_PTRS | flags)
        _chk(lib().mcq_sketch(self.h, C.byref(b), win_off_ptr, features_ptr, n_feat_ptr, stream))

    def lookup_count(self, features_ptr, n, list_len_ptr, list_src_ptr=None, stream=None):
        _chk(lib().mcq_lookup_count(self.h, features_ptr, n, list_len_ptr, list_src_ptr, stream))

    def lookup_gather(self, features_ptr, n, out_off_ptr, out_locs_ptr, list_len_ptr=None, list_src_ptr=None, stream=None):
        """out_locs in the handle's native width (loc_bytes())"""
        _chk(lib().mcq_lookup_gather(self.h, features_ptr, n, list_len_ptr, list_src_ptr, out_off_ptr, out_locs_ptr, stream))

    def loc_bytes(self):
        return int(lib().mcq_db_loc_bytes(self.h))

    def win_bits(self):
        return int(lib().mcq_db_win_bits(self.h))

    def layout(self):
        """what the handle was built as: location format / width, bucket size, load factor, sizes (mcq_db_layout)"""
        lo = DbLayout()
        _chk(lib().mcq_db_layout_get(self.h, C.byref(lo)))
        return lo.as_dict()

    def assemble(self, n_lists, list_len_ptr, src_slot_ptr, n_slots, src_locs_ptr, bases_ptr, seq_off_ptr, n_seqs, paired,
                 win_off_ptr, loc_off_ptr, query_len_ptr, dst_locs_ptr, stream=None, flags=0):
        b = Batch(n_seqs, bases_ptr, seq_off_ptr, 1 if paired else 0, MCQ_DEVICE_PTRS | flags)
        _chk(lib().mcq_assemble(self.h, n_lists, list_len_ptr, src_slot_ptr, n_slots, src_locs_ptr, C.byref(b), win_off_ptr,
                                loc_off_ptr, query_len_ptr, dst_locs_ptr, stream))

    def close(self):
        if getattr(self, "h", None):
            lib().mcq_db_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # interpreter shutdown
            pass


class Workspace:
    def __init__(self, db, max_queries, max_bases, max_locs_per_query=0):
        self.db = db
        self.max_queries = max_queries
        h = C.c_void_p()
        _chk(lib().mcq_ws_create(db.h, max_queries, max_bases, max_locs_per_query, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            lib().mcq_ws_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # interpreter shutdown
            pass

    def sync(self, stream=None):
        st = Stats()
        _chk(lib().mcq_ws_sync(self.h, stream, C.byref(st)))
        return st.as_dict()

    # ---- host-buffer call: numpy in, numpy out (copies + sync inside) -------------
    def query_host(self, bases, seq_off, paired, max_cand=2, emulate_ranks=1, insert_size_max=0, flags=0, packed=False):
        """packed: `bases` holds the packed form (pack_bases) of the batch instead of ASCII"""
        seq_off = np.ascontiguousarray(seq_off, np.uint64)
        n_seqs = len(seq_off) - 1
        nq = n_seqs // 2 if paired else n_seqs
        bases_arr = np.frombuffer(bases, dtype=np.uint8) if not isinstance(bases, np.ndarray) else bases
        bases_arr = np.ascontiguousarray(bases_arr)
        b = Batch(n_seqs, _np_ptr(bases_arr) if len(bases_arr) else None, _np_ptr(seq_off), 1 if paired else 0,
                  MCQ_BATCH_PACKED if packed else 0, int(seq_off[-1]) if packed else 0)
        o = QueryOpts(max_cand, emulate_ranks, insert_size_max, flags)
        cands = np.zeros((max(nq, 1), max_cand, 4), np.uint32)
        ncand = np.zeros(max(nq, 1), np.uint32)
        r = Result(_np_ptr(cands), _np_ptr(ncand), 0)
        _chk(lib().mcq_query(self.db.h, self.h, C.byref(b), C.byref(o), C.byref(r), None))
        return cands[:nq], ncand[:nq]

    # ---- device-buffer call: raw pointers, enqueue only --------------------------
    def query_device(self, bases_ptr, seq_off_ptr, n_seqs, paired, cands_ptr, ncand_ptr, max_cand=2,
                     emulate_ranks=1, insert_size_max=0, flags=0, stream=None, ranges=False, packed_bases=0):
        """packed_bases > 0: bases_ptr is the packed form of a batch of that many bases"""
        b = Batch(n_seqs, bases_ptr, seq_off_ptr, 1 if paired else 0,
                  MCQ_DEVICE_PTRS | (MCQ_BATCH_RANGES if ranges else 0) | (MCQ_BATCH_PACKED if packed_bases else 0), packed_bases)
        o = QueryOpts(max_cand, emulate_ranks, insert_size_max, flags)
        r = Result(cands_ptr, ncand_ptr, MCQ_DEVICE_PTRS)
        _chk(lib().mcq_query(self.db.h, self.h, C.byref(b), C.byref(o), C.byref(r), stream))

    # ---- host buffers, pipelined: raw HOST pointers (pinned), returns a ticket for wait()
    def query_pipelined(self, bases_ptr, seq_off_ptr, n_seqs, paired, cands_ptr, ncand_ptr, max_cand=2, emulate_ranks=1,
                        insert_size_max=0, flags=0, packed_bases=0):
        b = Batch(n_seqs, bases_ptr, seq_off_ptr, 1 if paired else 0, MCQ_BATCH_PACKED if packed_bases else 0, packed_bases)
        o = QueryOpts(max_cand, emulate_ranks, insert_size_max, flags)
        r = Result(cands_ptr, ncand_ptr, 0)
        t = C.c_uint64(0)
        _chk(lib().mcq_query_pipelined(self.db.h, self.h, C.byref(b), C.byref(o), C.byref(r), C.byref(t)))
        return int(t.value)

    def wait(self, ticket):
        _chk(lib().mcq_ws_wait(self.h, ticket))

    # ---- classification of every batch on the device (mcq_ws_set_classify / mcq_ws_taxon_counts)
    def set_classify(self, taxonomy, hits_min=1, hits_diff_fraction=1.0, highest_rank=19):
        """attaches a Taxonomy (None detaches): every query call then adds its classified queries into the counts"""
        if taxonomy is None:
            _chk(lib().mcq_ws_set_classify(self.h, None, None)); self._tx = None
            return
        o = ClassifyOpts(hits_min, hits_diff_fraction, highest_rank, 0)
        _chk(lib().mcq_ws_set_classify(self.h, taxonomy.h, C.byref(o)))
        self._tx = taxonomy; self._cls_n = taxonomy.n_taxa + 1

    def taxon_counts(self, reset=False):
        """u64 [n_taxa + 1]: classified queries per taxon index, the last slot the unclassified ones"""
        out = np.zeros(getattr(self, "_cls_n", 0), np.uint64)
        _chk(lib().mcq_ws_taxon_counts(self.h, _np_ptr(out), 1 if reset else 0))
        return out

    # ---- clade exclusion (mcq_ws_set_exclusion / mcq_ws_set_query_clades)
    def set_exclusion(self, tgt_clade, device_ptr=None, n_targets=0):
        """attaches the targets' clade keys (u32 [n_targets], MCQ_CLADE_NONE = no ancestor at the rank; None detaches): a host
        array, or (device_ptr, n_targets); either is copied.  A device table is not searched for MCQ_CLADE_KEEP_ALL."""
        if device_ptr is not None:
            _chk(lib().mcq_ws_set_exclusion(self.h, device_ptr, n_targets, MCQ_DEVICE_PTRS))
            return
        if tgt_clade is None:
            _chk(lib().mcq_ws_set_exclusion(self.h, None, 0, 0))
            return
        a = np.ascontiguousarray(tgt_clade, np.uint32)
        _chk(lib().mcq_ws_set_exclusion(self.h, _np_ptr(a), len(a), 0))

    def set_query_clades(self, query_clade, device_ptr=None, n_queries=0):
        """the clade keys of the NEXT batch (u32 per query; MCQ_CLADE_KEEP_ALL = no ground truth): a host array, which is
        copied, or (device_ptr, n_queries), which that batch's kernels read in place"""
        if device_ptr is not None:
            _chk(lib().mcq_ws_set_query_clades(self.h, device_ptr, n_queries, MCQ_DEVICE_PTRS))
            return
        a = np.ascontiguousarray(query_clade, np.uint32)
        _chk(lib().mcq_ws_set_query_clades(self.h, _np_ptr(a) if len(a) else _np_ptr(np.zeros(1, np.uint32)), len(a), 0))

    # ---- per-target window hit lists (mcq_target_hits): what -hits-per-seq prints
    def target_hits_range_cap(self, longest_query, insert_size_max=0):
        """range width of a query of that many bases (both mates): the range_cap a batch with that longest query needs"""
        return int(lib().mcq_target_hits_range_cap(self.db.h, longest_query, insert_size_max))

    def target_hits(self, bases_ptr, seq_off_ptr, n_seqs, paired, targets_ptr, n_slots, range_cap, ranges_ptr, counts_ptr,
                    status_ptr, insert_size_max=0, stream=None, ranges=False, packed_bases=0):
        """device pointers, enqueue only: targets u32 [nq, n_slots] (MCQ_TARGET_UNUSED = unused slot) -> ranges u32 [nq, n_slots, 4]
        (tgt, hits, win_beg, n_win), counts u32 [nq, n_slots, range_cap] (written for i < n_win only), status u32 [nq].  A query
        beyond a capacity gets n_win = 0 everywhere, a status bit, and makes the next sync() raise MCQ_E_CAPACITY."""
        b = Batch(n_seqs, bases_ptr, seq_off_ptr, 1 if paired else 0,
                  MCQ_DEVICE_PTRS | (MCQ_BATCH_RANGES if ranges else 0) | (MCQ_BATCH_PACKED if packed_bases else 0), packed_bases)
        _chk(lib().mcq_target_hits(self.db.h, self.h, C.byref(b), targets_ptr, n_slots, insert_size_max, range_cap, ranges_ptr,
                                   counts_ptr, status_ptr, stream))

    def target_hits_host(self, bases, seq_off, paired, targets, range_cap=None, insert_size_max=0, packed=False, fill=0, sync=True,
                         ranges=False):
        """convenience form for tests: numpy in, numpy out (the copies go through torch; waits for the device).  targets: u32
        [nq, n_slots].  range_cap None: what the longest query needs.  The words of counts the kernel leaves alone hold `fill`.
        Every output has 64 guard words behind it; a changed one raises.  sync False: the caller calls sync() (and gets the
        capacity error there).  ranges: seq_off holds 2 * n_seqs (begin, end) byte ranges into `bases` (MCQ_BATCH_RANGES)."""
        import torch
        dev = torch.device("cuda", self.db.device)
        seq_off = np.ascontiguousarray(seq_off, np.uint64)
        n_seqs = len(seq_off) // 2 if ranges else len(seq_off) - 1
        nq = n_seqs // 2 if paired else n_seqs
        targets = np.ascontiguousarray(targets, np.uint32).reshape(nq, -1)
        n_slots = targets.shape[1]
        lens = (seq_off[1::2].astype(np.int64) - seq_off[0::2].astype(np.int64)) if ranges else np.diff(seq_off.astype(np.int64))
        qlens = lens[0:2 * nq:2] + lens[1:2 * nq:2] if paired else lens
        if range_cap is None:
            range_cap = self.target_hits_range_cap(int(qlens.max()) if nq else 0, insert_size_max)
        raw = np.frombuffer(bases, dtype=np.uint8) if not isinstance(bases, np.ndarray) else bases.view(np.uint8)
        d_bases = torch.from_numpy(np.concatenate([raw, np.zeros(8, np.uint8)])).to(dev)
        d_off = torch.from_numpy(seq_off.view(np.int64)).to(dev)
        d_tgt = torch.from_numpy(targets.view(np.int32)).to(dev)
        guard, G = 0x5EEDFACE, 64
        sizes = (nq * n_slots * 4, nq * n_slots * range_cap, nq)
        host = [np.full(n + G, g, np.uint32) for n, g in zip(sizes, (guard, fill, guard))]
        for h, n in zip(host, sizes):
            h[n:] = guard
        d_rng, d_cnt, d_st = (torch.from_numpy(h.view(np.int32)).to(dev) for h in host)
        st = torch.cuda.current_stream(dev).cuda_stream
        self.target_hits(d_bases.data_ptr(), d_off.data_ptr(), n_seqs, paired, d_tgt.data_ptr(), n_slots, range_cap, d_rng.data_ptr(),
                         d_cnt.data_ptr(), d_st.data_ptr(), insert_size_max=insert_size_max, stream=st, ranges=ranges,
                         packed_bases=int(seq_off[-1]) if packed else 0)
        torch.cuda.synchronize(dev)
        got = [d.cpu().numpy().view(np.uint32) for d in (d_rng, d_cnt, d_st)]
        for g, n in zip(got, sizes):
            if not (g[n:] == guard).all():
                raise AssertionError("mcq_target_hits wrote behind an output")
        out = (got[0][:sizes[0]].reshape(nq, n_slots, 4), got[1][:sizes[1]].reshape(nq, n_slots, range_cap), got[2][:nq])
        if sync:
            self.sync(st)
        return out

    # ---- all hits of a read (mcq_all_hits_count / mcq_all_hits): what -allhits prints
    def all_hits_count(self, bases_ptr, seq_off_ptr, n_seqs, paired, loc_off_ptr, stream=None, ranges=False, packed_bases=0):
        """device pointers, enqueue only: loc_off u64 [nq + 1] = exclusive prefix sums of the queries' location counts"""
        b = Batch(n_seqs, bases_ptr, seq_off_ptr, 1 if paired else 0,
                  MCQ_DEVICE_PTRS | (MCQ_BATCH_RANGES if ranges else 0) | (MCQ_BATCH_PACKED if packed_bases else 0), packed_bases)
        _chk(lib().mcq_all_hits_count(self.db.h, self.h, C.byref(b), loc_off_ptr, stream))

    def all_hits(self, bases_ptr, seq_off_ptr, n_seqs, paired, loc_off_ptr, hits_ptr, cap, n_hits_ptr, status_ptr, stream=None,
                 ranges=False, packed_bases=0):
        """device pointers, enqueue only: query q's entries (HIT: tgt, win, hits; ascending) to hits[loc_off[q] .. + n_hits[q]); a query
        with a status bit (MCQ_ALL_HITS_*) gets n_hits = 0 and nothing written"""
        b = Batch(n_seqs, bases_ptr, seq_off_ptr, 1 if paired else 0,
                  MCQ_DEVICE_PTRS | (MCQ_BATCH_RANGES if ranges else 0) | (MCQ_BATCH_PACKED if packed_bases else 0), packed_bases)
        _chk(lib().mcq_all_hits(self.db.h, self.h, C.byref(b), loc_off_ptr, hits_ptr, cap, n_hits_ptr, status_ptr, stream))

    def all_hits_host(self, bases, seq_off, paired, packed=False, ranges=False):
        """convenience form: numpy in, numpy out (the copies go through torch; waits for the device).  Returns (hits, status): per
        query its entries as HIT records, and u32 [nq] status words (a query with a status bit has no entries)"""
        import torch
        dev = torch.device("cuda", self.db.device)
        seq_off = np.ascontiguousarray(seq_off, np.uint64)
        n_seqs = len(seq_off) // 2 if ranges else len(seq_off) - 1
        nq = n_seqs // 2 if paired else n_seqs
        raw = np.frombuffer(bases, dtype=np.uint8) if not isinstance(bases, np.ndarray) else bases.view(np.uint8)
        d_bases = torch.from_numpy(np.concatenate([raw, np.zeros(8, np.uint8)])).to(dev)
        d_seq = torch.from_numpy(seq_off.view(np.int64)).to(dev) if len(seq_off) else torch.zeros(1, dtype=torch.int64, device=dev)
        pb = int(seq_off[-1]) if packed else 0
        st = torch.cuda.current_stream(dev).cuda_stream
        d_off = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
        self.all_hits_count(d_bases.data_ptr(), d_seq.data_ptr(), n_seqs, paired, d_off.data_ptr(), stream=st, ranges=ranges, packed_bases=pb)
        off = d_off.cpu().numpy()
        total = int(off[nq])
        d_hits = torch.zeros((max(total, 1), 3), dtype=torch.int32, device=dev)
        d_n = torch.zeros(max(nq, 1), dtype=torch.int32, device=dev)
        d_st = torch.zeros(max(nq, 1), dtype=torch.int32, device=dev)
        self.all_hits(d_bases.data_ptr(), d_seq.data_ptr(), n_seqs, paired, d_off.data_ptr(), d_hits.data_ptr(), total, d_n.data_ptr(),
                      d_st.data_ptr(), stream=st, ranges=ranges, packed_bases=pb)
        torch.cuda.synchronize(dev)
        ent = d_hits.cpu().numpy().view(np.uint32).reshape(-1).view(HIT)
        n = d_n.cpu().numpy().view(np.uint32)
        return [ent[int(off[q]):int(off[q]) + int(n[q])].copy() for q in range(nq)], d_st.cpu().numpy().view(np.uint32)[:nq].copy()

    # ---- read-to-candidate alignment (mcq_align): what -align prints
    def align_device(self, bases_ptr, seq_off_ptr, n_seqs, paired, subjects_ptr, jobs_ptr, max_query, max_subject, out_ptr,
                     out_query_ptr, out_subject_ptr, text_cap, stream=None, ranges=False, packed_bases=0):
        """device pointers, enqueue only: jobs mcq_align_job [nq] (ALIGN_JOB) -> out mcq_alignment [nq] (ALIGNMENT) and the two aligned
        strings of query q at out_query / out_subject + q * text_cap.  A query beyond a capacity gets a status bit and length 0."""
        b = Batch(n_seqs, bases_ptr, seq_off_ptr, 1 if paired else 0,
                  MCQ_DEVICE_PTRS | (MCQ_BATCH_RANGES if ranges else 0) | (MCQ_BATCH_PACKED if packed_bases else 0), packed_bases)
        _chk(lib().mcq_align(self.h, C.byref(b), subjects_ptr, jobs_ptr, max_query, max_subject, out_ptr, out_query_ptr,
                             out_subject_ptr, text_cap, stream))

    def align(self, bases, seq_off, paired, subjects, jobs, max_query=None, max_subject=None, text_cap=None, ranges=False,
              packed=False, fill=0x2E):
        """numpy in, numpy out (the copies go through torch; waits for the device).  bases / subjects: bytes or u8 arrays; jobs: rows
        of (sub_off, sub_len, on).  max_query / max_subject None: what the longest mate / subject of the batch needs, within the
        kernel's capacities; text_cap None: their sum.  Returns a dict: score i32 [nq], reverse u32 [nq], status u32 [nq], length
        u32 [nq], query / subject: the aligned strings (bytes) per query, text_query / text_subject: the raw u8 [nq, text_cap]
        buffers, which held `fill` before the call.  Every output has 64 guard bytes behind it; a changed one raises."""
        import torch
        dev = torch.device("cuda", self.db.device)
        seq_off = np.ascontiguousarray(seq_off, np.uint64)
        n_seqs = len(seq_off) // 2 if ranges else len(seq_off) - 1
        nq = n_seqs // 2 if paired else n_seqs
        j = np.zeros(max(nq, 1), ALIGN_JOB)
        for i, (o, n, on) in enumerate(jobs):
            j[i] = (o, n, on)
        lens = (seq_off[1::2].astype(np.int64) - seq_off[0::2].astype(np.int64)) if ranges else np.diff(seq_off.astype(np.int64))
        if max_query is None:
            max_query = min(int(lens.max()) if len(lens) else 0, MCQ_ALIGN_MAX_QUERY)
        if max_subject is None:
            max_subject = min(int(j["sub_len"][:nq].max()) if nq else 0, MCQ_ALIGN_MAX_SUBJECT)
        if text_cap is None:
            text_cap = max(1, max_query + max_subject)

        def u8(x):
            return (np.frombuffer(x, dtype=np.uint8) if not isinstance(x, np.ndarray) else x.view(np.uint8))
        d_bases = torch.from_numpy(np.concatenate([u8(bases), np.zeros(8, np.uint8)])).to(dev)
        d_sub = torch.from_numpy(np.concatenate([u8(subjects), np.zeros(8, np.uint8)])).to(dev)
        d_off = torch.from_numpy(seq_off.view(np.int64)).to(dev) if len(seq_off) else torch.zeros(1, dtype=torch.int64, device=dev)
        d_jobs = torch.from_numpy(j.view(np.uint8)).to(dev)
        G, guard = 64, 0xA5
        h_out = np.full(max(nq, 1) * ALIGNMENT.itemsize + G, guard, np.uint8)
        h_q = np.full(nq * text_cap + G, fill, np.uint8); h_q[nq * text_cap:] = guard
        h_s = h_q.copy()
        d_out, d_q, d_s = (torch.from_numpy(h).to(dev) for h in (h_out, h_q, h_s))
        st = torch.cuda.current_stream(dev).cuda_stream
        self.align_device(d_bases.data_ptr(), d_off.data_ptr(), n_seqs, paired, d_sub.data_ptr(), d_jobs.data_ptr(), max_query,
                          max_subject, d_out.data_ptr(), d_q.data_ptr(), d_s.data_ptr(), text_cap, stream=st, ranges=ranges,
                          packed_bases=int(seq_off[-1]) if packed else 0)
        torch.cuda.synchronize(dev)
        g_out, g_q, g_s = (d.cpu().numpy() for d in (d_out, d_q, d_s))
        for g, n in ((g_out, nq * ALIGNMENT.itemsize), (g_q, nq * text_cap), (g_s, nq * text_cap)):
            if not (g[n:n + G] == guard).all() or (nq == 0 and not (g[:G] == guard).all()):
                raise AssertionError("mcq_align wrote behind an output")
        res = g_out[:nq * ALIGNMENT.itemsize].view(ALIGNMENT)
        tq, ts = g_q[:nq * text_cap].reshape(nq, text_cap), g_s[:nq * text_cap].reshape(nq, text_cap)
        return {"score": res["score"].copy(), "reverse": res["reverse"].copy(), "status": res["status"].copy(),
                "length": res["length"].copy(), "text_query": tq, "text_subject": ts,
                "query": [tq[q, :res["length"][q]].tobytes() for q in range(nq)],
                "subject": [ts[q, :res["length"][q]].tobytes() for q in range(nq)]}

    def timing(self, enable):
        _chk(lib().mcq_ws_timing(self.h, 1 if enable else 0))

    def kernel_time(self):
        ms, n = C.c_double(0), C.c_uint64(0)
        _chk(lib().mcq_ws_kernel_time(self.h, C.byref(ms), C.byref(n)))
        return ms.value, int(n.value)

    def phase_clocks(self):
        """diagnostic builds (-DMCQ_PHASE_CLOCK): shader clocks per phase of the workgroup kernel of the last synchronised call"""
        out = (C.c_uint64 * 22)()
        if hasattr(lib(), "mcq_debug_phase_clocks"):
            _chk(lib().mcq_debug_phase_clocks(self.h, out))
        return [int(x) for x in out]

    def kernel_times(self):
        """(ms of first wave stage, second wave stage, workgroup kernel summed over the timed batches; n batches)"""
        ms, n = (C.c_double * 3)(), C.c_uint64(0)
        _chk(lib().mcq_ws_kernel_times(self.h, ms, C.byref(n)))
        return [float(x) for x in ms], int(n.value)

    def reduce_device(self, n_queries, loc_off_ptr, locs_ptr, query_len_ptr, cands_ptr, ncand_ptr, max_cand=2,
                      emulate_ranks=1, insert_size_max=0, flags=0, stream=None):
        o = QueryOpts(max_cand, emulate_ranks, insert_size_max, flags)
        r = Result(cands_ptr, ncand_ptr, MCQ_DEVICE_PTRS)
        _chk(lib().mcq_reduce(self.db.h, self.h, n_queries, loc_off_ptr, locs_ptr, query_len_ptr, C.byref(o), C.byref(r), stream))

    def debug_matches(self, bases, seq_off, paired, path_flags=0):
        """sorted match list of every query, tapped on the path the query takes (path_flags = 0) or the one a
        test hook (MCQ_FORCE_BLOCK_PATH, MCQ_FORCE_RAW_SORT, MCQ_NO_WAVE16) selects"""
        seq_off = np.ascontiguousarray(seq_off, np.uint64)
        n_seqs = len(seq_off) - 1
        nq = n_seqs // 2 if paired else n_seqs
        bases_arr = np.ascontiguousarray(np.frombuffer(bases, dtype=np.uint8))
        b = Batch(n_seqs, _np_ptr(bases_arr) if len(bases_arr) else None, _np_ptr(seq_off), 1 if paired else 0, 0)
        moff = np.zeros(nq + 1, np.uint64)
        _chk(lib().mcq_debug_matches(self.db.h, self.h, C.byref(b), path_flags, _np_ptr(moff), None, 0))
        m = np.zeros(max(1, int(moff[nq])), np.uint64)
        _chk(lib().mcq_debug_matches(self.db.h, self.h, C.byref(b), path_flags, _np_ptr(moff), _np_ptr(m), len(m)))
        return moff, m[:int(moff[nq])]


class Taxonomy:
    """The ranked-lineage table classify needs, on the device (mcq_taxonomy_create): lineage u32 [n_taxa, 21], rank u8
    [n_taxa], as host.RefDb.lineages() returns them."""

    def __init__(self, lineage, rank, device=0):
        self._lin = np.ascontiguousarray(lineage, np.uint32)
        self._rank = np.ascontiguousarray(rank, np.uint8)
        self.n_taxa = len(self._rank)
        assert self._lin.size == self.n_taxa * 21
        h = C.c_void_p()
        _chk(lib().mcq_taxonomy_create(_np_ptr(self._lin), _np_ptr(self._rank), self.n_taxa, device, C.byref(h)))
        self.h = h

    def classify(self, cands_ptr, ncand_ptr, n_queries, max_cand, hits_min=1, hits_diff_fraction=1.0, highest_rank=19,
                 best_ptr=None, counts_ptr=None, stream=None):
        """mcq_classify on device buffers (enqueue only): best u32 [n_queries], counts u64 [n_taxa + 1] (added to)"""
        r = Result(cands_ptr, ncand_ptr, MCQ_DEVICE_PTRS)
        o = ClassifyOpts(hits_min, hits_diff_fraction, highest_rank, 0)
        _chk(lib().mcq_classify(self.h, C.byref(r), n_queries, max_cand, C.byref(o), best_ptr, counts_ptr, stream))

    def close(self):
        if getattr(self, "h", None):
            lib().mcq_taxonomy_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # interpreter shutdown
            pass


class Shard:
    """mcq_shard_*: the feature-sharded multi-GPU path of one rank (one process per GPU).  `db` is this rank's shard
    (Database(..., n_shards=n_ranks, shard_id=rank)).  All calls are collective."""

    def __init__(self, db, n_ranks, rank, max_queries, max_bases, max_seqs=0, max_locs_per_query=0,
                 max_features_per_peer=0, max_locations_per_peer=0):
        self.db, self.n_ranks, self.rank = db, n_ranks, rank
        cfg = ShardCfg(n_ranks, rank, max_queries, max_seqs, max_bases, max_locs_per_query, max_features_per_peer,
                       max_locations_per_peer)
        h = C.c_void_p()
        _chk(lib().mcq_shard_create(db.h, C.byref(cfg), C.byref(h)))
        self.h = h
        self._xfn = None

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(MCQ_SHARD_UNIQUE_ID_BYTES)
        _chk(lib().mcq_shard_unique_id(buf))
        return buf.raw

    def comm_rccl(self, unique_id):
        assert len(unique_id) == MCQ_SHARD_UNIQUE_ID_BYTES
        _chk(lib().mcq_shard_comm_rccl(self.h, C.create_string_buffer(unique_id, MCQ_SHARD_UNIQUE_ID_BYTES)))

    def set_exchange(self, fn):
        """fn: an EXCHANGE_FN (kept alive here)"""
        self._xfn = fn
        _chk(lib().mcq_shard_set_exchange(self.h, fn, None))

    def query(self, bases_ptr, seq_off_ptr, n_seqs, paired, cands_ptr, ncand_ptr, max_cand=2, emulate_ranks=1,
              insert_size_max=0, flags=0, stream=None, exact=False, next_batch=None):
        """next_batch = (bases_ptr, seq_off_ptr, n_seqs) of the following call (resident): sketched under this batch's exchange"""
        b = Batch(n_seqs, bases_ptr, seq_off_ptr, 1 if paired else 0, MCQ_DEVICE_PTRS)
        o = QueryOpts(max_cand, emulate_ranks, insert_size_max, flags)
        r = Result(cands_ptr, ncand_ptr, MCQ_DEVICE_PTRS)
        nb = None
        if next_batch is not None:
            nb = C.byref(Batch(next_batch[2], next_batch[0], next_batch[1], 1 if paired else 0, MCQ_DEVICE_PTRS))
        _chk(lib().mcq_shard_query(self.h, C.byref(b), C.byref(o), C.byref(r), stream, MCQ_SHARD_EXACT if exact else 0, nb))

    def sync(self, stream=None):
        st = Stats()
        _chk(lib().mcq_shard_sync(self.h, stream, C.byref(st)))
        return st.as_dict()

    def caps(self):
        f, l = C.c_uint64(0), C.c_uint64(0)
        _chk(lib().mcq_shard_get_caps(self.h, C.byref(f), C.byref(l)))
        return int(f.value), int(l.value)

    def set_caps(self, features_per_peer, locations_per_peer):
        _chk(lib().mcq_shard_set_caps(self.h, features_per_peer, locations_per_peer))

    def timing(self, enable):
        _chk(lib().mcq_shard_timing(self.h, 1 if enable else 0))

    def kernel_times(self):
        ms, n = (C.c_double * 3)(), C.c_uint64(0)
        _chk(lib().mcq_shard_kernel_times(self.h, ms, C.byref(n)))
        return [float(x) for x in ms], int(n.value)

    def stage_times(self):
        """({'S1': ms, 'X1': ms, 'S2': ms, 'X2': ms} summed over the batches, n batches)"""
        ms, n = (C.c_double * 4)(), C.c_uint64(0)
        _chk(lib().mcq_shard_stage_times(self.h, ms, C.byref(n)))
        return dict(zip(("S1", "X1", "S2", "X2"), [float(x) for x in ms])), int(n.value)

    def exchange_bytes(self):
        out = (C.c_uint64 * 8)()
        _chk(lib().mcq_shard_exchange_bytes(self.h, out))
        return dict(zip(("batches", "x1", "x2_ends", "x2_locations", "own_blocks", "rccl_ranks", "block_features", "block_locations"), [int(x) for x in out]))

    def close(self):
        if getattr(self, "h", None):
            lib().mcq_shard_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def packed_bytes(n_bases):
    return int(lib().mcq_packed_bytes(n_bases))


def pack_bases_host(bases):
    """ASCII bytes -> the packed form (numpy uint8 array of packed_bytes(len) bytes)"""
    src = np.frombuffer(bases, dtype=np.uint8) if not isinstance(bases, np.ndarray) else np.ascontiguousarray(bases, np.uint8)
    out = np.zeros(packed_bytes(len(src)), np.uint8)
    _chk(lib().mcq_pack_bases(_np_ptr(src) if len(src) else None, len(src), _np_ptr(out), 0, None))
    return out


def pack_bases_device(bases_ptr, n_bases, out_ptr, stream=None):
    _chk(lib().mcq_pack_bases(bases_ptr, n_bases, out_ptr, MCQ_DEVICE_PTRS, stream))


def bucket_features(features_ptr, n, n_shards, counts_ptr, bucketed_ptr, src_index_ptr, stream=None):
    _chk(lib().mcq_bucket_features(features_ptr, n, n_shards, counts_ptr, bucketed_ptr, src_index_ptr, stream))


def _build_desc(bases_ptr, seq_off_ptr, tgt2tax_ptr, n_targets, emulate_ranks, k, sketch_size, winlen, winstride,
                max_locs, n_shards, shard_id, device, flags, device_ptrs):
    d = BuildDesc()
    d.k, d.sketch_size, d.winlen, d.winstride, d.n_targets = k, sketch_size, winlen, winstride, n_targets
    d.bases, d.seq_off, d.tgt2tax = bases_ptr, seq_off_ptr, tgt2tax_ptr
    d.emulate_ranks, d.max_locs, d.n_shards, d.shard_id, d.device = emulate_ranks, max_locs, n_shards, shard_id, device
    d.flags = flags | (MCQ_DEVICE_PTRS if device_ptrs else 0)
    return d


class Table:
    """mcq_build_table: keys / list_off / locs of the union table as device arrays"""

    def __init__(self, bases_ptr, seq_off_ptr, n_targets, emulate_ranks=1, k=16, sketch_size=16, winlen=128, winstride=113,
                 max_locs=0, device=0, device_ptrs=True, flags=0):
        d = _build_desc(bases_ptr, seq_off_ptr, None, n_targets, emulate_ranks, k, sketch_size, winlen, winstride,
                        max_locs, 1, 0, device, flags, device_ptrs)
        h = C.c_void_p()
        rc = lib().mcq_build_table(C.byref(d), C.byref(h))
        if rc != 0:
            raise McqError(rc, (lib().mcq_build_last_error() or b"").decode())
        self._adopt(h, n_targets, device)

    def _adopt(self, h, n_targets, device):
        self.h, self.n_targets, self.device = h, n_targets, device
        nk, nl = C.c_uint64(), C.c_uint64()
        pk, po, pl, pw = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        _chk(lib().mcq_table_info(h, C.cast(C.byref(nk), C.c_void_p), C.cast(C.byref(nl), C.c_void_p),
                                  C.cast(C.byref(pk), C.c_void_p), C.cast(C.byref(po), C.c_void_p),
                                  C.cast(C.byref(pl), C.c_void_p), C.cast(C.byref(pw), C.c_void_p)))
        self.n_keys, self.n_locs = int(nk.value), int(nl.value)
        self.keys_ptr, self.list_off_ptr, self.locs_ptr, self.win_off_ptr = pk.value, po.value, pl.value, pw.value

    def to_host(self):
        """(keys u32, list_off u64, locs u64, win_off u64) as numpy arrays (hipMemcpy device -> host)"""
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

        def pull(ptr, n, dt):
            out = np.empty(n, dt)
            if n and hip.hipMemcpy(_np_ptr(out), ptr, out.nbytes, 2) != 0:      # hipMemcpyDeviceToHost
                raise McqError(MCQ_E_HIP, "hipMemcpy of a table array failed")
            return out
        return (pull(self.keys_ptr, self.n_keys, np.uint32), pull(self.list_off_ptr, self.n_keys + 1, np.uint64),
                pull(self.locs_ptr, self.n_locs, np.uint64), pull(self.win_off_ptr, self.n_targets + 1, np.uint64))

    def rank_split(self, n_ranks, rank):
        """mcq_table_rank_split: the table of reference rank `rank` of `n_ranks` (targets with tgt % n_ranks == rank), cut out of
        this union table on the device -- a Table of its own"""
        h = C.c_void_p()
        rc = lib().mcq_table_rank_split(self.h, n_ranks, rank, C.byref(h))
        if rc != 0:
            raise McqError(rc, (lib().mcq_build_last_error() or b"").decode())
        t = Table.__new__(Table)
        t._adopt(h, self.n_targets, self.device)
        return t

    def remove_ambiguous(self, tgt_key, max_keys=1, n_targets=None):
        """mcq_table_remove_ambiguous (-remove-ambig-features): (the table without the keys whose list names more than `max_keys`
        distinct tgt_key[target], number of keys dropped).  tgt_key: a numpy array (u32 [n_targets], host), or a raw device
        pointer (int) to that many words; n_targets defaults to the table's."""
        n = self.n_targets if n_targets is None else n_targets
        if isinstance(tgt_key, int):
            ptr, flags = C.c_void_p(tgt_key), MCQ_DEVICE_PTRS
        elif tgt_key is None:
            ptr, flags = None, 0
        else:
            keep = np.ascontiguousarray(tgt_key, np.uint32)
            if n_targets is None:
                n = len(keep)
            ptr, flags = _np_ptr(keep), 0
        h, removed = C.c_void_p(), C.c_uint64()
        rc = lib().mcq_table_remove_ambiguous(self.h, ptr, n, max_keys, flags, C.byref(h), C.byref(removed))
        if rc != 0:
            raise McqError(rc, (lib().mcq_build_last_error() or b"").decode())
        t = Table.__new__(Table)
        t._adopt(h, self.n_targets, self.device)
        return t, int(removed.value)

    def tgt_windows(self):
        """windows of every target (u32 [n_targets])"""
        out = np.zeros(self.n_targets, np.uint32)
        _chk(lib().mcq_table_tgt_windows(self.h, _np_ptr(out)))
        return out

    def shard_records_into(self, n_ranks, rank, out_ptr, cap_bytes):
        """mcq_table_shard_records as the header has it: the key records of reference rank `rank` as file bytes at the device
        pointer out_ptr (None: the sizes only) -> (n_bytes, n_keys, n_locs)"""
        nb, nk, nl = C.c_uint64(), C.c_uint64(), C.c_uint64()
        rc = lib().mcq_table_shard_records(self.h, n_ranks, rank, out_ptr, cap_bytes, C.byref(nb), C.byref(nk), C.byref(nl))
        if rc != 0:
            raise McqError(rc, (lib().mcq_build_last_error() or b"").decode())
        return int(nb.value), int(nk.value), int(nl.value)

    def shard_records(self, n_ranks, rank):
        """the key records of reference rank `rank` of `n_ranks` as the bytes of its shard file (numpy uint8): what
        host.ShardWriter.append takes, with the sizes shard_records_into(n_ranks, rank, None, 0) gives"""
        n_bytes = self.shard_records_into(n_ranks, rank, None, 0)[0]
        out = np.empty(n_bytes, np.uint8)
        if not n_bytes:
            return out
        hip = C.CDLL("libamdhip64.so")
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipFree.argtypes = [C.c_void_p]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        dev = C.c_void_p()
        if hip.hipMalloc(C.byref(dev), n_bytes) != 0:
            raise McqError(MCQ_E_HIP, "hipMalloc of the record block failed")
        try:
            self.shard_records_into(n_ranks, rank, dev, n_bytes)
            if hip.hipMemcpy(_np_ptr(out), dev, n_bytes, 2) != 0:       # hipMemcpyDeviceToHost
                raise McqError(MCQ_E_HIP, "hipMemcpy of the record block failed")
        finally:
            hip.hipFree(dev)
        return out

    def close(self):
        if getattr(self, "h", None):
            lib().mcq_table_free(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Parts:
    """mcq_build_parts: the table built in feature-hash ranges and kept as keys / list lengths / 32-bit global-window words
    (device memory) -- for tables whose one-piece build does not fit (RefSeq scale).  database() makes the queryable
    handle (any shard of it); the sequences may be released before that."""

    def __init__(self, bases_ptr, seq_off_ptr, n_targets, emulate_ranks=1, k=16, sketch_size=16, winlen=128, winstride=113,
                 max_locs=0, n_shards=1, shard_id=0, device=0, flags=0):
        d = _build_desc(bases_ptr, seq_off_ptr, None, n_targets, emulate_ranks, k, sketch_size, winlen, winstride,
                        max_locs, n_shards, shard_id, device, flags, True)
        h = C.c_void_p()
        rc = lib().mcq_build_parts(C.byref(d), C.byref(h))
        if rc != 0:
            raise McqError(rc, (lib().mcq_build_last_error() or b"").decode())
        self.h, self.n_targets, self.device = h, n_targets, device
        self.k, self.sketch_size, self.winlen, self.winstride = k, sketch_size, winlen, winstride
        nk, nl, nw, nb = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        npar = C.c_uint32()
        _chk(lib().mcq_parts_info(h, C.byref(nk), C.byref(nl), C.byref(nw), C.byref(npar), C.byref(nb)))
        self.n_keys, self.n_locs, self.n_windows, self.n_parts, self.bytes = int(nk.value), int(nl.value), int(nw.value), int(npar.value), int(nb.value)

    def database(self, tgt2tax_ptr, n_shards=1, shard_id=0, flags=0, device_ptrs=True):
        db = Database.__new__(Database)
        db.k, db.sketch_size, db.winlen, db.winstride, db.device = self.k, self.sketch_size, self.winlen, self.winstride, self.device
        h = C.c_void_p()
        rc = lib().mcq_db_from_parts(self.h, tgt2tax_ptr, n_shards, shard_id, flags | (MCQ_DEVICE_PTRS if device_ptrs else 0), C.byref(h))
        if rc != 0:
            raise McqError(rc, (lib().mcq_build_last_error() or b"").decode())
        db.h = h
        return db

    def close(self):
        if getattr(self, "h", None):
            lib().mcq_parts_free(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RangeBuild:
    """mcq_range_build_*: the union table of Table(...) built one feature-hash range at a time -- an iterator of Table, each
    holding the keys of its range in ascending feature order with the lists of the one-piece build.  n_ranges = 0 lets the
    library derive the count from the free device memory.  The sequences (device pointers) must outlive the object."""

    def __init__(self, bases_ptr, seq_off_ptr, n_targets, n_ranges=0, emulate_ranks=1, k=16, sketch_size=16, winlen=128, winstride=113,
                 max_locs=0, device=0, flags=0):
        d = _build_desc(bases_ptr, seq_off_ptr, None, n_targets, emulate_ranks, k, sketch_size, winlen, winstride,
                        max_locs, 1, 0, device, flags, True)
        h = C.c_void_p()
        rc = lib().mcq_range_build_create(C.byref(d), n_ranges, C.byref(h))
        if rc != 0:
            raise McqError(rc, (lib().mcq_build_last_error() or b"").decode())
        self.h, self.n_targets, self.device = h, n_targets, device
        nr, nx, nw = C.c_uint32(), C.c_uint32(), C.c_uint64()
        _chk(lib().mcq_range_build_info(h, C.byref(nr), C.byref(nx), C.byref(nw)))
        self.n_ranges, self.n_windows = int(nr.value), int(nw.value)

    def tgt_windows(self):
        """windows of every target (u32 [n_targets])"""
        out = np.zeros(self.n_targets, np.uint32)
        _chk(lib().mcq_range_build_tgt_windows(self.h, _np_ptr(out)))
        return out

    def __iter__(self):
        return self

    def __next__(self):
        h = C.c_void_p()
        rc = lib().mcq_range_build_next(self.h, C.byref(h))
        if rc != 0:
            raise McqError(rc, (lib().mcq_build_last_error() or b"").decode())
        if not h.value:
            raise StopIteration
        t = Table.__new__(Table)
        t._adopt(h, self.n_targets, self.device)
        return t

    def close(self):
        if getattr(self, "h", None):
            lib().mcq_range_build_free(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PartsBuilder:
    """mcq_parts_builder_*: table parts from streamed (feature, target, window) triples -- the reference's shard files without a
    host-side union (host.RefDb(meta_only=True).stream() feeds it).  finish() returns a Parts object."""

    def __init__(self, tgt_windows, k=16, sketch_size=16, winlen=128, winstride=113, tgt_winstride=0, expected_locations=0, n_ranges=0,
                 n_shards=1, shard_id=0, device=0):
        tw = np.ascontiguousarray(tgt_windows, np.uint32)
        d = PartsBuilderDesc(k, sketch_size, winlen, winstride, tgt_winstride, len(tw), tw.ctypes.data_as(C.c_void_p), expected_locations,
                             n_ranges, n_shards, shard_id, device)
        h = C.c_void_p()
        rc = lib().mcq_parts_builder_create(C.byref(d), C.byref(h))
        if rc != 0:
            raise McqError(rc, (lib().mcq_build_last_error() or b"").decode())
        self.h, self.n_targets, self.device = h, len(tw), device
        self.k, self.sketch_size, self.winlen, self.winstride = k, sketch_size, winlen, winstride

    def add(self, feat, tgt, win):
        f, t, w = (np.ascontiguousarray(x, np.uint32) for x in (feat, tgt, win))
        rc = lib().mcq_parts_builder_add(self.h, f.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), len(f), 0)
        if rc != 0:
            raise McqError(rc, (lib().mcq_build_last_error() or b"").decode())

    def set_bucket_limit(self, keep_first=0, remove_above=0):
        """mcq_parts_builder_set_bucket_limit: from now on add() applies the query-time bucket rules (bucket_limit below) to every
        chunk on the device before its append; every chunk must then hold whole key records of one shard file"""
        rc = lib().mcq_parts_builder_set_bucket_limit(self.h, keep_first, remove_above)
        if rc != 0:
            raise McqError(rc, (lib().mcq_build_last_error() or b"").decode())

    def bucket_counts(self):
        """(buckets shrunk, buckets removed) over the chunks added so far"""
        a, b = C.c_uint64(), C.c_uint64()
        rc = lib().mcq_parts_builder_bucket_counts(self.h, C.byref(a), C.byref(b))
        if rc != 0:
            raise McqError(rc, (lib().mcq_build_last_error() or b"").decode())
        return int(a.value), int(b.value)

    def finish(self):
        ph = C.c_void_p()
        rc = lib().mcq_parts_builder_finish(self.h, C.byref(ph))
        self.h = None if rc == 0 else self.h
        if rc != 0:
            raise McqError(rc, (lib().mcq_build_last_error() or b"").decode())
        p = Parts.__new__(Parts)
        p.h, p.n_targets, p.device = ph, self.n_targets, self.device
        p.k, p.sketch_size, p.winlen, p.winstride = self.k, self.sketch_size, self.winlen, self.winstride
        nk, nl, nw, nb = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        npar = C.c_uint32()
        _chk(lib().mcq_parts_info(ph, C.byref(nk), C.byref(nl), C.byref(nw), C.byref(npar), C.byref(nb)))
        p.n_keys, p.n_locs, p.n_windows, p.n_parts, p.bytes = int(nk.value), int(nl.value), int(nw.value), int(npar.value), int(nb.value)
        return p

    def close(self):
        if getattr(self, "h", None):
            lib().mcq_parts_builder_free(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bucket_limit(feat, tgt, win, keep_first=0, remove_above=0, n=None, device=0, stream=None):
    """mcq_bucket_limit: the query-time bucket rules on a chunk of (feature, target, window) triples -- a maximal run of equal `feat`
    is one bucket; one of more than remove_above locations goes, then one of more than keep_first keeps its first keep_first (0: rule
    off).  Host form (n is None): three numpy u32 arrays in, (feat, tgt, win, n_shrunk, n_removed) out, the arrays cut to what
    stays.  Device form: three raw device pointers and the count n; the call only enqueues on `stream` and returns the three
    ctypes counts (n_out, n_shrunk, n_removed), to be read (.value) after the caller has synchronised the stream."""
    no, ns, nr = C.c_uint64(), C.c_uint64(), C.c_uint64()
    if n is None:
        f, t, w = (np.array(x, np.uint32, copy=True) for x in (feat, tgt, win))
        ptrs = [x.ctypes.data_as(C.c_void_p) if len(x) else None for x in (f, t, w)]
        rc = lib().mcq_bucket_limit(ptrs[0], ptrs[1], ptrs[2], len(f), keep_first, remove_above, 0, device, stream, C.byref(no), C.byref(ns), C.byref(nr))
        _chk(rc)
        k = int(no.value)
        return f[:k], t[:k], w[:k], int(ns.value), int(nr.value)
    ptrs = [C.c_void_p(int(x)) if x else None for x in (feat, tgt, win)]
    _chk(lib().mcq_bucket_limit(ptrs[0], ptrs[1], ptrs[2], n, keep_first, remove_above, MCQ_DEVICE_PTRS, device, stream, C.byref(no), C.byref(ns), C.byref(nr)))
    return no, ns, nr


def bucket_limit_scratch_bytes(n):
    return int(lib().mcq_bucket_limit_scratch_bytes(n))


def bucket_limit_ws(feat_ptr, tgt_ptr, win_ptr, n, keep_first, remove_above, scratch_ptr, scratch_bytes, device=0, stream=None):
    """mcq_bucket_limit_ws: the device form of bucket_limit with the caller's scratch (bucket_limit_scratch_bytes(n) bytes of device
    memory): nothing is allocated.  Returns a ctypes array of three counts -- kept, buckets shrunk, buckets removed -- to be read
    after the caller has synchronised the stream."""
    counts = (C.c_uint64 * 3)()
    _chk(lib().mcq_bucket_limit_ws(C.c_void_p(int(feat_ptr)) if feat_ptr else None, C.c_void_p(int(tgt_ptr)) if tgt_ptr else None,
                                   C.c_void_p(int(win_ptr)) if win_ptr else None, n, keep_first, remove_above, device, stream,
                                   C.c_void_p(int(scratch_ptr)) if scratch_ptr else None, scratch_bytes, counts))
    return counts


class ContentStats:
    """mcq_content_stats_*: bucket size statistics and locations per target over chunks of (feature, target, window) triples -- a
    maximal run of equal `feat` is one bucket (host.RefDb(meta_only=True).stream() yields such chunks).  add() takes three numpy
    arrays (win may be None) or three device tensors (anything with data_ptr(): 4-byte integers, contiguous, ready on the null
    stream); totals() gives a dict (n_buckets, n_locations, sum2, sum3, max_size, hist[256]) since create or the last reset();
    target_locations() the locations per target since create -- reset() keeps them."""

    def __init__(self, n_targets):
        h = C.c_void_p()
        _chk(lib().mcq_content_stats_create(n_targets, C.byref(h)))
        self.h, self.n_targets = h, n_targets

    def add(self, feat, tgt, win=None):
        if hasattr(feat, "data_ptr"):
            n = int(feat.numel())
            for x in (feat, tgt):
                if not x.is_cuda or x.element_size() != 4 or not x.is_contiguous() or int(x.numel()) != n:
                    raise ValueError("ContentStats.add: device tensors of 4-byte integers, contiguous, of one length")
            ptrs, flags = [C.c_void_p(x.data_ptr()) if n else None for x in (feat, tgt)], MCQ_DEVICE_PTRS
        else:
            f, t = (np.ascontiguousarray(x, np.uint32) for x in (feat, tgt))
            if len(f) != len(t):
                raise ValueError("ContentStats.add: feat and tgt differ in length")
            n, ptrs, flags = len(f), [x.ctypes.data_as(C.c_void_p) if len(x) else None for x in (f, t)], 0
        _chk(lib().mcq_content_stats_add(self.h, ptrs[0], ptrs[1], None, n, flags))

    def totals(self):
        t = ContentTotals()
        _chk(lib().mcq_content_stats_totals(self.h, C.byref(t)))
        return t.as_dict()

    def target_locations(self):
        out = np.zeros(self.n_targets, np.uint64)
        _chk(lib().mcq_content_stats_target_locations(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def reset(self):
        _chk(lib().mcq_content_stats_reset(self.h))

    def close(self):
        if getattr(self, "h", None):
            lib().mcq_content_stats_free(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# mcq_target_coverage: one record per target (host.COVERAGE_DTYPE is the same)
COVERAGE_DTYPE = np.dtype([("hits", "<u8"), ("queries", "<u8"), ("windows_covered", "<u4"), ("reserved", "<u4")])


class Coverage:
    """mcq_coverage_*: window coverage per reference sequence, added up on the device over all batches of a run.  add() takes
    mcq_target_hits' device outputs as they are (pointers, or anything with data_ptr()) and only enqueues; read() returns a record
    array of COVERAGE_DTYPE, one per target, and the number of ranges that were refused; reset() zeroes everything."""

    def __init__(self, windows, device=0):
        w = np.ascontiguousarray(windows, np.uint32)
        h = C.c_void_p()
        _chk(lib().mcq_coverage_create(w.ctypes.data_as(C.c_void_p) if len(w) else None, len(w), device, C.byref(h)))
        self.h, self.n_targets = h, len(w)

    def add(self, ranges, counts, n_queries, n_slots, range_cap, stream=None):
        ptr = [C.c_void_p(int(x.data_ptr() if hasattr(x, "data_ptr") else x)) if n_queries else None for x in (ranges, counts)]
        _chk(lib().mcq_coverage_add(self.h, ptr[0], ptr[1], n_queries, n_slots, range_cap, stream))

    def read(self, stream=None):
        out = np.zeros(self.n_targets, COVERAGE_DTYPE)
        oor = C.c_uint64(0)
        _chk(lib().mcq_coverage_read(self.h, out.ctypes.data_as(C.c_void_p), C.byref(oor), stream))
        return out, int(oor.value)

    def bitmap(self, stream=None):
        """(words, word_off): the bitmap with its two guard words -- segment t is words[1 + word_off[t] : 1 + word_off[t + 1]]"""
        words = np.zeros(int(lib().mcq_coverage_bitmap_words(self.h)), np.uint32)
        off = np.zeros(self.n_targets + 1, np.uint64)
        _chk(lib().mcq_coverage_bitmap(self.h, words.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p), stream))
        return words, off

    def reset(self, stream=None):
        _chk(lib().mcq_coverage_reset(self.h, stream))

    def close(self):
        if getattr(self, "h", None):
            lib().mcq_coverage_free(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TableExtend:
    """mcq_table_extend_*: the locations of an existing database (chunks of (feature, target, window) triples, as
    host.RefDb(meta_only=True).stream() yields them) and new sequences through the build pipeline together -- `modify`.
    finish() returns a Table of the old and the new targets."""

    def __init__(self, old_tgt_windows, n_ranks=1, k=16, sketch_size=16, winlen=128, winstride=113, max_locs=0, flags=0,
                 expected_old_locations=0, device=0):
        tw = np.ascontiguousarray(old_tgt_windows, np.uint32)
        d = TableExtendDesc(k, sketch_size, winlen, winstride, n_ranks, max_locs, flags, device, len(tw),
                            tw.ctypes.data_as(C.c_void_p) if len(tw) else None, expected_old_locations)
        h = C.c_void_p()
        rc = lib().mcq_table_extend_create(C.byref(d), C.byref(h))
        if rc != 0:
            raise McqError(rc, (lib().mcq_build_last_error() or b"").decode())
        self.h, self.n_old_targets, self.device = h, len(tw), device

    def add(self, feat, tgt, win, n=None):
        """a chunk: three numpy u32 arrays (host), or three raw device pointers (int) and the count n"""
        if n is None:
            f, t, w = (np.ascontiguousarray(x, np.uint32) for x in (feat, tgt, win))
            ptrs, n, flags = [x.ctypes.data_as(C.c_void_p) for x in (f, t, w)], len(f), 0
        else:
            ptrs, flags = [C.c_void_p(int(x)) for x in (feat, tgt, win)], MCQ_DEVICE_PTRS
        rc = lib().mcq_table_extend_add(self.h, ptrs[0], ptrs[1], ptrs[2], n, flags)
        if rc != 0:
            raise McqError(rc, (lib().mcq_build_last_error() or b"").decode())

    def finish(self, bases_ptr, seq_off_ptr, n_new_targets, device_ptrs=True):
        th = C.c_void_p()
        rc = lib().mcq_table_extend_finish(self.h, bases_ptr, seq_off_ptr, n_new_targets, MCQ_DEVICE_PTRS if device_ptrs else 0, C.byref(th))
        if rc != 0:
            raise McqError(rc, (lib().mcq_build_last_error() or b"").decode())
        self.h = None                                           # (released by the call)
        t = Table.__new__(Table)
        t._adopt(th, self.n_old_targets + n_new_targets, self.device)
        return t

    def close(self):
        if getattr(self, "h", None):
            lib().mcq_table_extend_free(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


MCQ_ACCMAP_MAX_LINE = 1024
MCQ_ACCMAP_RULE_TARGETS, MCQ_ACCMAP_RULE_ACC, MCQ_ACCMAP_RULE_ACCVER, MCQ_ACCMAP_RULE_GI = 0, 1, 2, 3


def sorted_names(names):
    """the names of the targets (bytes, target t at index t) as mcq_accmap_create and host.accmap_host take them: (blob, name_off,
    name_target), ascending as std::string compares (Python's bytes compare the same way), a name that occurs twice kept once"""
    order = sorted(range(len(names)), key=lambda t: (names[t], t))
    keep = [t for i, t in enumerate(order) if i == 0 or names[t] != names[order[i - 1]]]
    off = np.zeros(len(keep) + 1, np.uint64)
    off[1:] = np.cumsum([len(names[t]) for t in keep])
    return b"".join(names[t] for t in keep), off, np.asarray(keep, np.uint32)


class AccMap:
    """mcq_accmap_*: *.accession2taxid text joined against the names of a database's targets on the GPU.  names: the target names
    (bytes; target t at index t); unranked: per target, non-zero where it has no parent.  chunk() takes whole lines of one file in
    DEVICE memory (a pointer and a byte count, or a torch uint8 tensor on the GPU) and returns whether the chunk was strict (and so
    applied); finish() returns (parent int64[n_targets], found bool[n_targets]).  rule: MCQ_ACCMAP_RULE_TARGETS (a build's three
    lookups) or _ACC / _ACCVER / _GI (the name equal to that column and nothing else: mcq_accmap_create_rule)."""

    def __init__(self, names, unranked, device=0, rule=MCQ_ACCMAP_RULE_TARGETS):
        blob, off, tgt = sorted_names([bytes(n) for n in names])
        u = np.ascontiguousarray(unranked, np.uint8)
        assert len(u) == len(names)
        h = C.c_void_p()
        _chk(lib().mcq_accmap_create_rule(blob, _np_ptr(off), len(tgt), _np_ptr(tgt), _np_ptr(u), len(u), rule, device, C.byref(h)))
        self.h, self.n_targets = h, len(u)

    def chunk(self, text, n_bytes=None, file_ordinal=0, first_line_no=0, stream=None):
        if n_bytes is None:
            ptr, n_bytes = text.data_ptr(), text.numel()
        else:
            ptr = int(text)
        strict = C.c_uint32(0)
        _chk(lib().mcq_accmap_chunk(self.h, C.c_void_p(ptr), n_bytes, file_ordinal, first_line_no, C.byref(strict), stream))
        return bool(strict.value)

    def finish(self):
        parent, found = np.zeros(self.n_targets, np.int64), np.zeros(self.n_targets, np.uint8)
        _chk(lib().mcq_accmap_finish(self.h, _np_ptr(parent), _np_ptr(found)))
        return parent, found.astype(bool)

    def close(self):
        if getattr(self, "h", None):
            lib().mcq_accmap_free(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


MCQ_MERGE_MAX_LINE = 4096
MCQ_MERGE_MAX_ITEMS = 64


class Merge:
    """mcq_merge_*: the reference's `merge` of query result files on the GPU.  tax: a Taxonomy on `device` (kept alive by this
    object); table: (taxon ids strictly ascending, taxon index of each) as host.taxid_table(db) gives it.  chunk() takes whole lines
    of one file in DEVICE memory (a pointer and a byte count, or a torch uint8 tensor on the GPU) and returns whether the chunk was
    strict (and so applied); lines() takes parsed lines; lists() returns (n_cand u32 [n_queries], pairs u32 [n_queries, max_cand, 2],
    number of items with an unknown taxid); finish() returns (best u32 [n_queries], counts u64 [n_taxa + 1])."""

    def __init__(self, tax, table, n_queries, max_cand=2, merge_below_rank=4, device=0):
        self._ids, self._idx = np.ascontiguousarray(table[0], np.int64), np.ascontiguousarray(table[1], np.uint32)
        assert len(self._ids) == len(self._idx)
        h = C.c_void_p()
        _chk(lib().mcq_merge_create(tax.h, _np_ptr(self._ids), _np_ptr(self._idx), len(self._ids), n_queries, max_cand, merge_below_rank,
                                    device, C.byref(h)))
        self.h, self.tax, self.n_queries, self.max_cand, self.device = h, tax, n_queries, max_cand, device

    def chunk(self, text, n_bytes=None, file_ordinal=0, chunk_offset=0, tophits_column=2, stream=None):
        if n_bytes is None:
            ptr, n_bytes = text.data_ptr(), text.numel()
        else:
            ptr = int(text)
        strict = C.c_int32(0)
        _chk(lib().mcq_merge_chunk(self.h, C.c_void_p(ptr), n_bytes, file_ordinal, chunk_offset, tophits_column, C.byref(strict), stream))
        return bool(strict.value)

    def lines(self, line_query, item_off, taxid, hits, header_off=None, header_len=None, file_ordinal=0, stream=None):
        """parsed lines (host arrays): line l names query line_query[l] (0-based) and holds the items [item_off[l], item_off[l + 1])"""
        q = np.ascontiguousarray(line_query, np.uint32)
        off, t, h = np.ascontiguousarray(item_off, np.uint64), np.ascontiguousarray(taxid, np.int64), np.ascontiguousarray(hits, np.uint32)
        ho = np.zeros(len(q), np.uint64) if header_off is None else np.ascontiguousarray(header_off, np.uint64)
        hl = np.zeros(len(q), np.uint32) if header_len is None else np.ascontiguousarray(header_len, np.uint32)
        assert len(off) == len(q) + 1 and len(t) == len(h) == int(off[-1]) and len(ho) == len(hl) == len(q)
        _chk(lib().mcq_merge_lines(self.h, _np_ptr(q), _np_ptr(off), _np_ptr(t), _np_ptr(h), _np_ptr(ho), _np_ptr(hl), len(q), file_ordinal, 0, stream))

    def lines_cut(self, line_query, item_off, taxid, hits, header_off, header_len, file_ordinal=0, stream=None):
        """lines() for lines in which a query may repeat (what host.merge_host gives): one call per run of distinct queries"""
        seen, first = set(), 0
        for l in range(len(line_query) + 1):
            if l == len(line_query) or int(line_query[l]) in seen:
                a, b = int(item_off[first]), int(item_off[l])
                self.lines(line_query[first:l], np.asarray(item_off[first:l + 1], np.uint64) - np.uint64(a), taxid[a:b], hits[a:b],
                           header_off[first:l], header_len[first:l], file_ordinal, stream)
                seen, first = set(), l
            if l < len(line_query):
                seen.add(int(line_query[l]))

    def lists(self):
        n, pairs = np.zeros(self.n_queries, np.uint32), np.zeros((self.n_queries, self.max_cand, 2), np.uint32)
        unknown = C.c_uint64(0)
        _chk(lib().mcq_merge_lists(self.h, _np_ptr(n), _np_ptr(pairs), C.byref(unknown)))
        return n, pairs, int(unknown.value)

    def headers(self):
        f, o, l = np.zeros(self.n_queries, np.uint32), np.zeros(self.n_queries, np.uint64), np.zeros(self.n_queries, np.uint32)
        _chk(lib().mcq_merge_headers(self.h, _np_ptr(f), _np_ptr(o), _np_ptr(l)))
        return f, o, l

    def finish(self, hits_min=5, hits_diff_fraction=1.0, highest_rank=19, stream=None):
        import torch
        dev = "cuda:%d" % self.device                          # (the handle's device, whatever torch's current one is)
        best = torch.zeros(max(1, self.n_queries), dtype=torch.int32, device=dev)
        counts = torch.zeros(self.tax.n_taxa + 1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        o = ClassifyOpts(hits_min, hits_diff_fraction, highest_rank, 0)
        _chk(lib().mcq_merge_finish(self.h, C.byref(o), C.c_void_p(best.data_ptr()), C.c_void_p(counts.data_ptr()), stream))
        torch.cuda.synchronize(dev)
        return best.cpu().numpy().view(np.uint32)[:self.n_queries], counts.cpu().numpy().view(np.uint64)

    def close(self):
        if getattr(self, "h", None):
            lib().mcq_merge_free(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fastq_index(text_ptr, n_bytes, ranges_ptr, max_seqs, n_seqs_ptr, stream=None):
    """raw FASTQ text in HBM -> (begin,end) ranges of the sequence lines (device buffers)"""
    _chk(lib().mcq_fastq_index(text_ptr, n_bytes, ranges_ptr, max_seqs, n_seqs_ptr, stream))


def fasta_index(text_ptr, n_bytes, ranges_ptr, max_seqs, n_seqs_ptr, stream=None):
    """the same for FASTA text with one sequence line per record"""
    _chk(lib().mcq_fasta_index(text_ptr, n_bytes, ranges_ptr, max_seqs, n_seqs_ptr, stream))


MCQ_READS_EOF1, MCQ_READS_EOF2, MCQ_READS_NOT_STRICT = 1, 2, 1
MCQ_READS_INTERLEAVED = 4
MCQ_READS_INFO_WORDS = 8


def reads_scratch_bytes(len1, len2, max_queries):
    return int(lib().mcq_reads_scratch_bytes(len1, len2, max_queries))


def reads_prepare(text1_ptr, len1, text2_ptr, len2, flags, max_queries, max_bases, scratch_ptr, scratch_bytes,
                  bases_ptr, seq_off_ptr, hdr_ptr, info_ptr, stream=None):
    """one chunk of FASTQ / FASTA text per file in HBM (text2_ptr None: single-end) -> compacted bases, seq_off, header
    ranges and info[MCQ_READS_INFO_WORDS] (device buffers; include/mcq.h mcq_reads_prepare)"""
    _chk(lib().mcq_reads_prepare(text1_ptr, len1, text2_ptr, len2, flags, max_queries, max_bases, scratch_ptr, scratch_bytes,
                                 bases_ptr, seq_off_ptr, hdr_ptr, info_ptr, stream))


def owner(feature, n_shards):
    return int(lib().mcq_owner(feature, n_shards))


def target_slots(cands_ptr, ncand_ptr, n_queries, max_cand, hits_min, tax2tgt_ptr, n_taxa, targets_ptr, n_slots, stream=None):
    """mcq_target_slots: the slot targets of a batch from its device results (sequence-level candidates with hits >= hits_min)"""
    r = Result(cands_ptr, ncand_ptr, MCQ_DEVICE_PTRS)
    _chk(lib().mcq_target_slots(C.byref(r), n_queries, max_cand, hits_min, tax2tgt_ptr, n_taxa, targets_ptr, n_slots, stream))
