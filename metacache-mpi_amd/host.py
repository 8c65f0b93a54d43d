"""ctypes mirror of include/mcq_host.h (reference shard reader, taxonomy keys, classify)."""
import ctypes as C
import os

import numpy as np

from .build import host_lib_path

NO_TAXON = 0xFFFFFFFF
RANK_SEQUENCE, RANK_SPECIES, RANK_ROOT, RANK_NONE = 0, 4, 20, 21


class Info(C.Structure):
    _fields_ = [("k", C.c_uint32), ("sketch_size", C.c_uint32), ("winlen", C.c_uint32), ("winstride", C.c_uint32),
                ("q_sketch_size", C.c_uint32), ("q_winlen", C.c_uint32), ("q_winstride", C.c_uint32),
                ("max_locs_per_feature", C.c_uint32), ("n_ranks", C.c_uint32), ("n_targets", C.c_uint32),
                ("n_taxa", C.c_uint32), ("n_keys", C.c_uint64), ("n_locs", C.c_uint64)]


class TaxonRec(C.Structure):
    _fields_ = [("id", C.c_int64), ("parent", C.c_int64), ("rank", C.c_uint8), ("name", C.c_char_p), ("file", C.c_char_p),
                ("index", C.c_uint64), ("windows", C.c_uint64)]


class EvalStatsRec(C.Structure):
    _fields_ = [(n, C.c_uint64 * 22) for n in ("assigned", "known", "correct", "wrong")]


class TaxonPrint(C.Structure):
    _fields_ = [("show_ranks", C.c_uint32), ("body", C.c_uint32), ("lineage", C.c_uint32), ("lowest_rank", C.c_uint32),
                ("highest_rank", C.c_uint32)]


class ShardParams(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("k", "sketch_size", "winlen", "winstride", "q_k", "q_sketch_size", "q_winlen",
                                         "q_winstride", "max_locs_per_feature")]


_lib = None


def _taxon_array(taxa):
    """(TaxonRec array, the byte strings it points into) of a list of dicts (id, parent, rank, name, file, index, windows)"""
    arr = (TaxonRec * max(1, len(taxa)))()
    keep = []
    for i, t in enumerate(taxa):
        nm, fl = t["name"].encode("latin-1"), t["file"].encode("latin-1")
        keep += [nm, fl]
        arr[i] = TaxonRec(t["id"], t["parent"], t["rank"], nm, fl, t["index"], t["windows"])
    return arr, keep


def write_shard(path, params, taxa, n_targets, keys, list_off, locs):
    """mcq_refdb_write_shard.  params: dict with the ShardParams field names; taxa: list of dicts
    (id, parent, rank, name, file, index, windows); keys u32, list_off u64 [n+1], locs u64 (tgt<<32|win)."""
    sp = ShardParams(**{k: int(v) for k, v in params.items()})
    arr, keep = _taxon_array(taxa)
    keys = np.ascontiguousarray(keys, np.uint32); list_off = np.ascontiguousarray(list_off, np.uint64)
    locs = np.ascontiguousarray(locs, np.uint64)
    rc = lib().mcq_refdb_write_shard(path.encode(), C.byref(sp), arr, len(taxa), n_targets, keys.ctypes.data_as(C.c_void_p),
                                     list_off.ctypes.data_as(C.c_void_p), locs.ctypes.data_as(C.c_void_p), len(keys))
    if rc != 0:
        raise RuntimeError(lib().mcq_host_last_error().decode())


class ShardWriter:
    """mcq_shard_writer_*: a shard file written in blocks -- the head of write_shard at once, then append(records, n_keys, n_locs)
    with whole key records as bytes (engine.Table.shard_records makes them), the two counts patched in by close()"""

    def __init__(self, path, params, taxa, n_targets):
        sp = ShardParams(**{k: int(v) for k, v in params.items()})
        arr, keep = _taxon_array(taxa)
        h = C.c_void_p()
        if lib().mcq_shard_writer_open(path.encode(), C.byref(sp), arr, len(taxa), n_targets, C.byref(h)) != 0:
            raise RuntimeError(lib().mcq_host_last_error().decode())
        self.h = h

    def append(self, records, n_keys, n_locs):
        rec = np.ascontiguousarray(records, np.uint8)
        if lib().mcq_shard_writer_append(self.h, rec.ctypes.data_as(C.c_void_p), rec.nbytes, n_keys, n_locs) != 0:
            raise RuntimeError(lib().mcq_host_last_error().decode())

    def close(self):
        h, self.h = getattr(self, "h", None), None
        if h and lib().mcq_shard_writer_close(h) != 0:
            raise RuntimeError(lib().mcq_host_last_error().decode())

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def lib():
    global _lib
    if _lib is None:
        p = host_lib_path()
        if not os.path.exists(p):
            raise ImportError("host library %s missing: run __graft_entry__.build()" % p)
        L = C.CDLL(p)
        L.mcq_refdb_open.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_void_p)]
        L.mcq_refdb_close.argtypes = [C.c_void_p]
        L.mcq_refdb_get_info.argtypes = [C.c_void_p, C.POINTER(Info)]
        for f, t in (("mcq_refdb_keys", C.POINTER(C.c_uint32)), ("mcq_refdb_list_off", C.POINTER(C.c_uint64)),
                     ("mcq_refdb_locs", C.POINTER(C.c_uint64))):
            getattr(L, f).restype = t; getattr(L, f).argtypes = [C.c_void_p]
        L.mcq_refdb_tgt2tax.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        L.mcq_refdb_taxon_id.restype = C.c_int64; L.mcq_refdb_taxon_id.argtypes = [C.c_void_p, C.c_uint32]
        L.mcq_refdb_taxon_rank.restype = C.c_uint32; L.mcq_refdb_taxon_rank.argtypes = [C.c_void_p, C.c_uint32]
        L.mcq_refdb_taxon_name.restype = C.c_char_p; L.mcq_refdb_taxon_name.argtypes = [C.c_void_p, C.c_uint32]
        L.mcq_refdb_ancestor.restype = C.c_uint32; L.mcq_refdb_ancestor.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        L.mcq_refdb_classify.restype = C.c_uint32
        L.mcq_refdb_classify.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_uint32]
        L.mcq_refdb_lineages.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.mcq_refdb_ground_truth.restype = C.c_uint32; L.mcq_refdb_ground_truth.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64]
        L.mcq_refdb_clade_keys.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        L.mcq_taxa_clade_keys.argtypes = [C.POINTER(TaxonRec), C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p]
        L.mcq_refdb_taxon_clade.restype = C.c_uint32; L.mcq_refdb_taxon_clade.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        L.mcq_refdb_ranked_lca.restype = C.c_uint32; L.mcq_refdb_ranked_lca.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        sp = C.POINTER(EvalStatsRec)
        L.mcq_eval_stats_assign.restype = None; L.mcq_eval_stats_assign.argtypes = [sp, C.c_uint32]
        L.mcq_eval_stats_assign_known_correct.restype = None
        L.mcq_eval_stats_assign_known_correct.argtypes = [sp, C.c_uint32, C.c_uint32, C.c_uint32]
        L.mcq_eval_stats_add.restype = None; L.mcq_eval_stats_add.argtypes = [sp, sp]
        for f in ("total", "unknown"):
            getattr(L, "mcq_eval_stats_" + f).restype = C.c_uint64; getattr(L, "mcq_eval_stats_" + f).argtypes = [sp]
        for f in ("assigned", "known", "correct", "wrong"):
            getattr(L, "mcq_eval_stats_" + f).restype = C.c_uint64; getattr(L, "mcq_eval_stats_" + f).argtypes = [sp, C.c_uint32]
        for f in ("unknown_rate", "unclassified_rate"):
            getattr(L, "mcq_eval_stats_" + f).restype = C.c_double; getattr(L, "mcq_eval_stats_" + f).argtypes = [sp]
        for f in ("known_rate", "classification_rate", "precision", "sensitivity"):
            getattr(L, "mcq_eval_stats_" + f).restype = C.c_double; getattr(L, "mcq_eval_stats_" + f).argtypes = [sp, C.c_uint32]
        L.mcq_eval_stats_text.restype = C.c_int64; L.mcq_eval_stats_text.argtypes = [sp, C.c_char_p, C.c_char_p, C.c_size_t]
        L.mcq_refdb_abundance_text.restype = C.c_int64
        L.mcq_refdb_abundance_text.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_char_p, C.c_size_t]
        L.mcq_hits_table_create.argtypes = [C.POINTER(C.c_void_p)]
        L.mcq_hits_table_add.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        L.mcq_hits_table_merge.argtypes = [C.c_void_p, C.c_void_p]
        L.mcq_hits_table_targets.restype = C.c_uint64; L.mcq_hits_table_targets.argtypes = [C.c_void_p]
        L.mcq_hits_table_entries.restype = C.c_uint64; L.mcq_hits_table_entries.argtypes = [C.c_void_p]
        L.mcq_hits_table_text.restype = C.c_int64
        L.mcq_hits_table_text.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(TaxonPrint), C.c_char_p, C.c_size_t]
        L.mcq_hits_table_free.argtypes = [C.c_void_p]
        L.mcq_refdb_seq_windows.argtypes = [C.c_void_p, C.c_void_p]
        L.mcq_coverage_cut.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_double, C.c_void_p]
        L.mcq_coverage_text.restype = C.c_int64
        L.mcq_coverage_text.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_char_p, C.c_char_p,
                                        C.POINTER(TaxonPrint), C.c_char_p, C.c_size_t]
        L.mcq_refdb_target_key.restype = C.c_uint32; L.mcq_refdb_target_key.argtypes = [C.c_void_p, C.c_uint32]
        L.mcq_refdb_tax2tgt.argtypes = [C.c_void_p, C.c_void_p]
        L.mcq_default_hits_min.restype = C.c_uint32; L.mcq_default_hits_min.argtypes = [C.c_uint32]
        L.mcq_rank_from_name.restype = C.c_uint32; L.mcq_rank_from_name.argtypes = [C.c_char_p]
        L.mcq_rank_name.restype = C.c_char_p; L.mcq_rank_name.argtypes = [C.c_uint32]
        L.mcq_host_last_error.restype = C.c_char_p
        L.mcq_refdb_write_shard.argtypes = [C.c_char_p, C.POINTER(ShardParams), C.POINTER(TaxonRec), C.c_uint64, C.c_uint32,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        L.mcq_shard_writer_open.argtypes = [C.c_char_p, C.POINTER(ShardParams), C.POINTER(TaxonRec), C.c_uint64, C.c_uint32, C.POINTER(C.c_void_p)]
        L.mcq_shard_writer_append.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64]
        L.mcq_shard_writer_close.argtypes = [C.c_void_p]
        L.mcq_refdb_open_meta.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_void_p)]
        L.mcq_refdb_tgt_windows.argtypes = [C.c_void_p, C.c_void_p]
        L.mcq_refdb_file_stats.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.mcq_shard_stream_open.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
        L.mcq_shard_stream_next.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.mcq_shard_stream_close.argtypes = [C.c_void_p]
        L.mcq_read_stream_open.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        L.mcq_read_stream_fill.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]
        L.mcq_read_stream_consume.argtypes = [C.c_void_p, C.c_uint64]
        L.mcq_read_stream_close.argtypes = [C.c_void_p]
        L.mcq_reads_parse.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mcq_refdb_taxon_parent.restype = C.c_int64; L.mcq_refdb_taxon_parent.argtypes = [C.c_void_p, C.c_uint32]
        L.mcq_refdb_taxon_file.restype = C.c_char_p; L.mcq_refdb_taxon_file.argtypes = [C.c_void_p, C.c_uint32]
        L.mcq_refdb_taxon_index.restype = C.c_uint64; L.mcq_refdb_taxon_index.argtypes = [C.c_void_p, C.c_uint32]
        L.mcq_refdb_taxon_windows.restype = C.c_uint64; L.mcq_refdb_taxon_windows.argtypes = [C.c_void_p, C.c_uint32]
        L.mcq_taxdump_read.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        L.mcq_taxdump_count.restype = C.c_uint64; L.mcq_taxdump_count.argtypes = [C.c_void_p]
        L.mcq_taxdump_taxa.restype = C.POINTER(TaxonRec); L.mcq_taxdump_taxa.argtypes = [C.c_void_p]
        L.mcq_taxdump_free.argtypes = [C.c_void_p]
        L.mcq_target_name.restype = C.c_int64; L.mcq_target_name.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_size_t]
        L.mcq_target_parent_taxid.restype = C.c_int64; L.mcq_target_parent_taxid.argtypes = [C.c_char_p, C.c_uint64]
        L.mcq_genome_files.argtypes = [C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_void_p)]
        L.mcq_file_list_count.restype = C.c_uint32; L.mcq_file_list_count.argtypes = [C.c_void_p]
        L.mcq_file_list_get.restype = C.c_char_p; L.mcq_file_list_get.argtypes = [C.c_void_p, C.c_uint32]
        L.mcq_file_list_free.argtypes = [C.c_void_p]
        L.mcq_genome_reader_open.argtypes = [C.POINTER(C.c_char_p), C.c_uint32, C.c_uint64, C.POINTER(C.c_void_p)]
        L.mcq_genome_reader_next.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]
        L.mcq_genome_reader_n_targets.restype = C.c_uint32; L.mcq_genome_reader_n_targets.argtypes = [C.c_void_p]
        L.mcq_genome_reader_target.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(TaxonRec), C.POINTER(C.c_uint64)]
        L.mcq_genome_reader_close.argtypes = [C.c_void_p]
        L.mcq_genome_reader_open_after.argtypes = [C.POINTER(C.c_char_p), C.c_uint32, C.c_uint64, C.c_void_p, C.POINTER(C.c_void_p)]
        L.mcq_genome_reader_n_skipped.restype = C.c_uint64; L.mcq_genome_reader_n_skipped.argtypes = [C.c_void_p]
        L.mcq_refdb_taxa.argtypes = [C.c_void_p, C.POINTER(TaxonRec)]
        L.mcq_seq2tax_create.argtypes = [C.POINTER(C.c_void_p)]
        L.mcq_seq2tax_add_file.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int32)]
        L.mcq_seq2tax_read.argtypes = [C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_void_p)]
        L.mcq_seq2tax_count.restype = C.c_uint64; L.mcq_seq2tax_count.argtypes = [C.c_void_p]
        L.mcq_seq2tax_entry.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_char_p), C.POINTER(C.c_int64)]
        L.mcq_seq2tax_find.restype = C.c_int64; L.mcq_seq2tax_find.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64]
        L.mcq_seq2tax_free.argtypes = [C.c_void_p]
        L.mcq_genome_reader_open_mapped.argtypes = [C.POINTER(C.c_char_p), C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        L.mcq_taxmap_files.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]
        L.mcq_accmap_host.argtypes = [C.c_char_p, C.c_uint64, C.c_int32, C.c_char_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_uint32, C.POINTER(C.c_uint64)]
        L.mcq_accmap_host_rule.argtypes = [C.c_char_p, C.c_uint64, C.c_int32, C.c_char_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]
        L.mcq_annotate_id.restype = C.c_int64; L.mcq_annotate_id.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_char_p, C.c_size_t]
        L.mcq_annotate_rewrite.restype = C.c_int64
        L.mcq_annotate_rewrite.argtypes = [C.c_char_p, C.c_uint64, C.c_int32, C.c_uint64, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t]
        L.mcq_refdb_from_taxdump.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.mcq_refdb_taxid_table.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
        L.mcq_results_properties.argtypes = [C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.mcq_merge_host.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_char_p, C.c_uint64, C.c_uint64] + [C.c_void_p] * 6 + \
                                    [C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        _lib = L
    return _lib


class RefDb:
    """The reference's <prefix>.db_<r> shard files, parsed and unioned on the host."""

    def __init__(self, prefix, n_ranks, meta_only=False):
        """meta_only: mcq_refdb_open_meta -- parameters and taxa only, the tables are streamed (stream())"""
        h = C.c_void_p()
        opener = lib().mcq_refdb_open_meta if meta_only else lib().mcq_refdb_open
        if opener(prefix.encode(), n_ranks, C.byref(h)) != 0:
            raise RuntimeError(lib().mcq_host_last_error().decode())
        self.h = h
        self.info = Info()
        lib().mcq_refdb_get_info(self.h, C.byref(self.info))

    def close(self):
        if getattr(self, "h", None):
            lib().mcq_refdb_close(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def tgt_windows(self):
        out = np.zeros(self.info.n_targets, np.uint32)
        if lib().mcq_refdb_tgt_windows(self.h, out.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError(lib().mcq_host_last_error().decode())
        return out

    def file_stats(self, rank):
        b, k, l = C.c_uint64(), C.c_uint64(), C.c_uint64()
        if lib().mcq_refdb_file_stats(self.h, rank, C.byref(b), C.byref(k), C.byref(l)) != 0:
            raise RuntimeError(lib().mcq_host_last_error().decode())
        return int(b.value), int(k.value), int(l.value)

    def stream(self, rank, chunk=1 << 20):
        """yields (feature, target, window) uint32 arrays, chunk by chunk in file order (meta_only handles)"""
        sh = C.c_void_p()
        if lib().mcq_shard_stream_open(self.h, rank, C.byref(sh)) != 0:
            raise RuntimeError(lib().mcq_host_last_error().decode())
        try:
            f, t, w = (np.zeros(chunk, np.uint32) for _ in range(3))
            n = C.c_uint64()
            while True:
                if lib().mcq_shard_stream_next(sh, f.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p),
                                               chunk, C.byref(n)) != 0:
                    raise RuntimeError(lib().mcq_host_last_error().decode())
                if n.value == 0:
                    return
                yield f[:n.value].copy(), t[:n.value].copy(), w[:n.value].copy()
        finally:
            lib().mcq_shard_stream_close(sh)

    def table(self):
        n, m = self.info.n_keys, self.info.n_locs
        keys = np.ctypeslib.as_array(lib().mcq_refdb_keys(self.h), shape=(n,)).copy() if n else np.zeros(0, np.uint32)
        off = np.ctypeslib.as_array(lib().mcq_refdb_list_off(self.h), shape=(n + 1,)).copy() if n else np.zeros(1, np.uint64)
        locs = np.ctypeslib.as_array(lib().mcq_refdb_locs(self.h), shape=(m,)).copy() if m else np.zeros(0, np.uint64)
        return keys, off, locs

    def tgt2tax(self, merge_below_rank):
        out = np.zeros(self.info.n_targets, np.uint32)
        if lib().mcq_refdb_tgt2tax(self.h, merge_below_rank, out.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError(lib().mcq_host_last_error().decode())
        return out

    def taxon_id(self, key):
        return int(lib().mcq_refdb_taxon_id(self.h, int(key)))

    def classify(self, cands, hits_min, hits_diff_fraction, highest_rank):
        """cands: array [n, 4] of (tax key, hits, beg, end) -> taxon index or NO_TAXON"""
        c = np.ascontiguousarray(cands, np.uint32).reshape(-1, 4)
        return int(lib().mcq_refdb_classify(self.h, c.ctypes.data_as(C.c_void_p), len(c), hits_min,
                                            C.c_float(hits_diff_fraction), highest_rank))

    def taxon_rank(self, key):
        return int(lib().mcq_refdb_taxon_rank(self.h, int(key)))

    def taxon_name(self, key):
        return lib().mcq_refdb_taxon_name(self.h, int(key)).decode("latin-1")

    def taxon_parent(self, key):
        return int(lib().mcq_refdb_taxon_parent(self.h, int(key)))

    def taxon_source(self, key):
        """(file, index, windows) of a taxon record: the source of a sequence-level taxon"""
        return (lib().mcq_refdb_taxon_file(self.h, int(key)).decode("latin-1"), int(lib().mcq_refdb_taxon_index(self.h, int(key))),
                int(lib().mcq_refdb_taxon_windows(self.h, int(key))))

    def taxa(self):
        """mcq_refdb_taxa: every taxon record in file order, as dicts (what write_shard takes), as rank 0's file holds them"""
        arr = (TaxonRec * max(1, self.info.n_taxa))()
        if lib().mcq_refdb_taxa(self.h, arr) != 0:
            raise RuntimeError(lib().mcq_host_last_error().decode())
        return [_rec(arr[i]) for i in range(self.info.n_taxa)]

    def ancestor(self, key, rank):
        return int(lib().mcq_refdb_ancestor(self.h, int(key), int(rank)))

    def ground_truth(self, header):
        """taxon index a read's header names (its next ranked ancestor), or NO_TAXON: mcq_refdb_ground_truth"""
        h = header.encode("latin-1") if isinstance(header, str) else header
        return int(lib().mcq_refdb_ground_truth(self.h, h, len(h)))

    def clade_keys(self, rank):
        """u32 [n_targets]: every target's ancestor at `rank`, 0xFFFFFFFF where it has none (Workspace.set_exclusion)"""
        out = np.zeros(self.info.n_targets, np.uint32)
        if lib().mcq_refdb_clade_keys(self.h, int(rank), out.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError(lib().mcq_host_last_error().decode())
        return out

    def taxon_clade(self, truth, rank):
        """clade key of a resolved truth at `rank` (0xFFFFFFFF: no ancestor there; 0xFFFFFFFE: no truth): one entry of Workspace.set_query_clades"""
        return int(lib().mcq_refdb_taxon_clade(self.h, int(truth), int(rank)))

    def ranked_lca(self, a, b):
        """taxon index of the ranked LCA of two taxa, NO_TAXON if either is NO_TAXON or they share no rank: mcq_refdb_ranked_lca"""
        return int(lib().mcq_refdb_ranked_lca(self.h, int(a), int(b)))

    def lineages(self):
        """(lineage u32 [n_taxa, 21], rank u8 [n_taxa]): the table mcq_taxonomy_create takes"""
        n = self.info.n_taxa
        lin = np.zeros((n, 21), np.uint32); rank = np.zeros(n, np.uint8)
        if lib().mcq_refdb_lineages(self.h, lin.ctypes.data_as(C.c_void_p), rank.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError(lib().mcq_host_last_error().decode())
        return lin, rank

    def target_key(self, target):
        return int(lib().mcq_refdb_target_key(self.h, int(target)))

    def seq_windows(self):
        """windows of every target as the -hits-per-seq table and the coverage report print them (mcq_refdb_seq_windows)"""
        out = np.zeros(self.info.n_targets, np.uint32)
        if lib().mcq_refdb_seq_windows(self.h, out.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError(lib().mcq_host_last_error().decode())
        return out

    def tax2tgt(self):
        out = np.zeros(self.info.n_taxa, np.uint32)
        lib().mcq_refdb_tax2tgt(self.h, out.ctypes.data_as(C.c_void_p))
        return out

    def abundance_text(self, counts, total, est_rank=RANK_NONE):
        """counts: u64 [n_taxa] classified queries per taxon index; est_rank RANK_NONE = the plain table, else the
        estimate to that rank (mcq_refdb_abundance_text)"""
        c = np.ascontiguousarray(counts, np.uint64)
        if len(c) < self.info.n_taxa:
            raise ValueError("counts needs n_taxa entries")
        n = lib().mcq_refdb_abundance_text(self.h, c.ctypes.data_as(C.c_void_p), int(total), int(est_rank), None, 0)
        if n < 0:
            raise RuntimeError(lib().mcq_host_last_error().decode())
        buf = C.create_string_buffer(n + 1)
        lib().mcq_refdb_abundance_text(self.h, c.ctypes.data_as(C.c_void_p), int(total), int(est_rank), buf, n + 1)
        return buf.raw[:n].decode("latin-1")


# mcq_target_coverage: what engine.Coverage.read() returns, one record per target
COVERAGE_DTYPE = np.dtype([("hits", "<u8"), ("queries", "<u8"), ("windows_covered", "<u4"), ("reserved", "<u4")])


def _coverage_args(cov, windows):
    c = np.ascontiguousarray(cov, COVERAGE_DTYPE)
    w = np.ascontiguousarray(windows, np.uint32)
    if len(c) != len(w):
        raise ValueError("coverage records and windows differ in length")
    return c, w


def coverage_cut(cov, windows, percentile):
    """mcq_coverage_cut: removed[t] (uint8) -- the floor(H * percentile / 100) hit targets of the least breadth (include/mcq_host.h)"""
    c, w = _coverage_args(cov, windows)
    removed = np.zeros(len(c), np.uint8)
    if lib().mcq_coverage_cut(c.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), len(c), float(percentile),
                              removed.ctypes.data_as(C.c_void_p)) != 0:
        raise RuntimeError(lib().mcq_host_last_error().decode())
    return removed


def coverage_text(db, cov, windows, removed=None, reads_skipped=0, out_of_range=0, comment="# ", column="\t|\t", show_ranks=True, body=0,
                  lineage=False, lowest_rank=0, highest_rank=19):
    """mcq_coverage_text: the report block of -coverage; body: 0 name, 1 id, 2 name(id)"""
    c, w = _coverage_args(cov, windows)
    r = None if removed is None else np.ascontiguousarray(removed, np.uint8)
    if r is not None and len(r) != len(c):
        raise ValueError("removed and the coverage records differ in length")
    m = TaxonPrint(1 if show_ranks else 0, body, 1 if lineage else 0, lowest_rank, highest_rank)
    args = (db.h, c.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), len(c), None if r is None else r.ctypes.data_as(C.c_void_p),
            int(reads_skipped), int(out_of_range), comment.encode(), column.encode(), C.byref(m))
    n = lib().mcq_coverage_text(*args, None, 0)
    if n < 0:
        raise RuntimeError(lib().mcq_host_last_error().decode())
    buf = C.create_string_buffer(n + 1)
    lib().mcq_coverage_text(*args, buf, n + 1)
    return buf.raw[:n].decode("latin-1")


class HitsTable:
    """mcq_hits_table: the accumulator and writer of the -hits-per-seq table (matches_per_target, show_matches_per_targets)"""

    def __init__(self):
        self.h = C.c_void_p()
        lib().mcq_hits_table_create(C.byref(self.h))

    def add(self, query_id, target, win_beg, counts):
        c = np.ascontiguousarray(counts, np.uint32)
        if lib().mcq_hits_table_add(self.h, int(query_id), int(target), int(win_beg), len(c), c.ctypes.data_as(C.c_void_p)) != 0:
            raise RuntimeError(lib().mcq_host_last_error().decode())

    def merge(self, other):
        lib().mcq_hits_table_merge(self.h, other.h)

    def entries(self):
        return int(lib().mcq_hits_table_entries(self.h))

    def targets(self):
        return int(lib().mcq_hits_table_targets(self.h))

    def text(self, db, comment="# ", column="\t|\t", show_ranks=True, body=0, lineage=False, lowest_rank=0, highest_rank=19):
        """body: 0 name, 1 id, 2 name(id)"""
        m = TaxonPrint(1 if show_ranks else 0, body, 1 if lineage else 0, lowest_rank, highest_rank)
        n = lib().mcq_hits_table_text(self.h, db.h, comment.encode(), column.encode(), C.byref(m), None, 0)
        if n < 0:
            raise RuntimeError(lib().mcq_host_last_error().decode())
        buf = C.create_string_buffer(n + 1)
        lib().mcq_hits_table_text(self.h, db.h, comment.encode(), column.encode(), C.byref(m), buf, n + 1)
        return buf.raw[:n].decode("latin-1")

    def close(self):
        if getattr(self, "h", None):
            lib().mcq_hits_table_free(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EvalStats:
    """mcq_eval_stats: the reference's classification_statistics (assign, assign_known_correct, accessors, summary text)"""

    def __init__(self):
        self.rec = EvalStatsRec()

    def assign(self, assigned):
        lib().mcq_eval_stats_assign(C.byref(self.rec), int(assigned))

    def assign_known_correct(self, assigned, known, correct):
        lib().mcq_eval_stats_assign_known_correct(C.byref(self.rec), int(assigned), int(known), int(correct))

    def add(self, other):
        lib().mcq_eval_stats_add(C.byref(self.rec), C.byref(other.rec))

    def _get(self, name, *rank):
        return getattr(lib(), "mcq_eval_stats_" + name)(C.byref(self.rec), *[int(r) for r in rank])

    def total(self): return int(self._get("total"))
    def unknown(self): return int(self._get("unknown"))
    def unassigned(self): return int(self._get("assigned", RANK_NONE))
    def assigned(self, rank=20): return int(self._get("assigned", rank))
    def known(self, rank=20): return int(self._get("known", rank))
    def correct(self, rank=20): return int(self._get("correct", rank))
    def wrong(self, rank=20): return int(self._get("wrong", rank))
    def unknown_rate(self): return float(self._get("unknown_rate"))
    def unclassified_rate(self): return float(self._get("unclassified_rate"))
    def known_rate(self, rank=20): return float(self._get("known_rate", rank))
    def classification_rate(self, rank=20): return float(self._get("classification_rate", rank))
    def precision(self, rank): return float(self._get("precision", rank))
    def sensitivity(self, rank): return float(self._get("sensitivity", rank))

    def text(self, prefix="# "):
        """the summary's statistics block (show_taxon_statistics): mcq_eval_stats_text"""
        n = lib().mcq_eval_stats_text(C.byref(self.rec), prefix.encode(), None, 0)
        buf = C.create_string_buffer(n + 1)
        lib().mcq_eval_stats_text(C.byref(self.rec), prefix.encode(), buf, n + 1)
        return buf.raw[:n].decode("latin-1")


def rank_from_name(name):
    return int(lib().mcq_rank_from_name(name.encode()))


# ---- read files in chunks (mcq_read_stream_*, mcq_reads_parse): what mcq_query_cli's input stage does, for the tests
READS_EOF1, READS_EOF2, READS_INTERLEAVED = 1, 2, 4
READS_N, READS_BASES, READS_CUT1, READS_CUT2, READS_STATUS, READS_COMPLETE1, READS_COMPLETE2, READS_INFO_WORDS = 0, 1, 2, 3, 4, 5, 6, 8
READS_NOT_STRICT = 1


def parse_chunk(texts, flags, max_queries, max_bases):
    """mcq_reads_parse on one chunk per file (texts: 1 or 2 bytes objects) -> (info, bases, seq_off, hdr) as numpy arrays"""
    t1 = texts[0]
    t2 = texts[1] if len(texts) > 1 else None
    cap_q = max(1, min(max_queries, min(len(t) for t in texts) // 2 + 2))     # (no chunk holds more records: as mcq_query_cli sizes it)
    bases = np.zeros(len(t1) + (len(t2) if t2 is not None else 0) + 1, np.uint8)
    seq_off = np.zeros(2 * cap_q + 1, np.uint64)
    hdr = np.zeros(2 * cap_q, np.uint64)
    info = np.zeros(READS_INFO_WORDS, np.uint64)
    rc = lib().mcq_reads_parse(t1, len(t1), t2, len(t2) if t2 is not None else 0, flags, cap_q, max_bases,
                               bases.ctypes.data_as(C.c_void_p), seq_off.ctypes.data_as(C.c_void_p), hdr.ctypes.data_as(C.c_void_p),
                               info.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise RuntimeError(lib().mcq_host_last_error().decode())
    return info, bases, seq_off, hdr


class ReadStream:
    """mcq_read_stream_*: one file read in chunks, the unconsumed tail of a chunk carried into the next"""

    def __init__(self, path):
        h = C.c_void_p()
        if lib().mcq_read_stream_open(str(path).encode(), C.byref(h)) != 0:
            raise RuntimeError(lib().mcq_host_last_error().decode())
        self.h = h

    def fill(self, buf, want):
        n, eof = C.c_uint64(), C.c_int32()
        if lib().mcq_read_stream_fill(self.h, buf, len(buf), want, C.byref(n), C.byref(eof)) != 0:
            raise RuntimeError(lib().mcq_host_last_error().decode())
        return int(n.value), bool(eof.value)

    def consume(self, n):
        if lib().mcq_read_stream_consume(self.h, n) != 0:
            raise RuntimeError(lib().mcq_host_last_error().decode())

    def close(self):
        if getattr(self, "h", None):
            lib().mcq_read_stream_close(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def read_batches(paths, chunk, max_queries=1 << 40, max_bases=1 << 62, prepare=None, interleaved=False):
    """The input stage of mcq_query_cli on 1 or 2 files: fill a chunk per file (three buffer sets in rotation, so the carry
    moves from one buffer to another), prepare it (default: parse_chunk; the GPU tests pass the device step), consume what
    it used; a file with no complete record in a full chunk gets a buffer twice as large, for that chunk only.  Yields
    (texts, info, bases, seq_off, hdr, caps) per batch; caps = the buffer sizes used.  interleaved: one file whose records
    2q, 2q+1 are the mates of query q (READS_INTERLEAVED is passed on to prepare)."""
    prepare = prepare or parse_chunk
    streams = [ReadStream(p) for p in paths]
    sets = [[C.create_string_buffer(max(1, chunk)) for _ in paths] for _ in range(3)]
    want = [max(1, chunk)] * len(paths)
    carry = [0] * len(paths)
    j = 0
    try:
        while True:
            bufs = sets[j % 3]
            texts, flags = [], (READS_INTERLEAVED if interleaved else 0)
            for m, s in enumerate(streams):
                old = bufs[m]                                       # (may hold the carry: alive until the fill has moved it)
                need = max(want[m], carry[m])
                if len(bufs[m]) < need:
                    bufs[m] = C.create_string_buffer(need)
                n, eof = s.fill(bufs[m], need)
                del old
                texts.append(bufs[m].raw[:n])
                flags |= (READS_EOF1 << m) if eof else 0
            info, bases, seq_off, hdr = prepare(texts, flags, max_queries, max_bases)
            n = int(info[READS_N])
            if n == 0:
                done = False
                for m in range(len(paths)):
                    if int(info[READS_COMPLETE1 + m]) == 0:
                        if flags & (READS_EOF1 << m):
                            done = True
                        else:
                            want[m] = 2 * len(texts[m])
                for m, s in enumerate(streams):
                    s.consume(0)
                    carry[m] = len(texts[m])
                if done:
                    return
                continue
            caps = [len(b) for b in bufs]
            for m, s in enumerate(streams):
                s.consume(int(info[READS_CUT1 + m]))
                carry[m] = len(texts[m]) - int(info[READS_CUT1 + m])
                want[m] = max(1, chunk)
            yield texts, info, bases, seq_off, hdr, caps
            j += 1
    finally:
        for s in streams:
            s.close()


# ---- the inputs of a build (mcq_taxdump_*, mcq_target_*, mcq_genome_files, mcq_genome_reader_*): what mcq_build_cli reads
def _err():
    return RuntimeError(lib().mcq_host_last_error().decode())


def _rec(r):
    return dict(id=int(r.id), parent=int(r.parent), rank=int(r.rank), name=(r.name or b"").decode("latin-1"),
                file=(r.file or b"").decode("latin-1"), index=int(r.index), windows=int(r.windows))


def read_taxdump(directory):
    """mcq_taxdump_read: the taxon records (dicts as write_shard takes them) of nodes.dmp / names.dmp / merged.dmp, in ascending id"""
    h = C.c_void_p()
    if lib().mcq_taxdump_read(str(directory).encode(), C.byref(h)) != 0:
        raise _err()
    try:
        arr = lib().mcq_taxdump_taxa(h)
        return [_rec(arr[i]) for i in range(lib().mcq_taxdump_count(h))]
    finally:
        lib().mcq_taxdump_free(h)


def taxonomy_db(directory):
    """mcq_refdb_from_taxdump: a RefDb that is the taxonomy of a dump alone (no targets, no table): what a merge works on"""
    h, d = C.c_void_p(), C.c_void_p()
    if lib().mcq_taxdump_read(str(directory).encode(), C.byref(d)) != 0:
        raise _err()
    try:
        if lib().mcq_refdb_from_taxdump(d, C.byref(h)) != 0:
            raise _err()
    finally:
        lib().mcq_taxdump_free(d)
    db = RefDb.__new__(RefDb)
    db.h, db.info = h, Info()
    lib().mcq_refdb_get_info(db.h, C.byref(db.info))
    return db


def taxid_table(db):
    """mcq_refdb_taxid_table: (ids int64 ascending, taxon index u32 of each): what mcq_merge_create takes"""
    ids, idx, n = np.zeros(db.info.n_taxa, np.int64), np.zeros(db.info.n_taxa, np.uint32), C.c_uint64(0)
    if lib().mcq_refdb_taxid_table(db.h, ids.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p), C.byref(n)) != 0:
        raise _err()
    return ids[:n.value], idx[:n.value]


def results_properties(path):
    """mcq_results_properties: (top_hits column, byte at which the results begin, number of mapping lines) of a results file"""
    col, begin, n = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
    if lib().mcq_results_properties(str(path).encode(), C.byref(col), C.byref(begin), C.byref(n)) != 0:
        raise _err()
    return int(col.value), int(begin.value), int(n.value)


def merge_host(text, n_queries, tophits_column=2, file_name="", first_line_no=1, text_offset=0):
    """mcq_merge_host: the reference's token parser over whole lines of a results file (bytes) -> (line_query u32, item_off u64,
    taxid int64, hits u32, header_off u64, header_len u32), the arrays of engine.Merge.lines"""
    line_cap, item_cap = text.count(b"\n") + 1, text.count(b":") + 1
    q, off = np.zeros(line_cap, np.uint32), np.zeros(line_cap + 1, np.uint64)
    tid, hits = np.zeros(item_cap, np.int64), np.zeros(item_cap, np.uint32)
    ho, hl = np.zeros(line_cap, np.uint64), np.zeros(line_cap, np.uint32)
    nl, ni = C.c_uint64(0), C.c_uint64(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    if lib().mcq_merge_host(text, len(text), tophits_column, n_queries, file_name.encode(), first_line_no, text_offset, p(q), p(off),
                            p(tid), p(hits), p(ho), p(hl), line_cap, item_cap, C.byref(nl), C.byref(ni)) != 0:
        raise _err()
    nl, ni = int(nl.value), int(ni.value)
    return q[:nl], off[:nl + 1], tid[:ni], hits[:ni], ho[:nl], hl[:nl]


def taxa_clade_keys(targets, dump, rank):
    """mcq_taxa_clade_keys: per target the key of its ancestor at `rank` (index into the taxon list a build writes: the targets'
    sequence-level taxa, last target first, then the dump's), NO_TAXON where it has none -- RefDb.clade_keys of the database
    built from these inputs, without the database.  targets: the records read_genomes gives; dump: those of read_taxdump."""
    taxa = list(reversed(targets)) + list(dump)
    arr = (TaxonRec * max(1, len(taxa)))()
    keep = []
    for i, t in enumerate(taxa):
        nm, fl = t["name"].encode("latin-1"), t["file"].encode("latin-1")
        keep += [nm, fl]
        arr[i] = TaxonRec(t["id"], t["parent"], t["rank"], nm, fl, t["index"], t["windows"])
    out = np.zeros(len(targets), np.uint32)
    if lib().mcq_taxa_clade_keys(arr, len(taxa), len(targets), rank, out.ctypes.data_as(C.c_void_p)) != 0:
        raise _err()
    return out


def target_name(header):
    """name of the sequence-level taxon of a sequence with this header (bytes, without the '>')"""
    n = lib().mcq_target_name(header, len(header), None, 0)
    buf = C.create_string_buffer(n + 1)
    lib().mcq_target_name(header, len(header), buf, n + 1)
    return buf.raw[:n]


def target_parent_taxid(header):
    return int(lib().mcq_target_parent_taxid(header, len(header)))


def genome_files(args):
    """the files a build reads for these command-line arguments, in the order it reads them"""
    arr = (C.c_char_p * len(args))(*[str(a).encode() for a in args])
    h = C.c_void_p()
    if lib().mcq_genome_files(arr, len(args), C.byref(h)) != 0:
        raise _err()
    try:
        return [lib().mcq_file_list_get(h, i).decode() for i in range(lib().mcq_file_list_count(h))]
    finally:
        lib().mcq_file_list_free(h)


class Seq2Tax:
    """mcq_seq2tax_*: the pre-mapping of sequence ids and file accessions to taxon ids (assembly_summary.txt and its like)"""

    def __init__(self, h=None):
        if h is None:
            h = C.c_void_p()
            if lib().mcq_seq2tax_create(C.byref(h)) != 0:
                raise _err()
        self.h = h

    def add_file(self, path):
        """reads one mapping file into the map; False (and nothing read) if it does not open"""
        opened = C.c_int32(0)
        if lib().mcq_seq2tax_add_file(self.h, str(path).encode(), C.byref(opened)) != 0:
            raise _err()
        return bool(opened.value)

    def items(self):
        out = []
        for i in range(lib().mcq_seq2tax_count(self.h)):
            k, v = C.c_char_p(), C.c_int64()
            if lib().mcq_seq2tax_entry(self.h, i, C.byref(k), C.byref(v)) != 0:
                raise _err()
            out.append((k.value, int(v.value)))
        return out

    def find(self, name):
        return int(lib().mcq_seq2tax_find(self.h, name, len(name)))

    def close(self):
        if getattr(self, "h", None):
            lib().mcq_seq2tax_free(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def read_seq2tax(dirs):
    """<dir>/assembly_summary.txt of every directory, in the order given, into one Seq2Tax (the first entry of a key stays)"""
    m = Seq2Tax()
    for d in dirs:
        m.add_file(str(d) + "/assembly_summary.txt")
    return m


def read_seq2tax_for(files):
    """mcq_seq2tax_read: the same for the distinct directories of the genome files, in the reference's order"""
    arr = (C.c_char_p * len(files))(*[str(f).encode() for f in files])
    h = C.c_void_p()
    if lib().mcq_seq2tax_read(arr, len(files), C.byref(h)) != 0:
        raise _err()
    return Seq2Tax(h)


def taxmap_files(taxdir, postmap=None):
    """mcq_taxmap_files: the *.accession2taxid files in reading order (they need not exist)"""
    h = C.c_void_p()
    if lib().mcq_taxmap_files(str(taxdir).encode() if taxdir else None, str(postmap).encode() if postmap else None, C.byref(h)) != 0:
        raise _err()
    try:
        return [lib().mcq_file_list_get(h, i).decode() for i in range(lib().mcq_file_list_count(h))]
    finally:
        lib().mcq_file_list_free(h)


def accmap_host(text, names, unranked, parent, skip_first_line=True, rule=None):
    """mcq_accmap_host: the reference's token parser over one mapping text (bytes).  names: the target names (bytes, target t at index
    t); unranked (uint8) and parent (int64) are numpy arrays that are UPDATED.  Returns the number of records read.  rule (0 to 3):
    mcq_accmap_host_rule -- 1 / 2 / 3: a record names the name equal to its acc / accver / gi word and nothing else."""
    from .engine import sorted_names
    blob, off, tgt = sorted_names([bytes(n) for n in names])
    assert unranked.dtype == np.uint8 and parent.dtype == np.int64 and len(unranked) == len(parent) == len(names)
    n = C.c_uint64(0)
    head = (text, len(text), 1 if skip_first_line else 0, blob, off.ctypes.data_as(C.c_void_p), len(tgt), tgt.ctypes.data_as(C.c_void_p),
            unranked.ctypes.data_as(C.c_void_p), parent.ctypes.data_as(C.c_void_p), len(names))
    rc = lib().mcq_accmap_host(*head, C.byref(n)) if rule is None else lib().mcq_accmap_host_rule(*head, rule, C.byref(n), None, None)
    if rc != 0:
        raise _err()
    return int(n.value)


ID_ACC, ID_ACCVER, ID_GI = 1, 2, 3


def annotate_id(line, id_type=ID_ACCVER):
    """mcq_annotate_id: the id annotate takes from a header line (bytes, WITH its '>' or '@'); b"" if it has none"""
    n = lib().mcq_annotate_id(line, len(line), id_type, None, 0)
    if n < 0:
        raise _err()
    buf = C.create_string_buffer(n + 1)
    lib().mcq_annotate_id(line, len(line), id_type, buf, n + 1)
    return buf.raw[:n]


def annotate_rewrite(line, has_id, taxid, field_sep=b" ", value_sep=b"|"):
    """mcq_annotate_rewrite: the header line (bytes) with its old taxid cut and, if has_id, taxid<vs>N<fs> put in"""
    n = lib().mcq_annotate_rewrite(line, len(line), 1 if has_id else 0, taxid, field_sep, value_sep, None, 0)
    if n < 0:
        raise _err()
    buf = C.create_string_buffer(n + 1)
    lib().mcq_annotate_rewrite(line, len(line), 1 if has_id else 0, taxid, field_sep, value_sep, buf, n + 1)
    return buf.raw[:n]


def read_genomes(files, cap, io_bytes=1 << 20, after=None, skipped=None, seq2tax=None):
    """mcq_genome_reader_* over `files` with a buffer of `cap` bases: (bases of all targets back to back as bytes, taxon records of
    the targets as dicts, lengths, number of fills).  after: a RefDb -- mcq_genome_reader_open_after, the sequences are added to
    that database (its names are taken, ids go on behind its targets); skipped: a list that gets mcq_genome_reader_n_skipped;
    seq2tax: a Seq2Tax -- mcq_genome_reader_open_mapped, the parents come from the map before the header."""
    arr = (C.c_char_p * len(files))(*[str(f).encode() for f in files])
    h = C.c_void_p()
    if seq2tax is not None:
        rc = lib().mcq_genome_reader_open_mapped(arr, len(files), io_bytes, after.h if after is not None else None, seq2tax.h, C.byref(h))
    elif after is None:
        rc = lib().mcq_genome_reader_open(arr, len(files), io_bytes, C.byref(h))
    else:
        rc = lib().mcq_genome_reader_open_after(arr, len(files), io_bytes, after.h, C.byref(h))
    if rc != 0:
        raise _err()
    try:
        buf = C.create_string_buffer(max(1, cap))
        out, fills = [], 0
        n, done = C.c_uint64(), C.c_int32()
        while not done.value:
            if lib().mcq_genome_reader_next(h, buf, cap, C.byref(n), C.byref(done)) != 0:
                raise _err()
            assert n.value <= cap
            out.append(buf.raw[:n.value]); fills += 1
        recs, lens = [], []
        for t in range(lib().mcq_genome_reader_n_targets(h)):
            r, ln = TaxonRec(), C.c_uint64()
            if lib().mcq_genome_reader_target(h, t, C.byref(r), C.byref(ln)) != 0:
                raise _err()
            recs.append(_rec(r)); lens.append(int(ln.value))
        if skipped is not None:
            skipped.append(int(lib().mcq_genome_reader_n_skipped(h)))
        return b"".join(out), recs, lens, fills
    finally:
        lib().mcq_genome_reader_close(h)
