"""Restatement of what -allhits and -locations print, for the tests of mcq_all_hits and of mcq_query_cli.

rle:               a read's sorted match list (OracleDb.matches: u64 (tgt << 32) | win, ascending) run-length compressed: one
                   (tgt, win, count) per distinct location, ascending -- what mcq_all_hits returns.
all_hits_column:   show_matches over match locations (src/printing.cpp:365-416): `name/win:count,` per entry with -lowest sequence,
                   `name:count,` above it, where name is that of the target's ancestor at -lowest or, without one, the target's own.
                   Every entry ends with a comma; nothing is merged across entries; no entry, empty text.
locations_column:  show_candidate_ranges (src/printing.cpp:422-432): `[w * beg,w * end + winlen] ` per candidate, each with a
                   trailing space."""
import numpy as np

HIT = np.dtype([("tgt", "<u4"), ("win", "<u4"), ("hits", "<u4")])


def rle(matches):
    """u64 sorted locations -> HIT records"""
    m = np.ascontiguousarray(matches, np.uint64)
    if len(m) == 0:
        return np.zeros(0, HIT)
    assert (m[1:] >= m[:-1]).all()
    u, c = np.unique(m, return_counts=True)
    out = np.zeros(len(u), HIT)
    out["tgt"] = (u >> np.uint64(32)).astype(np.uint32)
    out["win"] = (u & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    out["hits"] = c.astype(np.uint32)
    return out


def name_of_target(tax, tgt, lowest):
    """tax: oracle.dbfile.Taxonomy.  The name printed for target `tgt` at rank index `lowest` (0 = sequence)"""
    return tax.taxa[int(tax.target_keys(tgt + 1, lowest)[tgt]) & 0x7FFFFFFF]["name"]


def all_hits_column(entries, names, sequence_level, drop=()):
    """entries: HIT records (or (tgt, win, count) triples); names[tgt]: the printed name; drop: targets whose entries are left out
    (-exclude)"""
    out = []
    for t, w, c in (tuple(int(x) for x in e) for e in entries):
        if t in drop:
            continue
        out.append("%s/%d:%d," % (names[t], w, c) if sequence_level else "%s:%d," % (names[t], c))
    return "".join(out)


def locations_column(cands, stride, winlen):
    """cands: (beg, end) window pairs of the candidates of a read, in list order"""
    return "".join("[%d,%d] " % (stride * b, stride * e + winlen) for b, e in cands)
