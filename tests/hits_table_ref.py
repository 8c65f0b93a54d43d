"""Plain-Python restatement of the reference's -hits-per-seq table, for the tests of the host accumulator and of the CLI:
matches_per_target::insert and sort_match_lists (src/matches_per_target.h:111-184) and show_matches_per_targets
(src/printing.cpp:437-469) with show_taxon (:117-143, :305-330) for a sequence-level taxon."""
from oracle import dbfile


class RefHitsTable:
    def __init__(self):
        self.per_target = {}                 # target -> [(qid, [(win, hits), ...])]

    def insert(self, qid, matches, cands, hitmin=0):
        """matches: the read's sorted match list, u64 (tgt << 32) | win; cands: its candidates (tgt, hits, beg, end), all at
        sequence level.  Per candidate with hits >= hitmin: the distinct windows of the target inside [beg, end] with their
        multiplicities, in ascending window order."""
        ms = [(int(m) >> 32, int(m) & 0xFFFFFFFF) for m in matches]
        for tgt, hits, beg, end in cands:
            if hits < hitmin:
                continue
            mpw = []
            for t, w in ms:                  # (ms is sorted: windows ascend inside a target)
                if t == tgt and beg <= w <= end:
                    if mpw and mpw[-1][0] == w:
                        mpw[-1][1] += 1
                    else:
                        mpw.append([w, 1])
            if mpw:                          # (a candidate always has a match at its first window)
                self.per_target.setdefault(int(tgt), []).append((int(qid), [tuple(x) for x in mpw]))

    def add(self, qid, tgt, wins):
        self.per_target.setdefault(int(tgt), []).append((int(qid), [tuple(x) for x in wins]))

    def sort_match_lists(self):
        for lst in self.per_target.values():
            lst.sort(key=lambda c: (c[1][0][0], c[1][-1][0], c[0]))


def taxon_text(tax, idx, show_ranks=True, body=0, lineage=False, lowest=0, highest=19):
    """show_taxon(os, db, opt, tax) of taxon index idx: body 0 name, 1 id, 2 name(id)"""
    def one(i, rank):
        have = i != dbfile.NONE
        t = tax.taxa[int(i)] if have else None
        s = (dbfile.RANK_NAMES[t["rank"] if have else rank] + ":") if show_ranks else ""
        name, tid = (t["name"], t["id"]) if have else ("--", 0)
        return s + (name if body == 0 else str(tid) if body == 1 else "%s(%d)" % (name, tid))
    rmin = max(lowest, tax.taxa[idx]["rank"])
    rmax = max(rmin, highest) if lineage else rmin
    return ",".join(one(tax.lineage[idx, r], r) for r in range(rmin, rmax + 1))


def table_text(table, tax, windows_of_target, query_winstride, comment="# ", col="\t|\t", **mode):
    """the block of show_matches_per_targets; rows in ascending target id (the reference's order is that of an unordered_map)"""
    table.sort_match_lists()
    out = [comment + "--- list of hits for each reference sequence ---",
           comment + "window start position within sequence = window_index * window_stride(=%d)" % query_winstride,
           comment + "TABLE_LAYOUT:  sequence " + col + " windows_in_sequence " + col +
           "queryid/window_index:hits/window_index:hits/...,queryid/..."]
    for tgt in sorted(table.per_target):
        idx = tax.by_id[-(tgt + 1)]
        row = taxon_text(tax, idx, **mode) + col + str(windows_of_target[tgt]) + col
        row += ",".join(str(qid) + "".join("/%d:%d" % w for w in wins) for qid, wins in table.per_target[tgt])
        out.append(row)
    return "\n".join(out) + "\n"


def windows_of_targets(fx):
    """windows_in_sequence of every target of a golden fixture: the `windows` field of its taxon in the owning rank's shard"""
    out = [0] * fx.n_targets
    for s in fx.shards:
        for t in s["taxa"]:
            if t["id"] < 0 and -t["id"] - 1 < fx.n_targets and t["windows"]:
                out[-t["id"] - 1] = t["windows"]
    return out
