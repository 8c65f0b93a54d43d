"""Coverage of reference sequences restated in plain NumPy / Python: what mcq_coverage_add / mcq_coverage_read (include/mcq.h)
accumulate, the cut of mcq_coverage_cut and the report of mcq_coverage_text (include/mcq_host.h).  Nothing here calls the library."""
import math

import numpy as np

UNUSED = 0xFFFFFFFF
COL = "\t|\t"
HEAD = "--- coverage of reference sequences ---"
COLUMNS = ["windows_in_sequence", "windows_covered", "coverage", "queries", "hits"]


class RefCoverage:
    """one bit per (target, window), a segment per target that starts on a 32-bit word; queries and hits per target"""

    def __init__(self, windows):
        self.windows = [int(w) for w in windows]
        self.word_off = [0]
        for w in self.windows:
            self.word_off.append(self.word_off[-1] + (w + 31) // 32)
        self.reset()

    def reset(self):
        self.words = np.zeros(self.word_off[-1], np.uint32)
        self.queries = [0] * len(self.windows)
        self.hits = [0] * len(self.windows)
        self.out_of_range = 0

    def add(self, ranges, counts, range_cap):
        """ranges [n, 4] (tgt, hits, win_beg, n_win) and counts [n, range_cap] of n = n_queries * n_slots slots.  A slot is taken
        if tgt != UNUSED and n_win > 0; it is refused as a whole -- and counted -- if tgt is no target, the range ends behind the
        target's windows, or it is wider than a count row.  counts[i] is looked at for i < n_win only."""
        ranges = np.asarray(ranges, np.uint32).reshape(-1, 4)
        counts = np.asarray(counts, np.uint32).reshape(len(ranges), range_cap)
        for (tgt, _, beg, n_win), row in zip(ranges.tolist(), counts):
            if tgt == UNUSED or n_win == 0:
                continue
            if tgt >= len(self.windows) or n_win > range_cap or beg + n_win > self.windows[tgt]:
                self.out_of_range += 1
                continue
            self.queries[tgt] += 1
            for i in range(n_win):
                c = int(row[i])
                if c > 0:
                    self.hits[tgt] += c
                    w = beg + i
                    self.words[self.word_off[tgt] + w // 32] |= np.uint32(1 << (w % 32))

    def read(self):
        """[(hits, queries, windows_covered)] per target"""
        out = []
        for t in range(len(self.windows)):
            seg = self.words[self.word_off[t]:self.word_off[t + 1]]
            out.append((self.hits[t], self.queries[t], int(sum(bin(int(x)).count("1") for x in seg))))
        return out


def cut(covered, windows, percentile):
    """removed[t]: the hit targets (covered > 0) ordered by covered / windows ascending -- compared by cross-multiplication of
    integers, ties by target id --, the first floor(H * percentile / 100) of them"""
    hit = [t for t in range(len(covered)) if covered[t] > 0]

    def before(a, b):
        l, r = covered[a] * windows[b], covered[b] * windows[a]
        return l < r if l != r else a < b

    order = []
    for t in hit:                                   # insertion by the pairwise rule itself: no key, no float
        i = 0
        while i < len(order) and before(order[i], t):
            i += 1
        order.insert(i, t)
    k = min(len(hit), int(math.floor(len(hit) * float(percentile) / 100.0)))
    removed = [0] * len(covered)
    for t in order[:k]:
        removed[t] = 1
    return removed


def report(rows, names, windows, removed=None, reads_skipped=0, out_of_range=0, comment="# ", col=COL):
    """rows: [(hits, queries, covered)] per target; names[t]: the sequence column of target t"""
    lines = [comment + HEAD]
    if reads_skipped:
        lines.append(comment + "%d queries beyond the capacity of mcq_target_hits added nothing" % reads_skipped)
    if out_of_range:
        lines.append(comment + "%d candidate ranges outside their sequence added nothing" % out_of_range)
    lines.append(comment + "TABLE_LAYOUT:  sequence " + "".join(col + " " + c + " " for c in COLUMNS) + col + " kept")
    for t, (hits, queries, covered) in enumerate(rows):
        if queries == 0:
            continue
        frac = "%.6f" % (covered / windows[t] if windows[t] else 0.0)
        lines.append(col.join([names[t], str(windows[t]), str(covered), frac, str(queries), str(hits),
                               "removed" if removed is not None and removed[t] else "kept"]))
    return "\n".join(lines) + "\n"


def parse_report(lines, col=COL):
    """{sequence column: (windows, covered, coverage text, queries, hits, kept text)} from the lines of a report block"""
    out = {}
    for l in lines:
        if l and not l.startswith("#"):
            f = l.split(col)
            out[f[0]] = (int(f[1]), int(f[2]), f[3], int(f[4]), int(f[5]), f[6])
    return out
