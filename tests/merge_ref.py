"""Python restatement of the reference's `merge` mode for the tests of mcq_merge_*: read_results (src/mode_merge.cpp:209-264) over
the istream model of tests/taxmap_ref.py, best_distinct_matches_in_contiguous_window_ranges::insert (src/candidates.h:236-285),
classify (src/classification.cpp:235-265) with ranked_lca (src/taxonomy.h:531-537), and the strict form of include/mcq.h
(mcq_merge_chunk) line by line.  Where the reference's stream goes bad inside a mapping line it never returns (its loop waits for
a TAB that a failed stream does not deliver): the restatement raises Stop with the number of that line."""
import numpy as np

from taxmap_ref import IStream

NONE = 0xFFFFFFFF
RANKS = ["sequence", "form", "variety", "subspecies", "species", "subgenus", "genus", "subtribe", "tribe", "subfamily", "family",
         "suborder", "order", "subclass", "class", "subphylum", "phylum", "subkingdom", "kingdom", "domain", "root", "none"]
RANK = {n: i for i, n in enumerate(RANKS)}
RANK["superkingdom"] = RANK["domain"]
RANK["no rank"] = RANK["none"]
MAX_LINE, MAX_ITEMS = 4096, 64


class Stop(Exception):
    """the reference does not return from this line"""

    def __init__(self, line_no):
        Exception.__init__(self, "the reference's stream goes bad in line %d" % line_no)
        self.line_no = line_no


class Tax:
    """taxa: [(taxid, parent taxid, rank number)], taxon t at index t.  lineage[t, r] = index of the ancestor of t (t included) that
    has rank r, NONE if there is none; taxon 1 has rank root"""

    def __init__(self, taxa):
        self.ids = [t[0] for t in taxa]
        self.index = {}
        for i, t in enumerate(taxa):
            self.index.setdefault(t[0], i)
        self.rank = np.array([RANK["root"] if t[0] == 1 else t[2] for t in taxa], np.uint8)
        self.lineage = np.full((len(taxa), 21), NONE, np.uint32)
        for i, t in enumerate(taxa):
            j, seen = i, set()
            while j is not None and j not in seen:
                seen.add(j)
                if self.rank[j] < 21 and self.lineage[i, self.rank[j]] == NONE:
                    self.lineage[i, self.rank[j]] = j
                j = self.index.get(taxa[j][1]) if taxa[j][1] != taxa[j][0] else None

    @classmethod
    def of_dump(cls, nodes_dmp):
        """nodes.dmp (no merged.dmp), ascending id: the order mcq_taxdump_read gives"""
        rows = []
        for line in open(nodes_dmp, "rb").read().decode().splitlines():
            f = [x.strip() for x in line.split("|")]
            rows.append((int(f[0]), int(f[1]), RANK.get(f[2], RANK["none"])))
        return cls(sorted(rows))

    @classmethod
    def of_lineages(cls, ids, lineage, rank):
        t = cls([])
        t.ids, t.lineage, t.rank = [int(x) for x in ids], np.asarray(lineage, np.uint32).reshape(-1, 21), np.asarray(rank, np.uint8)
        for i, x in enumerate(t.ids):
            t.index.setdefault(x, i)
        return t

    def ranked_lca(self, a, b):
        for r in range(21):
            if self.lineage[a, r] != NONE and self.lineage[a, r] == self.lineage[b, r]:
                return int(self.lineage[a, r])
        return NONE


def insert(top, tax, hits, T, max_cand, merge_below):
    """top: list of [taxon index, hits], changed in place"""
    if merge_below > 0 and T.lineage[tax, merge_below] != NONE:
        tax = int(T.lineage[tax, merge_below])
    if T.rank[tax] != 0:
        for i, c in enumerate(top):
            if c[0] == tax:
                if hits > c[1]:
                    c[1] = hits
                # std::sort of top[0 .. i]: at most 16 entries, so an insertion sort, which is stable
                top[:i + 1] = sorted(top[:i + 1], key=lambda e: -e[1])
                return
    j = 0
    while j < len(top) and not hits > top[j][1]:                # upper_bound with a.hits > b.hits
        j += 1
    if j != len(top) or len(top) < max_cand:
        top.insert(j, [tax, hits])
        del top[max_cand:]


def classify(top, T, hits_min, frac, highest):
    if not top or top[0][1] < hits_min:
        return NONE
    lca = top[0][0]
    thr = np.float32(top[0][1] - hits_min) * np.float32(frac) if top[0][1] > hits_min else np.float32(0)
    for tax, hits in top[1:]:
        if not np.float32(hits) > thr:
            break
        lca = T.ranked_lca(lca, tax)
        if lca == NONE or T.rank[lca] > highest:
            return NONE
    return lca if T.rank[lca] <= highest else NONE


class _Stream(IStream):
    def peek(self):
        if not self.good():
            return -1
        if self.p >= len(self.d):
            self.eof = True
            return -1
        return self.d[self.p]

    def get(self):
        c = self.peek()
        if c < 0:
            self.fail = True
        else:
            self.p += 1
        return c


class Merged:
    def __init__(self, T, n_queries, max_cand=2, merge_below=RANK["species"]):
        self.T, self.max_cand, self.merge_below = T, max_cand, merge_below
        self.lists = [[] for _ in range(n_queries)]
        self.headers = [b""] * n_queries
        self.unknown = 0
        self.record = None                                       # a list: read_results appends (query, header offset, header, items) per line

    def read_results(self, text, tophits_column=2):
        """the mapping part of one file (from resultsBegin on), as read_results reads it"""
        s = _Stream(text)
        begin = s.peek()
        while s.good():
            line_no = text.count(b"\n", 0, s.p) + 1
            if begin != ord("#"):
                ok, qid = s.number(False)
                if ok:
                    line_no = text.count(b"\n", 0, s.p) + 1      # (behind blanks the id may stand in a later line)
                if not ok or qid == 0 or qid > len(self.lists):
                    raise Stop(line_no)                          # (0 aliases 1, beyond the count writes past the vectors: rejected here)
                qid -= 1
                s.ignore(b"|")
                token = text[s.p:s.p + MAX_LINE].split(None, 1)[:1]          # (bytes.split(None): the blanks of the stream's sentry)
                if token and b"|" in token[0]:
                    raise Stop(line_no)                        # (a '|' in the header token: the reference parses such a line in two
                                                                 #  ways, depending on whether it knows the header: rejected here)
                items, rest = [], text[s.p:s.p + MAX_LINE]
                token_at = s.p + len(rest) - len(rest.lstrip())
                if not self.headers[qid]:
                    w = s.word()
                    if w:
                        self.headers[qid] = w
                for _ in range(1, tophits_column):
                    s.ignore(b"|")
                s.ignore(b"\t")
                nxt = s.peek()
                while nxt != 9:
                    ok, taxid = s.number(True)
                    s.ignore(b":")
                    ok2, hits = s.number(False)
                    if not (ok and ok2) or not s.good() or hits >= 2 ** 32:
                        raise Stop(line_no)                      # (hits of 2^32 and more: not supported, rejected here)
                    items.append((taxid, hits))
                    if taxid in self.T.index:
                        insert(self.lists[qid], self.T.index[taxid], hits, self.T, self.max_cand, self.merge_below)
                    else:
                        self.unknown += 1
                    nxt = s.get()
                    if nxt < 0:
                        raise Stop(line_no)
                if self.record is not None:
                    self.record.append((qid, token_at, token[0] if token else b"", items))
            s.ignore(b"\n")
            begin = s.peek()

    def as_arrays(self):
        """(n_cand [n], pairs [n, max_cand, 2]) with zeros behind a list's end"""
        n = np.array([len(l) for l in self.lists], np.uint32)
        pairs = np.zeros((len(self.lists), self.max_cand, 2), np.uint32)
        for q, l in enumerate(self.lists):
            for i, c in enumerate(l):
                pairs[q, i] = c
        return n, pairs


def line_is_strict(line, n_queries, tophits_column=2):
    """one line without its LF"""
    if line[:1] == b"#":
        return True
    if len(line) + 1 > MAX_LINE:
        return False
    cols, rest = [], line
    for _ in range(tophits_column):                              # every column in front of top_hits ends in TAB | TAB
        k = rest.find(b"\t|\t")
        if k < 0:
            return False
        cols.append(rest[:k])
        rest = rest[k + 3:]
    if any(b"|" in c for c in cols):
        return False
    if not (cols[0].isdigit() and len(cols[0]) <= 18 and 1 <= int(cols[0]) <= n_queries):
        return False
    if not cols[1] or cols[1][:1] in b" \t\v\f\r":
        return False
    tab = rest.find(b"\t")
    if tab < 0:
        return False
    if tab == 0:
        return True
    items = rest[:tab].split(b",")
    if len(items) > MAX_ITEMS:
        return False
    for it in items:
        f = it.split(b":")
        if len(f) != 2 or not (f[0].isdigit() and f[1].isdigit() and len(f[0]) <= 18 and len(f[1]) <= 9):
            return False
    return True


def is_strict(text, n_queries, tophits_column=2):
    if not text:
        return True
    lines = text.split(b"\n")
    if text.endswith(b"\n"):
        lines.pop()
    ids = [int(l.split(b"\t")[0]) for l in lines if line_is_strict(l, n_queries, tophits_column) and l[:1] != b"#"]
    return all(l and line_is_strict(l, n_queries, tophits_column) for l in lines) and len(ids) == len(set(ids))
