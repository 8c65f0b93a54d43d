"""Python restatement of how the reference maps sequences to taxa with mapping files, for tests/test_host_taxmap.py and the GPU
tests of mcq_accmap_*: read_sequence_to_taxon_id_mapping and make_sequence_to_taxon_id_map (src/taxonomy_io.cpp:190-310),
find_taxon_id (src/mode_build.cpp:531-550), rank_targets_with_mapping_file (src/mode_build.cpp:248-312) with taxon_with_name and
taxon_with_similar_name (src/sketch_database.h:620-639).  The parsers are written against a small model of std::istream (good /
eof / fail, a sentry that skips white space, ignore, getline, num_get), so that the quirks of the originals -- passes that run
across lines, a stream that is still good after its last line -- come out of the model and are not listed case by case."""
import bisect
import re

_WS = b" \t\n\v\f\r"


class IStream:
    def __init__(self, data):
        self.d, self.p, self.eof, self.fail = data, 0, False, False

    def good(self):
        return not self.eof and not self.fail

    def getline(self):
        """the line, or None when nothing was extracted because the stream was not good (the caller's string keeps its text)"""
        if not self.good():
            self.fail = True
            return None
        i = self.d.find(b"\n", self.p)
        if i >= 0:
            line, self.p = self.d[self.p:i], i + 1
            return line
        line, self.p, self.eof = self.d[self.p:], len(self.d), True
        if not line:
            self.fail = True
        return line

    def ignore(self, c):
        if not self.good():
            self.fail = True
            return
        i = self.d.find(c, self.p)
        if i >= 0:
            self.p = i + 1
        else:
            self.p, self.eof = len(self.d), True

    def _sentry(self):
        if not self.good():
            self.fail = True
            return False
        while self.p < len(self.d) and self.d[self.p] in _WS:
            self.p += 1
        if self.p >= len(self.d):
            self.eof = self.fail = True
            return False
        return True

    def word(self):
        if not self._sentry():
            return None
        q = self.p
        while q < len(self.d) and self.d[q] not in _WS:
            q += 1
        w, self.p = self.d[self.p:q], q
        if q == len(self.d):
            self.eof = True
        return w

    def number(self, signed):
        """(extracted, value): value None = the variable keeps what it held (the sentry failed); a failed conversion stores 0"""
        if not self._sentry():
            return False, None
        q, neg = self.p, False
        if self.d[q:q + 1] in (b"+", b"-"):
            neg = self.d[q:q + 1] == b"-"
            q += 1
        b = q
        while q < len(self.d) and 48 <= self.d[q] <= 57:
            q += 1
        if q == len(self.d):
            self.eof = True
        if q == b:
            self.fail = True
            return False, 0
        v, self.p = int(self.d[b:q]), q
        if signed:
            v = -v if neg else v
            if not -2 ** 63 <= v < 2 ** 63:
                self.fail = True
                return False, (2 ** 63 - 1 if v > 0 else -2 ** 63)
            return True, v
        if v >= 2 ** 64:
            self.fail = True
            return False, 2 ** 64 - 1
        return True, (-v) % 2 ** 64 if neg else v


def read_mapping(data, m):
    """read_sequence_to_taxon_id_mapping on the bytes of a file that opened; m: dict, the first entry of a key stays"""
    s, header_row, line = IStream(data), 0, b""
    for _ in range(10):
        got = s.getline()
        line = line if got is None else got
        if line[:1] != b"#":
            break
        header_row += 1
    if header_row > 0:
        header_row -= 1
    s = IStream(data)
    for _ in range(header_row):
        s.getline()
    if not s.good():
        return
    keycol = taxcol = 0
    for col, w in enumerate((s.getline() or b"").split()[1:]):
        if w == b"taxid":
            taxcol = col
        elif w in (b"accession.version", b"assembly_accession"):
            keycol = col
    if taxcol < 1:
        s, taxcol = IStream(data), 1
    key, taxid = b"", None
    while s.good():
        for _ in range(keycol):
            s.ignore(b"\t")
        w = s.word()
        key = key if w is None else w
        for _ in range(taxcol):
            s.ignore(b"\t")
        _, v = s.number(True)
        taxid = taxid if v is None else v
        s.ignore(b"\n")
        if taxid is not None:                        # (an entry with an undefined taxid: only {"": ?} of a file without data lines)
            m.setdefault(key, taxid)


def make_map(files):
    """files: [(path, bytes or None if it does not open)] of the genome files' directories, in std::set order of the directories"""
    m = {}
    for _, data in files:
        if data is not None:
            read_mapping(data, m)
    return m


def unique_directories(filenames):
    out = set()
    for f in filenames:
        i = max(f.rfind("/"), f.rfind("\\"))
        out.add(f if i < 0 else f[:i])
    return sorted(out, key=lambda d: d.encode())


def find_taxon_id(m, name):
    if not m or not name:
        return 0
    if name in m:
        return m[name]
    keys = sorted(m)
    i = bisect.bisect_right(keys, name)
    if i == len(keys) or keys[i][:len(name)] != name:
        return 0
    return m[keys[i]]


class Names:
    """name2tax_ of a database: names[t] = the name of target t (bytes)"""

    def __init__(self, names):
        self.by_name = {}
        for t, n in enumerate(names):
            self.by_name.setdefault(n, t)
        self.keys = sorted(self.by_name)

    def exact(self, s):
        return self.by_name.get(s) if s else None

    def similar(self, s):
        if not s:
            return None
        i = bisect.bisect_right(self.keys, s)
        if i == len(self.keys) or self.keys[i][:len(s)] != s:
            return None
        return self.by_name[self.keys[i]]

    def target_of(self, acc, accver, gi):
        """the target a record names: a function of the record alone"""
        t = self.exact(accver)
        if t is None:
            t = self.similar(acc)
            if t is None:
                t = self.exact(gi)
        return t


def accmap(text, names, unranked, parent, skip_first_line=True):
    """rank_targets_with_mapping_file over one file's bytes; names: Names; unranked (list of bool) and parent (list of int) are
    updated.  Returns the number of records read."""
    if not any(unranked):
        return 0
    s, n = IStream(text), 0
    if skip_first_line:
        s.getline()
    while True:
        acc, accver = s.word(), s.word()
        ok, taxid = s.number(False)
        gi = s.word()
        if acc is None or accver is None or not ok or gi is None:
            return n
        n += 1
        t = names.target_of(acc, accver, gi)
        if t is not None and unranked[t]:
            parent[t] = taxid - 2 ** 64 if taxid >= 2 ** 63 else taxid
            unranked[t] = False
            if not any(unranked):
                return n


_FIELD = rb"[^ \t\n\v\f\r]+"
_LINE = re.compile(rb"(?:" + _FIELD + rb"\t" + _FIELD + rb"\t[0-9]{1,19}\t" + _FIELD + rb"\r?\n)")


def is_strict(text, max_line=1024):
    """the strict form of include/mcq.h (mcq_accmap_chunk), line by line"""
    p = 0
    while p < len(text):
        m = _LINE.match(text, p)
        if not m or m.end() - p > max_line:
            return False
        p = m.end()
    return True
