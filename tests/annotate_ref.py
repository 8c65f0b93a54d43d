"""Python restatement of the reference's `annotate taxid` (src/mode_annotate.cpp) for the tests of mcq_annotate_*,
mcq_accmap_host_rule, mcq_accmap_create_rule and mcq_annotate_cli: the three id extractors (src/sequence_io.cpp:576-700) applied to
the WHOLE header line as annotate_with_taxid applies them, the rewrite of a header line (:265-298), the map of
read_mappings_from_file (:181-229) on the stream model of tests/taxmap_ref.py, and the loop over a file (:243-309) that ends at the
first empty line.  Pinned against the reference's own outputs by tests/test_annotate_ref.py."""
import taxmap_ref as tr

ACC, ACCVER, GI = 1, 2, 3          # MCQ_ACCMAP_RULE_ACC / _ACCVER / _GI: also the column's place in (acc, accver, taxid, gi) -> 0, 1, 3
PREFIXES = [b"GCF_", b"AC_", b"NC_", b"NG_", b"NS_", b"NT_", b"NW_", b"NZ_", b"MKHE", b"AE", b"AJ", b"AL", b"AM", b"AP", b"AY", b"BA",
            b"BK", b"BX", b"CC", b"CM", b"CP", b"CR", b"CT", b"CU", b"FM", b"FN", b"FO", b"FP", b"FQ", b"FR", b"HE", b"JH"]
_WS = b" \t\n\v\f\r"


def _end(t, start):
    """end_of_accession_number: the first of | blank - _ , that occurs AT ALL from start on, in this order of preference"""
    if start >= len(t):
        return len(t)
    for c in (b"|", b" ", b"-", b"_", b","):
        k = t.find(c, start)
        if k >= 0:
            return k
    return len(t)


def accver(t):
    if len(t) < 2:
        return b""
    for p in PREFIXES:
        i = t.find(p)
        if i < 0:
            continue
        s = t.find(b".", i + len(p))
        if s < 0 or s - i > 25:
            continue
        num = t[i:_end(t, s + 1)].strip(_WS)
        if num:
            return num
    s = t.find(b".", 1)
    if 0 <= s < 25:
        return t[:_end(t, s + 1)].strip(_WS)
    return b""


def acc(t):
    for p in PREFIXES:
        i = t.find(p)
        if i < 0:
            continue
        j = i + len(p)
        k = _end(t, j)
        dot = t.find(b".", j)
        if 0 <= dot < k:
            k = dot
        num = t[i:k].strip(_WS)
        if num:
            return num
    return b""


def gi(t):
    i = t.find(b"gi|")
    if i < 0:
        return b""
    i += 3
    j = t.find(b"|", i)
    if j < 0:
        j = t.find(b" ", i)
        if j < 0:
            j = len(t)
    return t[i:j].strip(_WS)


def header_id(line, id_type):
    return {ACC: acc, ACCVER: accver, GI: gi}[id_type](line)


def rewrite(line, has_id, taxid, fs=b" ", vs=b"|"):
    j = line.find(b"taxid")
    if j >= 0:
        k = line.find(vs, j + 4)
        if k >= 0:
            end = line.find(fs, k + 1)
            if end < 0:
                end = line.find(vs, k + 1)
            if end >= 0:
                line = line[:j] + line[end + 1:]
            elif j > 0:                          # erase(j, npos - j + 1): the rest of the line; for j == 0 the count wraps to 0
                line = line[:j]
    if has_id:
        ins = b"taxid" + vs + str(taxid).encode() + fs
        ipos = line.find(fs)
        line = line + fs + ins if ipos < 0 else line[:ipos + 1] + ins + line[ipos + 1:]
    return line


def read_mappings(text, id_type, m, skip_first_line=True):
    """read_mappings_from_file on the bytes of a file that opened: m (dict) keeps the first taxid of a key.  Returns the records read."""
    s, n = tr.IStream(text), 0
    if skip_first_line:
        s.getline()
    while True:
        a, av = s.word(), s.word()
        ok, taxid = s.number(False)
        g = s.word()
        if a is None or av is None or not ok or g is None:
            return n
        n += 1
        m.setdefault({ACC: a, ACCVER: av, GI: g}[id_type], taxid)


def accmap_rule(text, names, unranked, parent, rule, skip_first_line=True):
    """mcq_accmap_host_rule for rules 1 to 3 on the model of taxmap_ref.accmap: names[t] = the name of target t (the first of a name
    counts); unranked / parent are updated; the reading ends when nothing is left unranked.  Returns the records read."""
    if not any(unranked):
        return 0
    by_name = {}
    for t, nm in enumerate(names):
        by_name.setdefault(nm, t)
    s, n = tr.IStream(text), 0
    if skip_first_line:
        s.getline()
    while True:
        a, av = s.word(), s.word()
        ok, taxid = s.number(False)
        g = s.word()
        if a is None or av is None or not ok or g is None:
            return n
        n += 1
        t = by_name.get({ACC: a, ACCVER: av, GI: g}[rule])
        if t is not None and unranked[t]:
            parent[t] = taxid - 2 ** 64 if taxid >= 2 ** 63 else taxid
            unranked[t] = False
            if not any(unranked):
                return n


def annotate(text, m, id_type=ACCVER, fs=b" ", vs=b"|"):
    """annotate_with_taxid over the bytes of a file: getline's lines up to the first empty one, joined by LF, none behind the last"""
    out = []
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()                              # (the getline behind a last LF extracts nothing: an empty line, the loop ends)
    for line in lines:
        if not line:
            break
        if line[:1] in (b">", b"@"):
            i = header_id(line, id_type)
            line = rewrite(line, bool(i), m.get(i, 0), fs, vs)
        out.append(line)
    return b"\n".join(out)
