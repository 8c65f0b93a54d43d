"""What the build tests share (tests/test_host_build_inputs.py, tests/test_gpu_build_cli.py): a fixture's genomes and taxonomy
laid out as the reference's build was given them, a Python restatement of how the reference reads genome files and names
their sequences (src/sequence_io.cpp:121-170, :576-748; src/mode_build.cpp:578-646; src/sketch_database.h:519-563), and the
comparison of two databases' taxon lists."""
import gzip
import os
import shutil

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# fixture -> (rank counts with golden shard files, build options of tests/golden/make_golden.py)
FIXTURES = {"mini": ((2, 4, 8), []), "tie": ((2, 4), []), "noanc": ((2, 4), []),
            "overpop": ((2, 4), ["-remove-overpopulated-features"]), "wide": ((16,), [])}


def has_build_inputs(tag):
    return all(os.path.exists(os.path.join(GOLDEN, tag, f)) for f in ("nodes.dmp", "names.dmp", "genomes.fa.gz"))


def lay_out(tag, work):
    """work/genomes/all.fna and work/tax/{nodes,names}.dmp: the directory `metacache build <tag> genomes -taxonomy tax` ran in
    when the fixture was made (the file name recorded in the golden taxa is genomes/all.fna)"""
    os.makedirs(os.path.join(work, "genomes")); os.makedirs(os.path.join(work, "tax"))
    with gzip.open(os.path.join(GOLDEN, tag, "genomes.fa.gz"), "rb") as f, open(os.path.join(work, "genomes", "all.fna"), "wb") as o:
        o.write(f.read())
    for n in ("nodes.dmp", "names.dmp"):
        shutil.copy(os.path.join(GOLDEN, tag, n), os.path.join(work, "tax", n))
    return work


# ---- the reference's naming of a sequence, restated ------------------------------------------------------------------------
_PREFIXES = [b"GCF_", b"AC_", b"NC_", b"NG_", b"NS_", b"NT_", b"NW_", b"NZ_", b"MKHE", b"AE", b"AJ", b"AL", b"AM", b"AP", b"AY", b"BA",
             b"BK", b"BX", b"CC", b"CM", b"CP", b"CR", b"CT", b"CU", b"FM", b"FN", b"FO", b"FP", b"FQ", b"FR", b"HE", b"JH"]


def _end(t, start):
    if start >= len(t):
        return len(t)
    for c in (b"|", b" ", b"-", b"_", b","):
        k = t.find(c, start)
        if k >= 0:
            return k
    return len(t)


def target_name(h):
    if not h:
        return h
    if len(h) >= 2:
        for p in _PREFIXES:
            i = h.find(p)
            if i < 0:
                continue
            s = h.find(b".", i + len(p))
            if s < 0 or s - i > 25:
                continue
            num = h[i:_end(h, s + 1)].strip()
            if num:
                return num
        s = h.find(b".", 1)
        if 0 <= s < 25:
            num = h[:_end(h, s + 1)].strip()
            if num:
                return num
    for p in _PREFIXES:
        i = h.find(p)
        if i < 0:
            continue
        j = i + len(p)
        k = _end(h, j)
        dot = h.find(b".", j)
        if 0 <= dot < k:
            k = dot
        num = h[i:k].strip()
        if num:
            return num
    i = h.find(b"gi|")
    if i >= 0:
        i += 3
        j = h.find(b"|", i)
        if j < 0:
            j = h.find(b" ", i)
            if j < 0:
                j = len(h)
        num = h[i:j].strip()
        if num:
            return num
    return h


def parent_taxid(h):
    i = h.find(b"taxid")
    if i < 0:
        return 0
    i += 6
    j = h.find(b"|", i)
    if j < 0:
        j = h.find(b" ", i)
        if j < 0:
            j = len(h)
    digits = h[i:j].lstrip()
    n = 0
    while n < len(digits) and digits[n:n + 1].isdigit():
        n += 1
    return int(digits[:n]) if n else 0


def file_kind(f):
    """1 = FASTA by its extension, 2 = FASTQ by its extension, 0 = by its first character: make_sequence_reader's comparisons in its
    unsigned arithmetic (the first ".fa" must be the last three characters; for a name shorter than ".fastq" n - 6 wraps to npos)"""
    f = os.fsencode(f)
    n = len(f)

    def ends(ext):
        i = f.find(ext)
        return (i if i >= 0 else 2 ** 64 - 1) == (n - len(ext)) % 2 ** 64
    if ends(b".fq") or ends(b".fnq") or ends(b".fastq"):
        return 2
    if ends(b".fa") or ends(b".fna") or ends(b".fasta"):
        return 1
    return 0


def read_genomes(files):
    """files: [(name, bytes)] in reading order -> [(taxon name, parent taxid, file name, index in file, sequence)], one per target"""
    out, taken = [], set()
    for fname, data in files:
        lines = data.split(b"\n")                    # getline; after a final '\n' one more (failed) getline adds nothing
        if not data or lines[0][:1] != b">" or file_kind(fname) == 2:
            continue                                 # "expected header char > not found" / "malformed fastq file": the file is left
        i = index = 0
        while i < len(lines):
            header = lines[i][1:]
            i += 1; index += 1
            seq = []
            while i < len(lines) and lines[i][:1] != b">":
                seq.append(lines[i]); i += 1
            seq = b"".join(seq)
            if not seq:
                break                                # "zero-length sequence": the file is left
            name = target_name(header)
            if name in taken:
                continue                             # non-unique sequence id: not added, no target id
            taken.add(name)
            out.append((name, parent_taxid(header), fname, index, seq))
    return out


def taxon_list(rdb):
    """every taxon record of an opened database (host.RefDb), in file order"""
    return [dict(id=rdb.taxon_id(k), parent=rdb.taxon_parent(k), rank=rdb.taxon_rank(k), name=rdb.taxon_name(k),
                 source=rdb.taxon_source(k)) for k in range(rdb.info.n_taxa)]
