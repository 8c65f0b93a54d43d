"""The reference's abundance tables from per-taxon counts (mcq_refdb_abundance_text; no GPU): the plain table and the
estimate to a rank, byte for byte against what the reference wrote (tests/golden/*/P*/cli_abund_*), plus synthetic
taxonomies for the corners of estimate_abundance (src/classification.cpp:362-428)."""
import gzip
import importlib
import os
import re

import numpy as np
import pytest

from golden_util import GOLDEN

host = importlib.import_module("metacache-mpi_amd.host")
NO = 0xFFFFFFFF
PLAIN = "# query summary: number of queries mapped per taxon"
EST = "# estimated abundance (number of queries) per "
RANKS = ["sequence", "form", "variety", "subspecies", "species", "subgenus", "genus", "subtribe", "tribe", "subfamily", "family",
         "suborder", "order", "subclass", "class", "subphylum", "phylum", "subkingdom", "kingdom", "domain", "root", "none"]


def _read(tag, P, name):
    with gzip.open(os.path.join(GOLDEN, tag, "P%d" % P, name), "rt") as f:
        return f.read()


def _sections(text):
    """{header line: table text incl. the header line} of every abundance table in a -out / abundance file"""
    out, cur = {}, None
    for line in text.split("\n"):
        if line.startswith(PLAIN) or line.startswith(EST):
            cur = line; out[cur] = line + "\n"
        elif cur and line and not line.startswith("#"):
            out[cur] += line + "\n"
        else:
            cur = None
    return out


def _total(text):
    root = int(re.search(r"^#   root .*\((\d+)\)$", text, re.M).group(1))
    m = re.search(r"^# unclassified: .*\((\d+)\)$", text, re.M)
    return root + (int(m.group(1)) if m else 0)


def _refdb(tag, P):
    prefix = os.path.join(GOLDEN, tag, "P%d" % P, tag)
    db = host.RefDb(prefix, P)
    names = {"%s:%s" % (RANKS[db.taxon_rank(i)], db.taxon_name(i)): i for i in range(db.info.n_taxa)}
    return db, names


@pytest.mark.parametrize("tag,P", [("mini", 4), ("tie", 2)])
def test_tables_equal_the_references(tag, P):
    db, names = _refdb(tag, P)
    both = _read(tag, P, "cli_abund_both_genus.out.gz")
    plain = _sections(both)[PLAIN]
    counts = np.zeros(db.info.n_taxa, np.uint64)
    for line in plain.split("\n")[1:-1]:
        name, cnt, _ = line.split("\t|\t")
        counts[names[name]] = int(cnt)
    total = _total(both)
    assert db.abundance_text(counts, total) == plain
    checked = 0
    for variant in ("species", "both_genus", "seq", "file", "nomap"):
        text = _read(tag, P, "cli_abund_%s.out.gz" % variant)
        if variant == "file":
            text = _read(tag, P, "cli_abund_file.ab.txt.gz")
        for head, table in _sections(text).items():
            rank = host.RANK_NONE if head == PLAIN else host.rank_from_name(head[len(EST):])
            assert db.abundance_text(counts, total, rank) == table, (variant, head)
            checked += 1
    assert checked == 7
    if tag == "mini":            # 188 species-level, 6 family-level reads: the family's reads are redistributed
        assert counts.sum() == 194 and "family:" in plain


# ---- synthetic taxonomies ---------------------------------------------------------------------------------------------
def _restated(taxa, lin, counts, rank):
    """estimate_abundance + show_abundance_table restated in numpy float32 / Python ints, op for op"""
    f32 = np.float32
    key = lambda i: (-taxa[i][1], taxa[i][0])
    m = {i: f32(c) for i, c in enumerate(counts) if c}
    if rank != host.RANK_NONE:
        if rank != 0:
            for i in sorted(m, key=key):
                if key(i) < (-(rank - 1), 0):
                    continue
                anc = next((a for a in lin[i][rank:21] if a != NO), NO)
                if anc != NO:
                    m[anc] = f32(m.get(anc, f32(0)) + m[i]); del m[i]
        w = {i: 0 for i in m}; ch = {}
        for i in sorted(m, key=key, reverse=True):
            for r in range((taxa[i][1] + 1) & 0xFF, 21):
                p = int(lin[i][r])
                if p != NO and p in w:
                    w[p] = int(f32(f32(w[p]) + f32(f32(w[i]) + m[i])))
                    ch.setdefault(p, []).append(i)
                    break
        for i in sorted(m, key=key):
            if i in ch:
                s = f32(w[i])
                for c in ch[i]:
                    m[c] = f32(m[c] + f32(f32(m[i] * f32(m[c] + f32(w[c]))) / s))
                del m[i]
    total = sum(counts) + 7
    return "".join("%s:%s\t|\t%g\t|\t%g%%\n" % (RANKS[taxa[i][1]], taxa[i][2], float(m[i]), float(m[i]) / float(total) * 100)
                   for i in sorted(m, key=key)), total


def _synthetic(tmp_path):
    """root > domain > {genus G1 > species S1, S2 ; species S3 directly under the domain (no genus); family F (no genus below)};
    sequence-level taxa (negative ids) under S1, S2, F, under G1 directly (no species) and one without any parent"""
    recs = [(1, 1, 20, "root"), (2, 1, 19, "Dom"), (10, 2, 6, "G1"), (11, 10, 4, "S1"), (12, 10, 4, "S2"), (13, 2, 4, "S3"),
            (14, 2, 10, "F"), (-1, 11, 0, "seqA"), (-2, 11, 0, "seqB"), (-3, 12, 0, "seqC"), (-4, 14, 0, "seqD"),
            (-5, 10, 0, "seqE"), (-6, 0, 0, "seqF")]
    taxa = [dict(id=i, parent=p, rank=r, name=n, file="", index=0, windows=0) for i, p, r, n in recs]
    path = str(tmp_path / "syn.db_0")
    host.write_shard(path, dict(k=16, sketch_size=16, winlen=128, winstride=113, q_k=16, q_sketch_size=16, q_winlen=128,
                                q_winstride=113, max_locs_per_feature=254), taxa, 6, np.zeros(0, np.uint32),
                     np.zeros(1, np.uint64), np.zeros(0, np.uint64))
    db = host.RefDb(str(tmp_path / "syn"), 1)
    lin, _ = db.lineages()
    return db, [(i, r, n) for i, _, r, n in recs], lin


@pytest.mark.parametrize("rank", ["none", "sequence", "form", "species", "genus", "family", "domain"])
@pytest.mark.parametrize("case", ["mixed", "big"])
def test_synthetic_estimates_follow_the_restatement(tmp_path, rank, case):
    db, taxa, lin = _synthetic(tmp_path)
    rng = np.random.default_rng(5)
    counts = rng.integers(1, 50, len(taxa)).astype(np.uint64)
    counts[0] = 0                                          # nothing on root
    if case == "big":
        counts[7] = (1 << 24) + 1                          # one conversion of the exact count: 16777217 -> 16777216.0f
        counts[3] = 3 << 25
    r = host.RANK_NONE if rank == "none" else host.rank_from_name(rank)
    want, total = _restated(taxa, lin, [int(c) for c in counts], r)
    got = db.abundance_text(counts, total, r)
    head, body = got.split("\n", 1)
    assert head == (PLAIN if rank == "none" else EST + rank)
    assert body == want


def test_synthetic_corners(tmp_path):
    db, taxa, lin = _synthetic(tmp_path)
    idx = {t[2]: i for i, t in enumerate(taxa)}
    counts = np.zeros(len(taxa), np.uint64)
    for n, c in (("seqA", 3), ("seqE", 5), ("seqF", 2), ("F", 4), ("S3", 1)):
        counts[idx[n]] = c
    # species: seqA -> S1; seqE has no species ancestor -> G1 (first ranked ancestor above); seqF has none and stays;
    # F and S3 are at or above the rank and stay.  G1 then hands its 5 to S1, its only child.
    text = db.abundance_text(counts, 20, host.RANK_SPECIES)
    assert text == (EST + "species\n" "family:F\t|\t4\t|\t20%\n" "species:S1\t|\t8\t|\t40%\n" "species:S3\t|\t1\t|\t5%\n"
                    "sequence:seqF\t|\t2\t|\t10%\n")
    # form: lower_bound(taxon{id 0, rank sequence}) skips the sequence-level taxa (negative ids): nothing is pruned
    text = db.abundance_text(counts, 20, host.rank_from_name("form"))
    assert "sequence:seqA\t|\t" in text and "sequence:seqF\t|\t2\t|\t10%" in text
    # sequence: no pruning, the counts of the parents go down to the sequences
    text = db.abundance_text(counts, 20, host.RANK_SEQUENCE)
    assert "sequence:seqE" in text and "species:S3" in text
    # past 2^24 on one taxon: the exact count, converted to float once
    counts[:] = 0; counts[idx["S1"]] = (1 << 24) + 1
    assert db.abundance_text(counts, (1 << 24) + 1) == PLAIN + "\nspecies:S1\t|\t1.67772e+07\t|\t100%\n"
    # root is not an estimation rank (the reference ignores -abundance-per root)
    with pytest.raises(RuntimeError):
        db.abundance_text(counts, 1, host.RANK_ROOT)
    # the length without a buffer equals the text
    assert len(db.abundance_text(counts, 1)) > 0
