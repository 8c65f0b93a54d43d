"""The inputs of mcq_build_cli on the host (no GPU): the taxonomy dump parser and the genome reader of libmcq_host.so against
the golden databases the reference built from the same files, and against a Python restatement of the reference's reader."""
import importlib
import os
import random
import subprocess

import numpy as np
import pytest

import build_inputs as bi
from golden_util import Fixture
from read_corpus import _fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(tag, P) for tag, (Ps, _) in sorted(bi.FIXTURES.items()) if bi.has_build_inputs(tag) for P in Ps]


@pytest.fixture(scope="module")
def host():
    pkg = importlib.import_module("metacache-mpi_amd")
    pkg.build_host()
    return importlib.import_module("metacache-mpi_amd.host")


def test_every_fixture_with_inputs_is_covered():
    assert {t for t, _ in CASES} == {"mini", "tie", "noanc", "overpop", "wide"}


@pytest.mark.parametrize("tag,P", CASES)
def test_taxa_from_the_dump_and_the_headers_equal_the_golden_database(host, tag, P, tmp_path, monkeypatch):
    """nodes.dmp + names.dmp through mcq_taxdump_read, the genome headers through mcq_genome_reader_*, written as a shard file
    without a table and read back: the taxon list of the reference's own <tag>.db_0 -- ids, parents, ranks, names, source file,
    index and windows of every record, mcq_refdb_tgt2tax at `species` and at `sequence`, and the ranked lineages"""
    fx = Fixture(tag, P)
    work = bi.lay_out(tag, str(tmp_path / "w"))
    monkeypatch.chdir(work)                                  # the recorded file name is relative: genomes/all.fna
    files = host.genome_files(["genomes"])
    assert files == ["genomes/all.fna"]
    _, targets, lens, _ = host.read_genomes(files, 1 << 16)
    gold = host.RefDb(fx.shard_paths[0][: -len(".db_0")], 1)
    meta = host.RefDb(fx.shard_paths[0][: -len(".db_0")], P, meta_only=True)
    assert len(targets) == gold.info.n_targets
    windows = meta.tgt_windows()
    for t, rec in enumerate(targets):                        # rank 0 owns the targets with t % P == 0 (`windows` is set only there)
        rec["windows"] = int(windows[t]) if t % P == 0 else 0
    taxa = targets[::-1] + host.read_taxdump("tax")
    p = fx.params
    host.write_shard(str(tmp_path / "mine.db_0"), dict(k=p["k"], sketch_size=p["s"], winlen=p["winlen"], winstride=p["winstride"], q_k=p["qk"],
                                                       q_sketch_size=p["qs"], q_winlen=p["qwinlen"], q_winstride=p["qwinstride"],
                                                       max_locs_per_feature=p["maxlocs"]),
                     taxa, len(targets), np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.uint64))
    mine = host.RefDb(str(tmp_path / "mine"), 1)
    assert mine.info.n_taxa == gold.info.n_taxa and mine.info.n_targets == gold.info.n_targets
    assert bi.taxon_list(mine) == bi.taxon_list(gold)
    for rank in (host.RANK_SPECIES, host.RANK_SEQUENCE):
        assert np.array_equal(mine.tgt2tax(rank), gold.tgt2tax(rank))
    (lm, rm), (lg, rg) = mine.lineages(), gold.lineages()
    assert np.array_equal(lm, lg) and np.array_equal(rm, rg)


def _run_reader(host, tmp_path, contents, cap, io_bytes):
    names = []
    for i, data in enumerate(contents):
        names.append(str(tmp_path / ("g%02d.fa" % i)))
        if not os.path.exists(names[-1]):
            with open(names[-1], "wb") as f:
                f.write(data)
    return names, host.read_genomes(names, cap, io_bytes)


def _check(host, tmp_path, contents, cap, io_bytes):
    names, (bases, recs, lens, fills) = _run_reader(host, tmp_path, contents, cap, io_bytes)
    want = bi.read_genomes(list(zip(names, contents)))
    assert len(recs) == len(want), (cap, io_bytes)
    assert bases == b"".join(w[4] for w in want), (cap, io_bytes)
    assert lens == [len(w[4]) for w in want]
    for t, (r, w) in enumerate(zip(recs, want)):
        assert (r["id"], r["parent"], r["rank"], r["name"].encode("latin-1"), r["file"], r["index"]) == (-(t + 1), w[1], 0, w[0], w[2], w[3])
    assert fills == max(1, -(-len(bases) // cap) + (len(bases) % cap == 0 and len(bases) > 0))   # full buffers, then the one that meets the end
    return want


def test_reader_on_minis_genomes_at_every_buffer_size_from_a_line_to_the_file(host, tmp_path):
    """mini's genomes wrapped at 60 columns: every buffer size below a line and around it, every whole number of lines up to
    the file, and the file's size and more; the io buffer from one byte up"""
    import gzip
    with gzip.open(os.path.join(bi.GOLDEN, "mini", "genomes.fa.gz"), "rb") as f:
        one_line = f.read()
    out = []
    for line in one_line.split(b"\n"):
        out += [line] if line[:1] == b">" else [line[i:i + 60] for i in range(0, len(line), 60)]
    data = b"\n".join(out) + b"\n"
    total = len(b"".join(w[4] for w in bi.read_genomes([("x", data)])))
    assert total > 100000
    want = _check(host, tmp_path, [data], total, 1 << 20)
    assert [w[0] for w in want] == [b"NC_%06d.1 taxid" % (i + 1) for i in range(10)] and want[2][1] == 102     # (ends at the '|': see below)
    for cap in list(range(1, 123)) + list(range(180, total + 61, 60)) + [total - 1, total + 1, 2 * total]:
        _check(host, tmp_path, [data], cap, 1 << 16)
    for io in (1, 2, 3, 59, 60, 61, 62, 4096):
        for cap in (1, 60, 61, 1000, total):
            if io * cap >= 60 or cap == total:               # (one byte at a time into one base at a time: minutes for nothing new)
                _check(host, tmp_path, [data], cap, io)


def _corpus():
    rng = random.Random(4711)
    acc = lambda i: "NC_%06d.%d Some organism taxid|%d chromosome" % (i, 1 + i % 3, 100 + i)
    plain = _fasta(rng, 12, width=60)
    return {
        "one_line": [_fasta(rng, 20, hdr=acc)],
        "wrap60": [_fasta(rng, 20, width=60, hdr=acc)],
        "wrap80_several_files": [_fasta(rng, 7, width=80, hdr=acc), _fasta(rng, 9, width=80, hdr=lambda i: acc(i + 50))],
        "crlf": [_fasta(rng, 15, width=60, eol="\r\n", hdr=acc)],
        "crlf_plain_headers": [_fasta(rng, 10, width=60, eol="\r\n")],
        "no_final_newline": [_fasta(rng, 15, width=60, hdr=acc)[:-1]],
        "blank_lines": [_fasta(rng, 20, width=60, blank=True, hdr=acc)],
        "plain_headers": [plain],
        "long_records": [_fasta(rng, 4, width=60, lens=(1500, 3000), hdr=acc)],
        "same_name_twice": [_fasta(rng, 6, width=60, hdr=lambda i: acc(i % 4))],
        "same_file_twice": [plain, plain],
        "record_without_sequence_ends_its_file": [b">NC_000001.1 a\nACGT\n>NC_000002.1 b\n>NC_000003.1 c\nGGGG\n", b">NC_000004.1 d\nTTTT\n"],
        "header_at_the_end": [b">NC_000001.1 a\nACGT\nAC\n>NC_000002.1 b"],
        "no_header_first": [b"ACGT\n>NC_000001.1 a\nACGT\n", b"\n>NC_000002.1 a\nACGT\n", b">NC_000003.1 x\nAC\n"],
        "empty_file": [b"", b">NC_000003.1 x\nAC\n"],
        "at_sign_lines_are_sequence": [b">NC_000001.1 a\nACGT\n@AC\n+\nIIII\n>gi|12345|ref x\nAC\n"],
        "names": [b">gi|55|gb|XYZ some\nAC\n>AE017334 plain accession taxid|77|\nAC\n>NZ_ABCD01000001.1-suffix_a taxid 9 x\nGT\n"
                  b">weird.name_with,commas and|bars\nAA\n>x taxid|abc\nCC\n>y taxid\nTT\n>" + b"L" * 40 + b".1 far dot\nGG\n"],
    }


@pytest.mark.parametrize("case", sorted(_corpus()))
def test_reader_equals_the_reference_restated(host, case, tmp_path):
    contents = _corpus()[case]
    total = sum(len(c) for c in contents)
    for cap in [1, 2, 3, 7, 59, 60, 61, 64, 100, 1000, max(1, total)]:
        for io in (1, 5, 64, 1 << 16):
            _check(host, tmp_path, contents, cap, io)


def test_the_extension_decides_how_a_file_is_read(host, tmp_path, monkeypatch):
    """FASTA text under a FASTQ extension -- also a 5-character name, which the reference takes for FASTQ -- is left as the
    reference's FASTQ reader leaves it; without a known extension the first character decides; a directory among the names and
    a missing file are passed over; what the reference would read as FASTQ is an error here"""
    monkeypatch.chdir(tmp_path)
    contents = {"a.fq": b">NC_000001.1 a\nACGT\n", "b1.fa": b">NC_000002.1 b\nACGT\n", "long_name.fa": b">NC_000003.1 c\nAC\nGT\n",
                "noextension": b">NC_000004.1 d\nGG\n", "x.fasta.gz.txt": b">NC_000005.1 e\nTT\n", "at.fna": b"@NC_000006.1 f\nAC\n+\nII\n"}
    for n, d in contents.items():
        with open(n, "wb") as f:
            f.write(d)
    os.mkdir("adir.fa")
    names = ["a.fq", "adir.fa", "at.fna", "b1.fa", "long_name.fa", "missing.fa", "noextension", "x.fasta.gz.txt"]
    assert [bi.file_kind(n) for n in names] == [2, 1, 1, 2, 1, 1, 0, 0]
    want = bi.read_genomes([(n, contents.get(n, b"")) for n in names])
    assert [w[0] for w in want] == [b"NC_000003.1", b"NC_000004.1", b"NC_000005.1"]
    for cap, io in ((1, 1), (3, 2), (100, 64)):
        bases, recs, lens, _ = host.read_genomes(names, cap, io)
        assert bases == b"".join(w[4] for w in want)
        assert [(r["name"].encode(), r["file"], r["index"]) for r in recs] == [(w[0], w[2], w[3]) for w in want]
    for name, data in (("real.fq", b"@r1\nACGT\n+\nIIII\n"), ("sniffed", b"@r1\nACGT\n+\nIIII\n")):
        with open(name, "wb") as f:
            f.write(data)
        with pytest.raises(RuntimeError, match="FASTQ genome files are not supported"):
            host.read_genomes([name], 100, 64)


def test_names_and_parents_from_headers(host):
    for h in [b"NC_000001.1 taxid|101 synthetic", b"gi|55|gb|XYZ some", b"AE017334 plain", b"NZ_ABCD01000001.1-x_y", b"plain header", b"a.b c",
              b"x" * 30 + b".1", b"r1 taxid|12|x", b"r1 taxid 7", b"r1 taxid|", b"r1 taxid", b"", b"N", b"NC_1.2\r", b"seq taxid|5\r"]:
        assert host.target_name(h) == bi.target_name(h), h
        assert host.target_parent_taxid(h) == bi.parent_taxid(h), h
    # the accession ends at the first '|' if the text has one at all, and only else at a ' ' (src/sequence_io.cpp:576-598): the
    # name the golden databases carry for this header
    assert host.target_name(b"NC_000001.1 taxid|101 synthetic") == b"NC_000001.1 taxid"
    assert host.target_name(b"NC_000001.1 Escherichia coli") == b"NC_000001.1"
    assert host.target_parent_taxid(b"NC_000001.1 taxid|101 synthetic") == 101


def test_taxdump_merged_ranks_and_first_record_wins(host, tmp_path):
    d = tmp_path / "tax"
    d.mkdir()
    (d / "nodes.dmp").write_text("1\t|\t1\t|\tno rank\t|\t\t|\n2\t|\t1\t|\tsuperkingdom\t|\t\t|\n9\t|\t2\t|\tspecies group\t|\t\t|\n"
                                 "7\t|\t5\t|\tspecies\t|\t\t|\n9\t|\t1\t|\tgenus\t|\t\t|\n11\t|\t9\t|\tstrain\t|\t\t|\n12\t|\t9\t|\tspecies\t|\t\t|\n")
    (d / "names.dmp").write_text("1\t|\tall\t|\t\t|\tsynonym\t|\n1\t|\troot\t|\t\t|\tscientific name\t|\n2\t|\tBacteria\t|\tBacteria <bacteria>\t|\tscientific name\t|\n"
                                 "9\t|\tA b  group\t|\t\t|\tscientific name\t|\n9\t|\tother\t|\t\t|\tscientific name\t|\n7\t|\tA seven\t|\t\t|\tauthority\t|\n")
    (d / "merged.dmp").write_text("5\t|\t9\t|\n12\t|\t13\t|\n")
    recs = {r["id"]: r for r in host.read_taxdump(str(d))}
    assert [r["id"] for r in host.read_taxdump(str(d))] == sorted(recs)
    assert recs[1]["rank"] == host.RANK_ROOT and recs[1]["name"] == "root"
    assert recs[2]["rank"] == 19 and recs[2]["name"] == "Bacteria"
    assert recs[9] == dict(id=9, parent=2, rank=5, name="A b group", file="", index=0, windows=0)       # species group; the first record of id 9
    assert recs[5]["parent"] == 9 and recs[5]["rank"] == host.RANK_NONE and recs[5]["name"] == ""      # an old id of merged.dmp
    assert recs[7]["parent"] == 9 and recs[7]["name"] == "--"                                           # parent 5 -> 9; no scientific name
    assert recs[11]["rank"] == host.RANK_NONE                                                            # a rank name the reference does not know
    assert recs[12]["parent"] == 13 and recs[13]["parent"] == 9 and recs[13]["name"] == "--"            # node 12 becomes 13, after the merged record of 12


def test_a_directory_is_expanded_recursively_and_sorted(host, tmp_path):
    for rel in ("g/b/2.fa", "g/a.fa", "g/b/1.fa", "g/c/d/x.fna", "z.fa"):
        p = tmp_path / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(">s\nA\n")
    g = str(tmp_path / "g")
    assert host.genome_files([str(tmp_path / "z.fa"), g + "/"]) == sorted([g + "/a.fa", g + "/b/1.fa", g + "/b/2.fa", g + "/c/d/x.fna", str(tmp_path / "z.fa")])
    assert host.genome_files(["no/such/file.fa"]) == ["no/such/file.fa"]


KEEP_ENV = "MCQ_BUILD_CLI_KEEP_SHARDS"     # the directory tests/test_gpu_build_cli.py copies mini's files (P = 2) to when it is set


def test_the_references_reader_loads_the_shards_mcq_build_cli_wrote(tmp_path):
    """only where the reference has been compiled (oracle/_ref/ref_query: its database::read and query path) and the GPU test
    left its files: the reference reads what mcq_build_cli wrote and gives, rank by rank, the parameters, lineages, taxa, match
    lists and candidates it gives on the files its own build wrote"""
    ref_query = os.path.join(ROOT, "oracle", "_ref", "ref_query")
    kept = os.environ.get(KEEP_ENV, "")
    if not os.path.exists(ref_query) or not all(os.path.exists(os.path.join(kept, "mini.db_%d" % r)) for r in (0, 1)):
        pytest.skip("needs oracle/_ref/ref_query (make -C oracle ref, where the reference's sources are) and, in the directory %s names, "
                    "mini.db_0 and mini.db_1 as `pytest -m gpu tests/test_gpu_build_cli.py -k 'shard_files and mini-2'` leaves them "
                    "there when the variable is set" % KEEP_ENV)
    fx = Fixture("mini", 2)
    with open(tmp_path / "q.txt", "w") as f:
        for a, b in list(zip(fx.r1, fx.r2))[:32]:
            f.write("%s %s\n" % (a, b))
    out = []
    for prefix in (os.path.join(kept, "mini"), fx.shard_paths[0][: -len(".db_0")]):
        r = subprocess.run([ref_query, prefix, "2", str(tmp_path / "q.txt"), str(fx.maxcand), fx.q["lowest"], "0"],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        out.append(r.stdout)
    assert out[0].count("\nM ") == 64 and out[0] == out[1]
