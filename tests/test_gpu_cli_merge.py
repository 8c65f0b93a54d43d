"""mcq_merge_cli against the reference's merged -out files (tests/golden/merge, make_golden_merge.py: three databases of disjoint thirds
of `mini`'s genomes, the `mini` reads and 96 pairs whose mates lie in two databases), byte for byte bar the two measured lines; on
mcq_query_cli's own result files against the restatement (tests/merge_ref.py); and its rejections."""
import gzip
import importlib
import json
import os
import re
import subprocess

import pytest

import merge_ref as ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "merge")
MINI = os.path.join(HERE, "golden", "mini")
SETS = {"tophits": ["-maxcand", "4", "-tophits", "-queryids"],
        "lineage": ["-maxcand", "4", "-taxids", "-lineage"],
        "abundance": ["-maxcand", "4", "-abundance-per", "species", "-mapped-only"],
        "genus": ["-maxcand", "2", "-highest", "genus"]}


def _norm(text):
    text = re.sub(r"^# time:    .*$", "# time:    T ms", text, flags=re.M)
    return re.sub(r"^# speed:   .*$", "# speed:   S queries/min", text, flags=re.M)


def _golden(name):
    with gzip.open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


@pytest.fixture
def inputs(tmp_path):
    os.mkdir(tmp_path / "tax")
    for n in ("nodes.dmp", "names.dmp"):
        (tmp_path / "tax" / n).write_bytes(open(os.path.join(MINI, n), "rb").read())
    for k in range(3):
        (tmp_path / ("res_%d.txt" % k)).write_bytes(_golden("res_%d.txt.gz" % k))
    return tmp_path


def _merge(d, files, extra, out="m.txt"):
    pkg = importlib.import_module("metacache-mpi_amd")
    return subprocess.run([pkg.merge_cli_path()] + files + ["-taxonomy", "tax", "-hitmin", "4", "-lowest", "species"] + extra + ["-out", out],
                          cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)


@pytest.mark.parametrize("how", [["-parser", "gpu"], ["-parser", "host"], ["-parser", "gpu", "-read-chunk", "3000"], ["-parser", "host", "-read-chunk", "3000"]],
                         ids=["gpu", "host", "gpu_small_chunks", "host_small_chunks"])
@pytest.mark.parametrize("name", sorted(SETS))
def test_the_four_golden_merges_byte_for_byte(inputs, name, how):
    r = _merge(inputs, ["res_0.txt", "res_1.txt", "res_2.txt"], SETS[name] + how)
    assert r.returncode == 0, r.stderr
    assert _norm(open(inputs / "m.txt").read()) == _norm(_golden("merged_%s.out.gz" % name).decode())
    if "-read-chunk" in how:                                    # (every file took several chunks)
        n = [int(x) for x in re.findall(r"chunks parsed on the GPU: (\d+), on the host: (\d+)", r.stderr)[0]]
        assert sum(n) >= 9 and (n[0] == 0) == (how[1] == "host")
    elif how[1] == "gpu":
        assert "on the GPU: 3, on the host: 0" in r.stderr      # (the reference's own result files are strict)


def test_a_directory_of_files_and_the_order_they_are_named_in(inputs):
    os.mkdir(inputs / "d")
    for k in range(3):
        os.rename(inputs / ("res_%d.txt" % k), inputs / "d" / ("res_%d.txt" % k))
    r = _merge(inputs, ["d"], SETS["tophits"])
    assert r.returncode == 0, r.stderr
    got = _norm(open(inputs / "m.txt").read())
    assert got == _norm(_golden("merged_tophits.out.gz").decode()).replace("# res_", "# d/res_")
    r = _merge(inputs, ["d/res_2.txt", "d/res_0.txt", "d/res_1.txt"], SETS["tophits"], "m2.txt")       # (sorted before they are read)
    assert r.returncode == 0 and _norm(open(inputs / "m2.txt").read()) == got


def test_the_projects_own_result_files_are_mergeable(tmp_path, inputs):
    """mcq_query_cli on mini/P2 and on mini/P4 with -tophits -queryids -lowest species, then the merge of the two outputs, against the
    restatement: merged top_hits, header and classification of every read"""
    pkg = importlib.import_module("metacache-mpi_amd")
    with open(os.path.join(MINI, "queries.json")) as f:
        q = json.load(f)
    for fn, seqs in (("r1.fq", q["r1"]), ("r2.fq", q["r2"])):
        with open(inputs / fn, "w") as f:
            for n, s in zip(q["names"], seqs):
                f.write("@%s\n%s\n+\n%s\n" % (n, s, "I" * len(s)))
    for P in (2, 4):
        r = subprocess.run([pkg.cli_path(), os.path.join(MINI, "P%d" % P, "mini"), str(P), "r1.fq", "r2.fq", "-pairfiles", "-tophits", "-queryids",
                            "-lowest", "species", "-maxcand", "4", "-hitmin", "4", "-out", "own_%d.txt" % P],
                           cwd=inputs, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
    r = _merge(inputs, ["own_2.txt", "own_4.txt"], SETS["tophits"])
    assert r.returncode == 0, r.stderr
    assert "on the host: 0" in r.stderr                          # (the project's files are strict)
    host = importlib.import_module("metacache-mpi_amd.host")
    T = ref.Tax.of_dump(os.path.join(MINI, "nodes.dmp"))
    names = {int(l.split("|")[0]): l.split("|")[1].strip() for l in open(os.path.join(MINI, "names.dmp"))}
    want = ref.Merged(T, len(q["names"]), 4)
    for P in (2, 4):
        col, begin, n = host.results_properties(str(inputs / ("own_%d.txt" % P)))
        assert (col, n) == (2, len(q["names"]))
        want.read_results(open(inputs / ("own_%d.txt" % P), "rb").read()[begin:], col)
    lines = [l for l in open(inputs / "m.txt").read().split("\n") if l and not l.startswith("#")]
    assert len(lines) == len(q["names"])
    for i, l in enumerate(lines):
        best = ref.classify(want.lists[i], T, 4, 1.0, ref.RANK["domain"])
        cls = "--" if best == ref.NONE else "%s:%s" % (ref.RANKS[T.rank[best]], names[T.ids[best]])
        assert l == "\t|\t".join([str(i + 1), want.headers[i].decode(), ",".join("%d:%d" % (T.ids[t], h) for t, h in want.lists[i]), cls]), i


REJECTED = {
    "a_file_with_another_line_count": (lambda t: re.sub(rb"\n293\t\|[^\n]*", b"", t), "mapping lines"),        # (its last mapping line is gone)
    "a_file_without_query_id": (lambda t: t.replace(b"TABLE_LAYOUT: query_id\t|\t", b"TABLE_LAYOUT: "), "no query_id"),
    "a_file_classified_at_sequence": (lambda t: t.replace(b"ranks from 'species'", b"ranks from 'sequence'"), "sequence level"),
}


@pytest.mark.parametrize("what", sorted(REJECTED))
def test_a_file_that_is_rejected_ends_the_run_and_nothing_is_written(inputs, what):
    change, why = REJECTED[what]
    text = (inputs / "res_1.txt").read_bytes()
    assert change(text) != text
    (inputs / "res_1.txt").write_bytes(change(text))
    r = _merge(inputs, ["res_0.txt", "res_1.txt", "res_2.txt"], SETS["tophits"])
    assert r.returncode != 0 and why in r.stderr and "res_1.txt" in r.stderr and len(r.stderr.strip().split("\n")) == 1
    assert not os.path.exists(inputs / "m.txt")


def test_one_file_only_an_option_it_does_not_have_and_a_line_the_reference_hangs_on(inputs):
    r = _merge(inputs, ["res_0.txt"], SETS["tophits"])
    assert r.returncode != 0 and "two result files" in r.stderr and not os.path.exists(inputs / "m.txt")
    r = _merge(inputs, ["res_0.txt", "res_1.txt"], ["-separator", ";"])
    assert r.returncode != 0 and "-separator" in r.stderr and len(r.stderr.strip().split("\n")) == 1 and not os.path.exists(inputs / "m.txt")
    text = (inputs / "res_1.txt").read_bytes()
    bad = text.replace(b"\t|\tq0002_g3\t|\t", b"\t|\tq0002_g3 taxid|5\t|\t")
    assert bad != text
    (inputs / "res_1.txt").write_bytes(bad)
    r = _merge(inputs, ["res_0.txt", "res_1.txt", "res_2.txt"], SETS["tophits"])
    line_no = bad[:bad.index(b"q0002_g3 taxid|5")].count(b"\n") + 1
    assert r.returncode != 0 and "res_1.txt: line %d: " % line_no in r.stderr
