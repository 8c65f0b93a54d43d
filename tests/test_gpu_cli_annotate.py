"""mcq_annotate_cli against the files the reference's `annotate taxid` wrote (tests/golden/annotate, make_golden_annotate.py) byte for
byte -- joined on the GPU, on the host, and in several chunks per mapping file --, and -outdir (not in the reference) against the
restatement tests/annotate_ref.py on the genome directories of the `accmap` fixture."""
import importlib
import os
import subprocess

import pytest

import annotate_ref as ar
import taxmap_inputs as ti
from test_annotate_ref import MAPPINGS, RUNS, golden, mapping

pytestmark = pytest.mark.gpu
ID_OPT = {ar.ACC: "-id=acc", ar.ACCVER: "-id=accver", ar.GI: "-id=gi"}
ROUTES = {"gpu": ["-mapper", "gpu"], "host": ["-mapper", "host"], "chunks": ["-map-chunk", "4096"], "small_io": ["-io-bytes", "128"]}


def _run(*args, cwd=None):
    pkg = importlib.import_module("metacache-mpi_amd")
    return subprocess.run([pkg.annotate_cli_path()] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=cwd, timeout=120)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("annotate_in")
    for name in ("in.fa", "gap.fa", "reads.fq"):
        (d / name).write_bytes(golden(name))
    return d


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("infile,outfile,id_type,fs,vs", RUNS, ids=[r[1] for r in RUNS])
def test_golden_outputs_byte_for_byte(inputs, tmp_path, infile, outfile, id_type, fs, vs, route):
    opts = ["-field-sep", fs.decode(), "-value-sep", vs.decode(), ID_OPT[id_type]] + ROUTES[route]
    r = _run("taxid", inputs / infile, *MAPPINGS, "-out", tmp_path / "o", *opts)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "o").read_bytes() == golden(outfile)
    out = r.stdout.decode()
    assert out.startswith("Annotating sequences in '%s' with taxonomic ids.\nOutput will be written to '%s'\n" % (inputs / infile, tmp_path / "o"))
    assert [l for l in out.splitlines() if l.startswith("Processing")] == ["Processing mappings in file '%s'" % m for m in MAPPINGS]
    assert out.endswith("Mapping ... complete.\n")
    assert (b"the output ends at the empty line at byte" in r.stderr) == (infile == "gap.fa")


def test_the_text_on_stdout_and_the_defaults(inputs):
    """without -out the annotated text alone is stdout and the reference's lines go to stderr; accver and " ", "|" are the defaults"""
    r = _run("taxid", inputs / "in.fa", *MAPPINGS)
    assert r.returncode == 0 and r.stdout == golden("in.accver.fa")
    assert b"Annotating sequences in" in r.stderr and b"'stdout'" in r.stderr and r.stderr.count(b"Processing mappings in file") == 3
    r = _run("taxid", inputs / "in.fa", *MAPPINGS, "-field-separator", "_", "-value-separator", ":")
    assert r.returncode == 0 and r.stdout == golden("in.sep.fa")
    r = _run("taxid", inputs / "in.fa", os.path.dirname(MAPPINGS[0]), "-id=acc")             # the directory: its files in name order
    want = {}
    for n in sorted(os.listdir(os.path.dirname(MAPPINGS[0]))):
        with open(os.path.join(os.path.dirname(MAPPINGS[0]), n), "rb") as f:
            ar.read_mappings(f.read(), ar.ACC, want)
    assert r.returncode == 0 and r.stdout == ar.annotate(golden("in.fa"), want, ar.ACC)


@pytest.mark.parametrize("chunk", [[], ["-map-chunk", "300"]])
def test_a_mapping_file_that_is_not_strict_goes_through_the_host_parser(inputs, tmp_path, chunk):
    """blank-separated columns, and a record that runs across two lines: the same bytes, by the host route from the first chunk on or
    (-map-chunk 300) behind strict chunks that the GPU took"""
    texts = [open(m, "rb").read() for m in MAPPINGS]
    lines = texts[0].split(b"\n")
    lines[40] = lines[40].replace(b"\t", b" ")                                          # line 40 of nucl_gb: blanks
    lines[60] = lines[60].replace(b"\t", b"\n", 1)                                      # a record across two lines
    blanks = [tmp_path / "gb.map", tmp_path / "wgs.map", MAPPINGS[2]]
    blanks[0].write_bytes(b"\n".join(lines))
    blanks[1].write_bytes(texts[1].replace(b"\t", b"  "))
    for id_type, outfile in ((ar.ACCVER, "in.accver.fa"), (ar.ACC, "in.acc.fa"), (ar.GI, "in.gi.fa")):
        r = _run("taxid", inputs / "in.fa", *blanks, "-out", tmp_path / "o", ID_OPT[id_type], "-timing", *chunk)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / "o").read_bytes() == golden(outfile)
        assert b"host parser" in r.stderr and b"in 2 files" in r.stderr, r.stderr


def test_an_unreadable_mapping_file_is_passed_over(inputs, tmp_path):
    r = _run("taxid", inputs / "in.fa", MAPPINGS[0], tmp_path / "nosuch.accession2taxid", MAPPINGS[1], MAPPINGS[2], "-out", tmp_path / "o")
    assert r.returncode == 0, r.stderr
    assert ("File '%s' could not be read." % (tmp_path / "nosuch.accession2taxid")).encode() in r.stderr
    assert (tmp_path / "o").read_bytes() == golden("in.accver.fa") and r.stdout.count(b"Processing mappings in file") == 3


@pytest.mark.parametrize("id_type", [ar.ACCVER, ar.GI])
def test_outdir_over_the_genome_directories(tmp_path, id_type):
    host = importlib.import_module("metacache-mpi_amd.host")
    work = ti.lay_out(str(tmp_path / "w"), summaries=False, maps=False)       # (two assembly_summary.txt would clash)
    out = tmp_path / "G2"
    r = _run("taxid", os.path.join(work, "genomes"), *MAPPINGS, "-outdir", out, ID_OPT[id_type])
    assert r.returncode == 0, r.stderr
    m = mapping(id_type)
    parents = {}
    files = [f for f in ti.genome_files(work) if f.endswith(".fna")]
    assert sorted(os.listdir(out)) == sorted(os.path.basename(f) for f in files) and len(files) == 3
    for f in files:
        text = open(os.path.join(work, f), "rb").read()
        got = (out / os.path.basename(f)).read_bytes()
        assert got == ar.annotate(text, m, id_type), f
        for old, new in zip(text.split(b"\n"), got.split(b"\n")):
            if new[:1] == b">":
                parents[old[1:]] = host.target_parent_taxid(new[1:])
    assert len(parents) == 10
    if id_type == ar.ACCVER:
        assert parents[b"NC_000006.1 synthetic"] == 202 and parents[b"NC_000001.1 synthetic"] == 777 and parents[b"NC_000003.1 synthetic"] == 102
        assert parents[b"NC_000010.1 synthetic"] == 0 and parents[b"NC_000009.1 synthetic"] == 0 and parents[b"gi|5550008|synthetic"] == 0
    else:
        assert parents[b"gi|5550008|synthetic"] == 301 and parents[b"NC_000006.1 synthetic"] == 0
        assert sorted(parents.values()) == [0] * 9 + [301]                   # (the old taxid|201 is cut from a header without an id too)


def test_a_basename_clash_aborts_with_nothing_written(tmp_path):
    for d in ("x", "y"):
        os.makedirs(tmp_path / "g" / d)
        (tmp_path / "g" / d / "same.fa").write_bytes(b">NC_000006.1 %s\nACGT\n" % d.encode())
    r = _run("taxid", tmp_path / "g", *MAPPINGS, "-outdir", tmp_path / "out")
    assert r.returncode != 0 and b"ABORT:" in r.stderr and b"same.fa" in r.stderr
    assert not (tmp_path / "out").exists()


def test_a_header_longer_than_the_buffer_aborts_before_the_output_is_opened(tmp_path):
    (tmp_path / "long.fa").write_bytes(b">NC_000006.1 " + b"x" * 200 + b"\nACGT\n")
    (tmp_path / "seq.fa").write_bytes(b">NC_000006.1 x\n" + b"ACGT" * 100 + b"\n")               # a sequence line of any length passes
    r = _run("taxid", tmp_path / "long.fa", *MAPPINGS, "-out", tmp_path / "o", "-io-bytes", "64")
    assert r.returncode != 0 and b"ABORT:" in r.stderr and not (tmp_path / "o").exists()
    r = _run("taxid", tmp_path / "seq.fa", *MAPPINGS, "-out", tmp_path / "o", "-io-bytes", "64")
    assert r.returncode == 0 and (tmp_path / "o").read_bytes() == b">NC_000006.1 taxid|202 x\n" + b"ACGT" * 100


def test_help_and_rejections(tmp_path):
    r = _run("-help")
    text = r.stdout.decode()
    for opt in ("-out ", "-outdir", "-field-sep", "-field-separator", "-value-sep", "-value-separator", "-id=accver", "-id=acc", "-id=gi",
                "-mapper", "-map-chunk", "-io-bytes", "-device", "-timing", "-help", "mcq_build_cli"):
        assert opt in text, opt
    for args in (["taxid"], ["taxid", "x.fa"], ["names", "x.fa", MAPPINGS[0]], ["taxid", "x.fa", MAPPINGS[0], "-nosuch"],
                 ["taxid", "x.fa", MAPPINGS[0], "-mapper", "cpu"], ["taxid", "x.fa", MAPPINGS[0], "-out", "o", "stray"],
                 ["taxid", "x.fa", MAPPINGS[0], "-map-chunk", "8"], ["taxid", "x.fa", MAPPINGS[0], "-out", "a", "-outdir", "b"]):
        r = _run(*args, cwd=tmp_path)
        assert r.returncode != 0 and b"ABORT:" in r.stderr, args
    r = _run("taxid", tmp_path / "nosuch.fa", MAPPINGS[0], "-out", tmp_path / "o")
    assert r.returncode != 0 and b"could not be opened" in r.stderr and not (tmp_path / "o").exists()
