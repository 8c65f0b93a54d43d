#!/usr/bin/env python3
"""Generate tests/golden/annotate/ by RUNNING the reference's annotate mode (build container only: needs /root/reference and
oracle/_ref/metacache_mpi, built by `make -C oracle ref`): `metacache_mpi annotate taxid INFILE MAPPING... -out FILE [options]`, a
singleton without mpiexec, as make_golden_info.py runs `info`.

The mapping files are the three of tests/golden/accmap/tax/ (nucl_gb, nucl_wgs, extra .accession2taxid), used where they lie, in
this order (the first line that names an id wins).  What they give, per column:
  accver  NC_000001.1 -> 777 (nucl_gb names it before nucl_wgs does with 101), NC_000006.1 -> 202 (999 and 998 come later),
          NC_000009.1 -> 0 (301 comes later), NC_000007.2 -> 202, NC_000002.1 -> 101, NC_000003.1 -> 102, QX000001.1 -> 301
  acc     NC_000006 -> 777, NC_000009 -> 0, NC_000007 -> 202, NC_000001 -> 101, NC_000002 -> 101, NC_000003 -> 102
  gi      5550008 -> 301 (and 11 .. 15, 21 .. 25, which no header holds)

Inputs (all new, a few KB, stored gzipped so that no checkout touches the CR of in.fa):
  in.fa     the ten headers of make_golden_taxmap.py -- `NC_000005.1 taxid|201 synthetic` (an old taxid in the middle) and
            `gi|5550008|synthetic` (no blank: the taxid is appended; under -id=gi the only header that is named) among them -- and
              >NC_000002.1                       no field separator
              >NC_000003.1 again taxid|55        the old taxid is the last field: the cut runs to the end of the line
              >seq7.1 plasmid                    no known prefix but a '.': under accver the id is `>seq7.1`, which no line names
                                                 (taxid|0 is put in); under acc and gi there is no id and nothing is put in
              >NZ_999999.1 unknown               an id no line names
              >NC_000006.1 crlf\\r\\n              CR LF (the CR stays in the line; the sequence lines of this record have it too)
              >NC_000007.2_x taxid:9_y z         for -field-sep _ -value-sep : (under the default separators nothing is cut: no '|')
  gap.fa    two records, an empty line, two more records: the output ends at the empty line
  reads.fq  four records; the quality line of the second begins with '@' and holds a '.' (a header for annotate: taxid|0 goes into
            it under accver), that of the fourth begins with '@' and holds none (a header without an id: unchanged)

Recorded (the file the reference wrote with -out):
  in.accver.fa, in.acc.fa, in.gi.fa     the three id types, default separators
  in.sep.fa                             -field-sep _ -value-sep :   (accver)
  gap.accver.fa, reads.accver.fq

The reference counts its non-prefixed arguments in one list and indexes the list of ALL arguments with that count
(mapping_filenames, src/mode_annotate.cpp:87-116), so an option in front of the mapping files would cut them short; with every
option behind them it reads the files the run names.  The maker asserts that from its "Processing mappings in file" lines.

usage: python tests/golden/make_golden_annotate.py
"""
import gzip
import os
import random
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, ensure_mpilib, sh     # noqa: E402
from make_golden_taxmap import HEADERS              # noqa: E402

OUT = os.path.join(HERE, "annotate")
TAX = os.path.join(HERE, "accmap", "tax")
MAPPINGS = [os.path.join(TAX, n + ".accession2taxid") for n in ("nucl_gb", "nucl_wgs", "extra")]
MORE = ["NC_000002.1", "NC_000003.1 again taxid|55", "seq7.1 plasmid", "NZ_999999.1 unknown", "NC_000006.1 crlf\r", "NC_000007.2_x taxid:9_y z"]
RUNS = [("in.fa", "in.accver.fa", ["-id=accver"]), ("in.fa", "in.acc.fa", ["-id=acc"]), ("in.fa", "in.gi.fa", ["-id=gi"]),
        ("in.fa", "in.sep.fa", ["-field-sep", "_", "-value-sep", ":"]), ("gap.fa", "gap.accver.fa", []), ("reads.fq", "reads.accver.fq", [])]


def seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def write_inputs(root):
    rng = random.Random(20261021)
    with open(os.path.join(root, "in.fa"), "w", newline="") as f:
        for h in HEADERS + MORE:
            eol = "\r\n" if h.endswith("\r") else "\n"
            f.write(">" + h.rstrip("\r") + eol)
            for _ in range(2):
                f.write(seq(rng, 60) + eol)
    with open(os.path.join(root, "gap.fa"), "w", newline="") as f:
        f.write(">NC_000006.1 before the gap\n%s\n>NC_000001.1 too\n%s\n\n>NC_000002.1 behind the gap\n%s\n>NC_000003.1 too\n%s\n"
                % tuple(seq(rng, 50) for _ in range(4)))
    with open(os.path.join(root, "reads.fq"), "w", newline="") as f:
        quals = ["I" * 40, "@II.I" + "I" * 35, "#" * 40, "@" + "F" * 39]
        for i, (h, q) in enumerate(zip(["NC_000006.1 read1", "NC_000007.2 read2/1", "gi|5550008|read3", "NZ_999999.1 read4"], quals)):
            f.write("@%s\n%s\n+\n%s\n" % (h, seq(rng, 40), q))


def store(src, name):
    with open(src, "rb") as fi, gzip.GzipFile(os.path.join(OUT, name + ".gz"), "wb", mtime=0) as fo:
        fo.write(fi.read())


def main():
    if not os.path.isdir("/root/reference"):
        sys.exit("needs /root/reference (build container only)")
    ensure_mpilib()
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    work = tempfile.mkdtemp(prefix="golden_annotate_")
    write_inputs(work)
    for name in ("in.fa", "gap.fa", "reads.fq"):
        store(os.path.join(work, name), name)
    for infile, outfile, opts in RUNS:
        txt = sh([os.path.join(REF, "metacache_mpi"), "annotate", "taxid", infile] + MAPPINGS + ["-out", outfile] + opts, cwd=work)
        read = [l[len("Processing mappings in file '"):-1] for l in txt.splitlines() if l.startswith("Processing mappings in file '")]
        assert read == MAPPINGS, (read, MAPPINGS)
        assert "Mapping ... complete." in txt, txt
        store(os.path.join(work, outfile), outfile)
    shutil.rmtree(work, ignore_errors=True)
    print("wrote %d files under %s" % (len(os.listdir(OUT)), OUT))


if __name__ == "__main__":
    main()
