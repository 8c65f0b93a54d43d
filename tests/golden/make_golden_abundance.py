#!/usr/bin/env python3
"""Generate the abundance fixtures under tests/golden/ by RUNNING the reference.

Runs only in the build container (needs /root/reference and oracle/_ref/metacache_mpi, built by
`make -C oracle ref`).  Queries the committed shard files of `mini` (P = 4) and `tie` (P = 2) with the reads
of their queries.json, the options of make_golden.py's make_cliout (-threads 2 -query-limit 128 -maxcand
-hitmin 4 -hitdiff 80) plus the abundance options, and keeps the reference's whole -out file:

  <tag>/P<p>/cli_abund_species.out.gz     -abundance-per species            (the scripted command line)
  <tag>/P<p>/cli_abund_both_genus.out.gz  -abundances -abundance-per genus  (plain table + estimate)
  <tag>/P<p>/cli_abund_seq.out.gz         -abundance-per sequence           (estimation without pruning)
  <tag>/P<p>/cli_abund_file.out.gz        -abundances ab.txt -abundance-per species
  <tag>/P<p>/cli_abund_file.ab.txt.gz       ... and the file the tables went to
  <tag>/P<p>/cli_abund_nomap.out.gz       -nomap -abundance-per species

usage: python tests/golden/make_golden_abundance.py
"""
import gzip
import json
import os
import shutil
import sys
import tempfile

from make_golden import HERE, REF, ensure_mpilib, sh, write_fastq

VARIANTS = {
    "species": ["-abundance-per", "species"],
    "both_genus": ["-abundances", "-abundance-per", "genus"],
    "seq": ["-abundance-per", "sequence"],
    "file": ["-abundances", "ab.txt", "-abundance-per", "species"],
    "nomap": ["-nomap", "-abundance-per", "species"],
}


def gz(src, dst):
    with open(src, "rb") as fi, gzip.GzipFile(dst, "wb", mtime=0) as fo:
        fo.write(fi.read())


def main():
    for tag, P in (("mini", 4), ("tie", 2)):
        d = os.path.join(HERE, tag, "P%d" % P)
        with open(os.path.join(HERE, tag, "queries.json")) as f:
            q = json.load(f)
        work = tempfile.mkdtemp(prefix="golden_abund_" + tag + "_")
        for r in range(P):
            shutil.copy(os.path.join(d, "%s.db_%d" % (tag, r)), work)
        write_fastq(os.path.join(work, "r1.fq"), q["names"], q["r1"])
        write_fastq(os.path.join(work, "r2.fq"), q["names"], q["r2"])
        for name, extra in VARIANTS.items():
            out = os.path.join(work, "out_%s.txt" % name)
            ab = os.path.join(work, "ab.txt")
            if os.path.exists(ab):
                os.remove(ab)
            sh(["/opt/conda/bin/mpiexec", "-n", str(P), os.path.join(REF, "metacache_mpi"),
                "query", tag, "r1.fq", "r2.fq", "-pairfiles", "-lowest", q["lowest"], "-threads", "2",
                "-maxcand", str(q["maxcand"]), "-hitmin", "4", "-hitdiff", "80", "-query-limit", "128", "-out", out] + extra,
               cwd=work)
            gz(out, os.path.join(d, "cli_abund_%s.out.gz" % name))
            print("%s P=%d cli_abund_%s: %d lines" % (tag, P, name, sum(1 for _ in open(out))))
            if name == "file":
                gz(ab, os.path.join(d, "cli_abund_file.ab.txt.gz"))
                print("%s P=%d cli_abund_file.ab.txt: %d lines" % (tag, P, sum(1 for _ in open(ab))))
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    if not os.path.isdir("/root/reference"):
        sys.exit("needs /root/reference (build container only)")
    ensure_mpilib()
    main()
