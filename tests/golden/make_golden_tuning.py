#!/usr/bin/env python3
"""Generate the database-query-option fixtures under tests/golden/ by RUNNING the reference.

Runs only in the build container (needs /root/reference and oracle/_ref/metacache_mpi, built by
`make -C oracle ref`).  Queries the committed shard files with the reads of queries.json, with the options of
make_golden.py's make_cliout (-threads 2 -query-limit 128 -maxcand -hitmin 4 -hitdiff 80), `-tophits -lowest sequence` (so
that a lost location shows) and the database query options of get_database_query_options (src/query_options.cpp:41-66),
and keeps the reference's whole -out file as <set>/P<n>/cli_tune_<name>.out.gz:

  overpop P2 maxlocs40        -max-locations-per-feature 40            both shard files hold buckets of up to 100 locations
  overpop P4 remove40         -remove-overpopulated-features -max-locations-per-feature 40     ranks 2 and 3 hold the long buckets
                              (this run alone with -lowest species: under -lowest sequence the MPI program drops every
                              sequence-level candidate a rank other than 0 sends, src/querying.h:958, :983-985, so nothing of
                              ranks 2 and 3 ever reaches the output and no N makes the run differ)
  overpop P2 remove1          -remove-overpopulated-features -max-locations-per-feature 1      the quirk: nothing removed, every bucket cut to 1
  overpop P2 maxlocs1         -max-locations-per-feature 1             ignored: must EQUAL the run without it
  mini    P2 maxlocs2         -max-locations-per-feature 2             rank 0 has buckets of 3, rank 1 of up to 15 (N = 4 and 3 were
                              tried first: no line differs, what rank 1 sends is dropped under -lowest sequence as above)
  mini    P4 win64_sketch8    -winlen 64 -sketchlen 8
  mini    P2 win100_stride50  -winlen 100 -winstride 50
  mini    P4 stride32         -winstride 32

A run stops here if no mapping line differs from the same run without the tuning options (maxlocs1: if one does): a fixture
that equals the untuned output would let a test pass on code that skips the options.  If a run does not differ, raise or
lower N, or change the window, until it does, and write the chosen values into RUNS.

usage: python tests/golden/make_golden_tuning.py
"""
import gzip
import json
import os
import shutil
import sys
import tempfile

from make_golden import HERE, REF, ensure_mpilib, sh, write_fastq

MAXLOCS = ["-max-locations-per-feature"]
REMOVE = ["-remove-overpopulated-features"]
# (set, P, name, -lowest, options, must differ from the untuned run); tests/test_gpu_cli_tuning.py holds the same table
RUNS = [("overpop", 2, "maxlocs40", "sequence", MAXLOCS + ["40"], True),
        ("overpop", 4, "remove40", "species", REMOVE + MAXLOCS + ["40"], True),
        ("overpop", 2, "remove1", "sequence", REMOVE + MAXLOCS + ["1"], True),
        ("overpop", 2, "maxlocs1", "sequence", MAXLOCS + ["1"], False),
        ("mini", 2, "maxlocs2", "sequence", MAXLOCS + ["2"], True),
        ("mini", 4, "win64_sketch8", "sequence", ["-winlen", "64", "-sketchlen", "8"], True),
        ("mini", 2, "win100_stride50", "sequence", ["-winlen", "100", "-winstride", "50"], True),
        ("mini", 4, "stride32", "sequence", ["-winstride", "32"], True)]


def gz(src, dst):
    with open(src, "rb") as fi, gzip.GzipFile(dst, "wb", mtime=0) as fo:
        fo.write(fi.read())


def mapping_lines(path):
    return [l for l in open(path).read().split("\n") if l and not l.startswith("#")]


def by_header(lines):
    return {l.split("\t|\t")[0]: l for l in lines}


def main():
    for tag, P, name, lowest, extra, must_differ in RUNS:
        d = os.path.join(HERE, tag, "P%d" % P)
        with open(os.path.join(HERE, tag, "queries.json")) as f:
            q = json.load(f)
        work = tempfile.mkdtemp(prefix="golden_tune_" + tag + "_")
        for r in range(P):
            shutil.copy(os.path.join(d, "%s.db_%d" % (tag, r)), work)
        write_fastq(os.path.join(work, "r1.fq"), q["names"], q["r1"])
        write_fastq(os.path.join(work, "r2.fq"), q["names"], q["r2"])
        base = ["/opt/conda/bin/mpiexec", "-n", str(P), os.path.join(REF, "metacache_mpi"),
                "query", tag, "r1.fq", "r2.fq", "-pairfiles", "-lowest", lowest, "-tophits", "-threads", "2",
                "-maxcand", str(q["maxcand"]), "-hitmin", "4", "-hitdiff", "80", "-query-limit", "128"]
        out, plain = os.path.join(work, "out.txt"), os.path.join(work, "plain.txt")
        sh(base + ["-out", out] + extra, cwd=work)
        sh(base + ["-out", plain], cwd=work)
        a, b = by_header(mapping_lines(out)), by_header(mapping_lines(plain))
        differ = sum(1 for h in a if a[h] != b.get(h))
        print("%s P=%d cli_tune_%s: %d mapping lines, %d differ from the run without %s" % (tag, P, name, len(a), differ, " ".join(extra)))
        if set(a) != set(b):
            sys.exit("%s %s: the two runs name different reads" % (tag, name))
        if must_differ and differ == 0:
            sys.exit("%s %s: no mapping line differs from the untuned run: choose other values for this run" % (tag, name))
        if not must_differ and differ != 0:
            sys.exit("%s %s: this run must equal the untuned one, %d lines differ" % (tag, name, differ))
        gz(out, os.path.join(d, "cli_tune_%s.out.gz" % name))
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    if not os.path.isdir("/root/reference"):
        sys.exit("needs /root/reference (build container only)")
    ensure_mpilib()
    main()
