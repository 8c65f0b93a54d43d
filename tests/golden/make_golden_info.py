#!/usr/bin/env python3
"""Generate tests/golden/info/ by RUNNING the reference's info mode on the shard files already under tests/golden/.

Runs only in the build container (needs /root/reference and oracle/_ref/metacache_mpi, built by `make -C oracle ref`).
The reference reads ONE shard file per run (`metacache_mpi info <db>.db_<r> <mode>`, a singleton without mpiexec); its stdout
is recorded, gzip'd (mtime 0, so a rerun gives the same bytes), its stderr ("Reading database from file ...") is not:

  info/<tag>/P<p>/db_<r>.statistics.txt.gz       mini P2/P4/P8, overpop P2/P4, noanc P2, tie P2: every shard
  info/<tag>/P2/db_<r>.bare.txt.gz               mini, noanc, accmap: shards 0 and 1 -- `info <db>` alone
  info/<tag>/P2/db_<r>.lineages.txt.gz
  info/<tag>/P2/db_<r>.rank_species.txt.gz, .rank_genus.txt.gz
  info/<tag>/P2/db_<r>.targets.txt.gz            every target
  info/<tag>/P2/db_<r>.targets_named.txt.gz      `targets NC_000003.1 nosuchname`
  info/mini/P2/db_<r>.featurecounts.txt.gz       static block, content block and the `feature -> size` lines in hash table order

usage: python tests/golden/make_golden_info.py
"""
import gzip
import os
import sys

from make_golden import HERE, REF, ensure_mpilib, sh

OUT = os.path.join(HERE, "info")
STATISTICS = [("mini", 2), ("mini", 4), ("mini", 8), ("overpop", 2), ("overpop", 4), ("noanc", 2), ("tie", 2)]
META = ["mini", "noanc", "accmap"]
MODES = [("bare", []), ("lineages", ["lineages"]), ("rank_species", ["rank", "species"]), ("rank_genus", ["rank", "genus"]),
         ("targets", ["targets"]), ("targets_named", ["targets", "NC_000003.1", "nosuchname"])]


def record(tag, P, r, name, args):
    d = os.path.join(OUT, tag, "P%d" % P)
    os.makedirs(d, exist_ok=True)
    txt = sh([os.path.join(REF, "metacache_mpi"), "info", "%s.db_%d" % (tag, r)] + args, cwd=os.path.join(HERE, tag, "P%d" % P))
    with gzip.GzipFile(os.path.join(d, "db_%d.%s.txt.gz" % (r, name)), "wb", mtime=0) as f:
        f.write(txt.encode())
    return txt


def main():
    n = 0
    for tag, P in STATISTICS:
        for r in range(P):
            record(tag, P, r, "statistics", ["statistics"]); n += 1
    for tag in META:
        for r in (0, 1):
            for name, args in MODES:
                record(tag, 2, r, name, args); n += 1
    for r in (0, 1):
        record("mini", 2, r, "featurecounts", ["featurecounts"]); n += 1
    print("%d files under %s" % (n, OUT))


if __name__ == "__main__":
    if not os.path.isdir("/root/reference"):
        sys.exit("needs /root/reference (build container only)")
    ensure_mpilib()
    main()
