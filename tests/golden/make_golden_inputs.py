#!/usr/bin/env python3
"""Generate the input-list fixtures under tests/golden/ by RUNNING the reference.

Runs only in the build container (needs /root/reference and oracle/_ref/metacache_mpi, built by
`make -C oracle ref`).  Queries the committed shard files of `mini` (P = 4) and `tie` (P = 2) with the reads of
their queries.json split into three pairs of files -- reads [0, n/3) as c_1.fq / c_2.fq, the next third as a_*, the
last as b_* -- named on the command line in a seeded shuffled order, under -pairfiles and the options of
make_golden_abundance.py's `species` variant, and keeps the reference's whole -out file:

  <tag>/P<p>/cli_inputs_three_pairs.out.gz

Under mpiexec every rank of the reference opens the -out file and writes its own parameter lines and "# f1 + f2" lines
into it (src/mode_query.cpp:73-123, src/querying.h:1336-1340), at its own offsets.  With one pair of files those bytes
are the ones rank 0 writes there; with several pairs the unit lines of ranks >= 1 land on rank 0's mapping lines, and which
survive depends on who flushes last.  A file is kept only if it is whole -- every unit line once, in sorted order, every
read's mapping line once behind its unit's line; otherwise this script says what it found and keeps nothing for that
fixture (2026-10: `tie` P = 2 whole; `mini` P = 4 not: 178 of 180 mapping lines, unit lines doubled).

(No file for -pairseq: the reference's MPI query crashes in sequence_pair_reader::close without a second reader.)

usage: python tests/golden/make_golden_inputs.py
"""
import json
import os
import random
import shutil
import sys
import tempfile

from make_golden import HERE, REF, ensure_mpilib, sh, write_fastq
from make_golden_abundance import gz

GROUPS = ("c", "a", "b")
SEED = 20261017


def not_whole(lines, names, n):
    """None if the file has the three unit lines in sorted order, each followed by the mapping lines of exactly its reads"""
    at = next(i for i, l in enumerate(lines) if l.startswith("# TABLE_LAYOUT"))
    end = next((i for i, l in enumerate(lines) if l.startswith("# estimated abundance")), len(lines))
    units = []
    for l in lines[at + 1:end]:
        if l.startswith("# "):
            units.append((l, []))
        elif not units:
            return "a mapping line in front of the first unit line"
        else:
            units[-1][1].append(l.split("\t|\t")[0])
    if [u for u, _ in units] != ["# %s_1.fq + %s_2.fq" % (g, g) for g in sorted(GROUPS)]:
        return "unit lines %r" % [u for u, _ in units]
    for g, (_, got) in zip(sorted(GROUPS), units):
        i = GROUPS.index(g)
        if sorted(got) != sorted(names[n * i // 3: n * (i + 1) // 3]):
            return "unit %s holds %d mapping lines of %d reads" % (g, len(got), n * (i + 1) // 3 - n * i // 3)
    return None


def main():
    for tag, P in (("mini", 4), ("tie", 2)):
        d = os.path.join(HERE, tag, "P%d" % P)
        with open(os.path.join(HERE, tag, "queries.json")) as f:
            q = json.load(f)
        work = tempfile.mkdtemp(prefix="golden_inputs_" + tag + "_")
        for r in range(P):
            shutil.copy(os.path.join(d, "%s.db_%d" % (tag, r)), work)
        n, files = len(q["names"]), []
        for i, g in enumerate(GROUPS):
            part = slice(n * i // 3, n * (i + 1) // 3)
            for m, key in (("1", "r1"), ("2", "r2")):
                files.append("%s_%s.fq" % (g, m))
                write_fastq(os.path.join(work, files[-1]), q["names"][part], q[key][part])
        random.Random(SEED).shuffle(files)
        out = os.path.join(work, "out.txt")
        sh(["/opt/conda/bin/mpiexec", "-n", str(P), os.path.join(REF, "metacache_mpi"), "query", tag] + files +
           ["-pairfiles", "-lowest", q["lowest"], "-threads", "2", "-maxcand", str(q["maxcand"]), "-hitmin", "4", "-hitdiff", "80",
            "-query-limit", "128", "-abundance-per", "species", "-out", out], cwd=work)
        problem = not_whole(open(out).read().split("\n"), q["names"], n)
        if problem:
            print("%s P=%d cli_inputs_three_pairs: NOT KEPT, the ranks' writes collided: %s" % (tag, P, problem))
        else:
            gz(out, os.path.join(d, "cli_inputs_three_pairs.out.gz"))
            print("%s P=%d cli_inputs_three_pairs (%s): %d lines" % (tag, P, " ".join(files), sum(1 for _ in open(out))))
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    if not os.path.isdir("/root/reference"):
        sys.exit("needs /root/reference (build container only)")
    ensure_mpilib()
    main()
