#!/usr/bin/env python3
"""Generate tests/golden/merge/ by RUNNING the reference's merge mode.

Runs only in the build container (needs /root/reference and oracle/_ref/metacache_mpi, built by `make -C oracle ref`).
The genomes of `mini` are split into three disjoint thirds (record i goes to database i % 3); each third becomes a
database (`mpiexec -n 2 metacache_mpi build`), each database is queried with the reads of mini/queries.json
(-pairfiles -tophits -queryids -lowest species -maxcand 4 -hitmin 4 -threads 2; -query-limit 128 as in make_golden.py: the
MPI program sizes a table by it), and the three result files are merged
(`mpiexec -n 1 metacache_mpi merge res_0.txt res_1.txt res_2.txt -taxonomy tax -hitmin 4 ...`) under four option sets.

Committed, gzip'd: the three result files res_<k>.txt.gz and the reference's merged -out files

  merged_tophits.out.gz      -maxcand 4 -tophits -queryids
  merged_lineage.out.gz      -maxcand 4 -taxids -lineage
  merged_abundance.out.gz    -maxcand 4 -abundance-per species -mapped-only
  merged_genus.out.gz        -maxcand 2 -highest genus

The reads of `mini` alone do not pin a merge: each comes from one genome, the database that holds it gives its species with the
most hits, and the merge repeats that (4 of 197 merged classifications differ from every single input's).  So 96 pairs are added
behind them (x0000 .. x0095, seeded): mate 1 from a genome of one database, mate 2 from a genome of another species in another
database.  Every database classifies such a pair by the mate it knows; only the merge sees both.  The reads written are
committed as reads.json.

A run fails here if fewer than one tenth of the merged classifications differ from every single input's: a merge that
changes nothing pins nothing.

usage: python tests/golden/make_golden_merge.py
"""
import gzip
import json
import os
import random
import shutil
import sys
import tempfile

from make_golden import HERE, REF, ensure_mpilib, sh, write_fastq

OUT = os.path.join(HERE, "merge")
MINI = os.path.join(HERE, "mini")
SETS = [("tophits", ["-maxcand", "4", "-tophits", "-queryids"]),
        ("lineage", ["-maxcand", "4", "-taxids", "-lineage"]),
        ("abundance", ["-maxcand", "4", "-abundance-per", "species", "-mapped-only"]),
        ("genus", ["-maxcand", "2", "-highest", "genus"])]


def gz(src, dst):
    with open(src, "rb") as fi, gzip.GzipFile(dst, "wb", mtime=0) as fo:
        fo.write(fi.read())


def fasta_records(path):
    recs = []
    for line in gzip.open(path, "rt"):
        if line.startswith(">"):
            recs.append([line])
        else:
            recs[-1].append(line)
    return ["".join(r) for r in recs]


CROSS = [(0, 4), (3, 7), (6, 1), (9, 5), (2, 3), (8, 0), (5, 1), (7, 2)]      # (genome of mate 1, genome of mate 2): two databases, two species


def cross_pairs(recs, n=96, length=120):
    rng = random.Random(20)
    seqs = ["".join(r.split("\n")[1:]) for r in recs]
    names, r1, r2 = [], [], []
    for j in range(n):
        a, b = CROSS[j % len(CROSS)]
        pa, pb = rng.randrange(len(seqs[a]) - length), rng.randrange(len(seqs[b]) - length)
        names.append("x%04d" % j)
        r1.append(seqs[a][pa:pa + length])
        r2.append(seqs[b][pb:pb + length])
    return names, r1, r2


def classifications(path):
    """last column of every mapping line, by the line's first column"""
    out = {}
    for l in open(path).read().split("\n"):
        if l and not l.startswith("#"):
            cols = l.split("\t|\t")
            out[cols[0]] = cols[-1]
    return out


def main():
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(MINI, "queries.json")) as f:
        q = json.load(f)
    recs = fasta_records(os.path.join(MINI, "genomes.fa.gz"))
    work = tempfile.mkdtemp(prefix="golden_merge_")
    os.makedirs(os.path.join(work, "tax"))
    for n in ("nodes.dmp", "names.dmp"):
        shutil.copy(os.path.join(MINI, n), os.path.join(work, "tax"))
    xn, x1, x2 = cross_pairs(recs)
    reads = {"names": q["names"] + xn, "r1": q["r1"] + x1, "r2": q["r2"] + x2}
    with open(os.path.join(OUT, "reads.json"), "w") as f:
        json.dump(reads, f, indent=0)
    write_fastq(os.path.join(work, "r1.fq"), reads["names"], reads["r1"])
    write_fastq(os.path.join(work, "r2.fq"), reads["names"], reads["r2"])
    mpiexec, prog = "/opt/conda/bin/mpiexec", os.path.join(REF, "metacache_mpi")
    res = []
    for k in range(3):
        g = os.path.join(work, "genomes_%d" % k)
        os.makedirs(g)
        with open(os.path.join(g, "part.fa"), "w") as f:
            f.write("".join(recs[k::3]))
        sh([mpiexec, "-n", "2", prog, "build", "db%d" % k, "genomes_%d" % k, "-taxonomy", "tax"], cwd=work)
        res.append("res_%d.txt" % k)
        sh([mpiexec, "-n", "2", prog, "query", "db%d" % k, "r1.fq", "r2.fq", "-pairfiles", "-tophits", "-queryids", "-lowest", "species",
            "-maxcand", "4", "-hitmin", "4", "-threads", "2", "-query-limit", "128", "-out", res[-1]], cwd=work)
    singles = [classifications(os.path.join(work, r)) for r in res]
    for name, opts in SETS:
        out = "merged_%s.out" % name
        sh([mpiexec, "-n", "1", prog, "merge"] + res + ["-taxonomy", "tax", "-hitmin", "4", "-lowest", "species"] + opts + ["-out", out], cwd=work)
        if name == "tophits":
            merged = classifications(os.path.join(work, out))
            differ = sum(1 for h in merged if all(merged[h] != s.get(h) for s in singles))
            print("%d reads, %d merged classifications differ from every single input's" % (len(merged), differ))
            if differ * 10 < len(merged):
                sys.exit("the merge changes fewer than one tenth of the classifications: split the genomes another way")
        gz(os.path.join(work, out), os.path.join(OUT, out + ".gz"))
    for r in res:
        gz(os.path.join(work, r), os.path.join(OUT, r + ".gz"))
    shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    if not os.path.isdir("/root/reference"):
        sys.exit("needs /root/reference (build container only)")
    ensure_mpilib()
    main()
