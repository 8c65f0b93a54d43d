#!/usr/bin/env python3
"""Generate tests/golden/accmap/ by RUNNING the reference (build container only: needs /root/reference and oracle/_ref).

The genomes of the `mini` fixture (tests/golden/mini/genomes.fa.gz: the same ten sequences, so the same features) with the
taxid|N cut from their headers, in two genome directories, and mapping files that put every way the reference has of finding a
sequence's taxon in front of it (src/taxonomy_io.cpp:190-310, src/mode_build.cpp:248-312, :493-604):

  target  name          where its taxon comes from
  0, 1    NC_000001.1,  genomes/a/assembly_summary.txt (two '#' lines, the second is the header row), keyed by the GCF_ accession
          NC_000002.1   of the FILE name GCF_000001.1_a.fna                                                            -> 101
  2       NC_000003.1   the same file, GCF_000002.1_b.fna                                                              -> 102
  3       NC_000004.1   genomes/b/assembly_summary.txt in the two-column form, keyed by the sequence id                -> 201
  4       NC_000005.1 taxid   its header keeps taxid|201 (the name ends at the '|', as in the mini fixture)            -> 201
  5       NC_000006.1   nucl_gb: a line names it by accver (202); a later line and one in nucl_wgs name it with other taxids
                        (ignored); BEFORE them a line whose accver names the ranked target 0 while its acc would name this
                        one (taxid 777: a parser that falls through gets it wrong)                                     -> 202
  6       NC_000007.1   nucl_wgs: only through acc (accver names version .2; taxon_with_similar_name)                  -> 202
  7       5550008       (header gi|5550008|...) extra.accession2taxid: only through gi                                 -> 301
  8       NC_000009.1   nucl_gb: its first line has taxid 0, a later one 301 (ignored): the parent stays 0             -> unranked
  9       NC_000010.1   named by no line                                                                               -> unranked
nucl_wgs also names targets 0-2 (ranked before the files are read: nothing happens; a database built without the
assembly summaries finds them there).  About 130 lines per file, the others name nothing.

Committed: the inputs and the reference's accmap.db_0 / accmap.db_1 (`mpiexec -n 2 metacache_mpi build accmap genomes -taxonomy tax`).
"""
import gzip
import os
import random
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg     # noqa: E402  (sh, ensure_mpilib, ref_build)

OUT = os.path.join(HERE, "accmap")
HEADERS = ["NC_000001.1 synthetic", "NC_000002.1 synthetic", "NC_000003.1 synthetic", "NC_000004.1 synthetic",
           "NC_000005.1 taxid|201 synthetic", "NC_000006.1 synthetic", "NC_000007.1 synthetic", "gi|5550008|synthetic",
           "NC_000009.1 synthetic", "NC_000010.1 synthetic"]
FILES = [("genomes/a/GCF_000001.1_a.fna", [0, 1]), ("genomes/a/GCF_000002.1_b.fna", [2]), ("genomes/b/part.fna", [3, 4, 5, 6, 7, 8, 9])]


def mini_sequences():
    seqs = []
    with gzip.open(os.path.join(HERE, "mini", "genomes.fa.gz"), "rt") as f:
        for line in f:
            if not line.startswith(">"):
                seqs.append(line.strip())
    assert len(seqs) == 10
    return seqs


def decoys(rng, n, tag):
    """lines that name nothing: no target name is greater than such an acc and begins with it, no target is named by the gi"""
    out = []
    for _ in range(n):
        a = "%s%06d" % (tag, rng.randrange(10 ** 6))
        out.append("%s\t%s.%d\t%d\t%d\n" % (a, a, rng.randint(1, 3), rng.randint(2, 9999), rng.randrange(10 ** 7, 10 ** 8)))
    return out


def mapping_file(rng, lines_at, n, tag):
    """header line + n decoys with the given lines put in at the given positions (ascending)"""
    body = decoys(rng, n, tag)
    for at, line in sorted(lines_at, reverse=True):
        body.insert(at, line)
    return "accession\taccession.version\ttaxid\tgi\n" + "".join(body)


def write_inputs(root):
    rng = random.Random(20261020)
    seqs = mini_sequences()
    for name, targets in FILES:
        os.makedirs(os.path.dirname(os.path.join(root, name)), exist_ok=True)
        with open(os.path.join(root, name), "w") as f:
            for t in targets:
                f.write(">%s\n" % HEADERS[t])
                for i in range(0, len(seqs[t]), 80):
                    f.write(seqs[t][i:i + 80] + "\n")
    with open(os.path.join(root, "genomes/a/assembly_summary.txt"), "w") as f:
        f.write("#   See the README of the genomes directory for a description of the columns in this file.\n")
        f.write("# assembly_accession\tbioproject\tbiosample\twgs_master\trefseq_category\ttaxid\tspecies_taxid\torganism_name\n")
        f.write("GCF_000001.1\tPRJNA1\tSAMN01\t\trepresentative genome\t101\t101\tGenA one\n")
        f.write("GCF_000002.1\tPRJNA2\tSAMN02\t\tna\t102\t102\tGenA two\n")
        f.write("GCF_000001.1\tPRJNA3\tSAMN03\t\tna\t999\t999\ta second entry of a key is not entered\n")
    with open(os.path.join(root, "genomes/b/assembly_summary.txt"), "w") as f:
        f.write("NC_000004.1\t201\nNC_000004.1\t998\nXY_000001.1\t5\n")
    os.makedirs(os.path.join(root, "tax"))
    for n in ("nodes.dmp", "names.dmp"):
        shutil.copy(os.path.join(HERE, "mini", n), os.path.join(root, "tax", n))
    gb = mapping_file(rng, [(10, "NC_000006\tNC_000001.1\t777\t11\n"),        # accver: ranked target 0; acc would name target 5
                            (30, "NC_000006\tNC_000006.1\t202\t12\n"),
                            (31, "NC_000009\tNC_000009.1\t0\t13\n"),
                            (90, "NC_000006\tNC_000006.1\t999\t14\n"),
                            (100, "NC_000009\tNC_000009.1\t301\t15\n")], 125, "AB")
    wgs = mapping_file(rng, [(5, "NC_000006\tNC_000006.1\t998\t21\n"),
                             (40, "NC_000007\tNC_000007.2\t202\t22\n"),
                             (41, "NC_000001\tNC_000001.1\t101\t23\n"),
                             (42, "NC_000002\tNC_000002.1\t101\t24\n"),
                             (43, "NC_000003\tNC_000003.1\t102\t25\n")], 125, "AC")
    extra = mapping_file(rng, [(60, "QX000001\tQX000001.1\t301\t5550008\n")], 130, "QX9")
    for n, text in (("nucl_gb", gb), ("nucl_wgs", wgs), ("extra", extra)):
        with open(os.path.join(root, "tax", n + ".accession2taxid"), "w") as f:
            f.write(text)


def main():
    if not os.path.isdir("/root/reference"):
        sys.exit("needs /root/reference (build container only)")
    mg.ensure_mpilib()
    shutil.rmtree(OUT, ignore_errors=True)
    work = tempfile.mkdtemp(prefix="golden_accmap_")
    write_inputs(work)
    mg.ref_build(work, "accmap", 2)
    os.makedirs(os.path.join(OUT, "P2"))
    for r in range(2):
        shutil.copy(os.path.join(work, "accmap.db_%d" % r), os.path.join(OUT, "P2"))
    for d, _, names in os.walk(work):
        for n in names:
            if n.startswith("accmap.db_"):
                continue
            src = os.path.join(d, n)
            dst = os.path.join(OUT, os.path.relpath(src, work))
            os.makedirs(os.path.dirname(dst), exist_ok=True)
            if n.endswith(".fna"):              # the genome files are stored gzipped (tests/taxmap_inputs.py unpacks them)
                with open(src, "rb") as fi, gzip.GzipFile(dst + ".gz", "wb", mtime=0) as fo:
                    fo.write(fi.read())
            else:
                shutil.copy(src, dst)
    shutil.rmtree(work, ignore_errors=True)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
