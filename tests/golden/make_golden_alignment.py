#!/usr/bin/env python3
"""Generate the alignment fixtures under tests/golden/ by RUNNING the reference.

Runs only in the build container (needs /root/reference and oracle/_ref/metacache_mpi, built by `make -C oracle ref`).

  align/cases.json.gz            [[query, subject, score, aligned query, aligned subject], ...]: what the reference's
                                 align_semi_global with default_alignment_scheme (src/alignment.h) returns.  A small driver is
                                 written into a temporary directory and compiled there; it includes the reference's header where
                                 it lies.  Neither the driver nor anything of the reference is kept.  Every (query, subject) is
                                 recorded in both orientations of the query (reverse_complement, src/dna_encoding.h:146-165, is
                                 restated here: only ACGTacgt change).
  mini/P4/cli_align.out.gz       the reference's whole -out file of
                                   mpiexec -n 4 metacache_mpi query mini r1.fq r2.fq -pairfiles -lowest sequence -threads 2
                                       -maxcand 4 -hitmin 4 -hitdiff 80 -query-limit 128 -align
                                 run where genomes/all.fna (the name the shard files store) exists
  mini/P4/cli_seq_plain.out.gz   the same line without -align

The run fails if fewer than half of the mapping lines of the -align run carry an alignment block.

The shapes of cases.json.gz are the smallest at which a kernel that sweeps the matrix in strips of 8 columns per lane and panels of
512 columns can go wrong: query lengths 1, 2, 7, 8, 9, 63, 64, 65; subject lengths 1, 63, 64, 65, 127, 128, 129, 511, 512, 513; 4096
against a query of 65; an empty query and an empty subject; homopolymers against longer homopolymers (every cell and every end
position ties); a read embedded in its subject; a read overhanging either end; lower-case bases and N; `A` against `C` and `AC`
against `G`, which score -1; and a few larger pairs whose predecessor matrix exceeds 10240 words of 8 cells.

usage: python tests/golden/make_golden_alignment.py
"""
import gzip
import json
import os
import random
import shutil
import subprocess
import sys
import tempfile

from make_golden import HERE, REF, ensure_mpilib, mutate, rand_seq, sh, write_fastq

DRIVER = r"""
#include <iostream>
#include <string>
#include <type_traits>
#include "alignment.h"
int main() {
    std::string q, s;
    const auto scheme = mc::default_alignment_scheme{};
    while (std::getline(std::cin, q) && std::getline(std::cin, s)) {
        if (q == "-") q.clear();
        if (s == "-") s.clear();
        auto a = mc::align_semi_global(q, s, scheme);
        std::cout << a.score << '\n' << std::string(a.query.begin(), a.query.end()) << '\n'
                  << std::string(a.subject.begin(), a.subject.end()) << '\n';
    }
}
"""

QLENS = [1, 2, 7, 8, 9, 63, 64, 65]
SLENS = [1, 63, 64, 65, 127, 128, 129, 511, 512, 513]


def revcomp_acgt(s):
    return s[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca"))


def indel(rng, s, n):
    out = list(s)
    for _ in range(n):
        if not out:
            break
        i = rng.randrange(len(out))
        if rng.random() < 0.5:
            del out[i]
        else:
            out.insert(i, rng.choice("ACGT"))
    return "".join(out)


def read_of(rng, subject, n, rc=False):
    """a read of exactly n bases that resembles a stretch of the subject (substitutions and indels)"""
    if len(subject) >= n:
        a = rng.randrange(len(subject) - n + 1)
        r = subject[a:a + n]
    else:
        r = subject + rand_seq(rng, n - len(subject))
    r = indel(rng, mutate(rng, r, 0.05), n // 30)
    r = (r + rand_seq(rng, n))[:n]
    return revcomp_acgt(r) if rc else r


def make_pairs():
    rng = random.Random(20261019)
    pairs = []
    for k, ls in enumerate(SLENS):
        for m, lq in enumerate(QLENS):
            sub = rand_seq(rng, ls)
            pairs.append((read_of(rng, sub, lq, rc=(k + m) % 3 == 0), sub))
    sub = rand_seq(rng, 4096)
    pairs.append((read_of(rng, sub, 65), sub))
    pairs += [("", "ACGT"), ("ACGT", ""), ("", ""), ("A", "C"), ("AC", "G"), ("A", "A"), ("N", "N"), ("a", "A")]
    for c, lq, ls in (("A", 5, 9), ("A", 9, 5), ("C", 64, 130), ("T", 65, 513), ("G", 8, 8), ("N", 7, 20)):
        pairs.append((c * lq, c * ls))
    sub = rand_seq(rng, 467)
    read = sub[200:350]
    pairs.append((read, sub))                                       # embedded
    pairs.append((rand_seq(rng, 40) + sub[:110], sub))              # overhangs the left end
    pairs.append((sub[-110:] + rand_seq(rng, 40), sub))             # overhangs the right end
    pairs.append((revcomp_acgt(mutate(rng, read, 0.03)), sub))      # embedded, other strand
    low = "".join(ch.lower() if rng.random() < 0.3 else ch for ch in sub)
    pairs.append((read, low))                                       # case matters
    pairs.append((read[:60] + "NNNN" + read[64:], sub[:260] + "NNNN" + sub[264:]))
    pairs.append((low[100:250], low))
    # beyond 10240 predecessor words of 8 cells
    for lq, ls in ((100, 900), (300, 600), (150, 1100)):
        sub = rand_seq(rng, ls)
        pairs.append((read_of(rng, sub, lq), sub))
    out, seen = [], set()
    for q, s in pairs:
        for qq in (q, revcomp_acgt(q)):
            if (qq, s) not in seen:
                seen.add((qq, s)); out.append((qq, s))
    return out


def make_cases(work):
    src = os.path.join(work, "driver.cpp")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(work, "driver")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-w", "-I/root/reference/src", src, "-o", exe])
    pairs = make_pairs()
    text = "".join("%s\n%s\n" % (q or "-", s or "-") for q, s in pairs)
    got = subprocess.run([exe], input=text, stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    cases = []
    for i, (q, s) in enumerate(pairs):
        cases.append([q, s, int(got[3 * i]), got[3 * i + 1], got[3 * i + 2]])
    os.makedirs(os.path.join(HERE, "align"), exist_ok=True)
    with gzip.GzipFile(os.path.join(HERE, "align", "cases.json.gz"), "wb", mtime=0) as fo:
        fo.write(json.dumps(cases, separators=(",", ":")).encode())
    print("align/cases.json.gz: %d cases, scores %d .. %d" % (len(cases), min(c[2] for c in cases), max(c[2] for c in cases)))


def make_cli(work):
    tag, P = "mini", 4
    d = os.path.join(HERE, tag)
    os.makedirs(os.path.join(work, "genomes"))
    with gzip.open(os.path.join(d, "genomes.fa.gz"), "rt") as f, open(os.path.join(work, "genomes", "all.fna"), "w") as o:
        o.write(f.read())
    for r in range(P):
        shutil.copy(os.path.join(d, "P%d" % P, "%s.db_%d" % (tag, r)), work)
    with open(os.path.join(d, "queries.json")) as f:
        q = json.load(f)
    write_fastq(os.path.join(work, "r1.fq"), q["names"], q["r1"])
    write_fastq(os.path.join(work, "r2.fq"), q["names"], q["r2"])
    base = ["/opt/conda/bin/mpiexec", "-n", str(P), os.path.join(REF, "metacache_mpi"), "query", tag, "r1.fq", "r2.fq", "-pairfiles",
            "-lowest", "sequence", "-threads", "2", "-maxcand", "4", "-hitmin", "4", "-hitdiff", "80", "-query-limit", "128"]
    out, plain = os.path.join(work, "align.txt"), os.path.join(work, "plain.txt")
    sh(base + ["-out", out, "-align"], cwd=work)
    sh(base + ["-out", plain], cwd=work)
    lines = open(out).read().split("\n")
    blocks = sum(1 for l in lines if l.startswith("#   score  "))
    mapping = sum(1 for l in lines if l and not l.startswith("#"))
    print("mini P=4 -lowest sequence -align: %d alignment blocks over %d mapping lines" % (blocks, mapping))
    if 2 * blocks < mapping:
        sys.exit("fewer than half of the mapping lines carry an alignment block")
    for src, name in ((out, "cli_align"), (plain, "cli_seq_plain")):
        with open(src, "rb") as fi, gzip.GzipFile(os.path.join(d, "P%d" % P, "%s.out.gz" % name), "wb", mtime=0) as fo:
            fo.write(fi.read())


def main():
    work = tempfile.mkdtemp(prefix="golden_align_")
    try:
        make_cases(work)
        make_cli(os.path.join(work, "cli"))
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    if not os.path.isdir("/root/reference"):
        sys.exit("needs /root/reference (build container only)")
    ensure_mpilib()
    main()
