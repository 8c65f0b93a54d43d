#!/usr/bin/env python3
"""Generate the clade-exclusion fixtures under tests/golden/ by RUNNING the reference.

Runs only in the build container (needs /root/reference and oracle/_ref/metacache_mpi, built by
`make -C oracle ref`).  Queries the committed shard files with the reads of queries.json under new headers
(<tag>/eval_headers.json, written here and committed: the tests read that file, not this script):

  q%04d_g%d  ->  q%04d_g%d taxid|<id of genome g's parent taxon: its species, or what the target hangs under>
                 (lower-case names: no accession prefix matches, every rank resolves the same truth)
  every fifth of them gets the id of that taxon's genus instead: under -exclude species the truth has no ancestor at
                 the rank, and null equals null (src/classification.cpp:141-157)
  one read gets taxid|999999, which the taxonomy does not have: no truth
  the e_* reads keep their names: no truth, nothing excluded

with the options of make_golden.py's make_cliout (-threads 2 -query-limit 128 -maxcand -hitmin 4 -hitdiff 80) plus
-exclude, and keeps the reference's whole -out file:

  mini/P4/cli_excl_species.out.gz         -exclude species
  mini/P4/cli_excl_genus_tophits.out.gz   -exclude genus -tophits
  tie/P2/cli_excl_species.out.gz          -exclude species
  noanc/P2/cli_excl_species.out.gz        -exclude species   (the null case removes the target that has no species)

A run fails here if fewer than one tenth of its mapping lines differ from the same run without -exclude: a fixture that
exclusion does not touch pins nothing.  mini is also run once with -exclude species -precision -ground-truth, and what
the MPI program's rank 0 prints of the truth is reported.

usage: python tests/golden/make_golden_evaluation.py
"""
import gzip
import json
import os
import shutil
import sys
import tempfile

from make_golden import HERE, REF, ensure_mpilib, sh, write_fastq

RUNS = [("mini", 4, "species", ["-exclude", "species"]),
        ("mini", 4, "genus_tophits", ["-exclude", "genus", "-tophits"]),
        ("tie", 2, "species", ["-exclude", "species"]),
        ("noanc", 2, "species", ["-exclude", "species"])]
GENUS = 6          # taxonomy::rank::Genus


def gz(src, dst):
    with open(src, "rb") as fi, gzip.GzipFile(dst, "wb", mtime=0) as fo:
        fo.write(fi.read())


def shard_taxa(path):
    """(id, parent, rank) of every taxon of a shard file (src/sketch_database.h:959-998, src/taxonomy.h:326-335)"""
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from oracle import dbfile
    return dbfile.parse_shard(path)["taxa"]


def eval_headers(tag, P, names):
    taxa = shard_taxa(os.path.join(HERE, tag, "P%d" % P, "%s.db_0" % tag))
    by_id = {t["id"]: t for t in taxa}

    def genus_of(tid):
        cur = tid
        while cur in by_id and cur != 0:
            t = by_id[cur]
            if t["rank"] == GENUS:
                return cur
            cur = t["parent"] if t["parent"] != cur else 0
        return tid

    out, k = [], 0
    for n in names:
        if not n.startswith("q"):
            out.append(n)
            continue
        g = int(n.split("_g")[1])
        parent = by_id[-(g + 1)]["parent"]
        tid = 999999 if k == 7 else (genus_of(parent) if k % 5 == 4 else parent)
        out.append("%s taxid|%d" % (n, tid))
        k += 1
    return out


def mapping_lines(path):
    return [l for l in open(path).read().split("\n") if l and not l.startswith("#")]


def by_header(lines):
    """mapping line of every read, by its header (the first column): two runs are compared read by read"""
    return {l.split("\t|\t")[0]: l for l in lines}


def main():
    done = {}
    for tag, P, name, extra in RUNS:
        d = os.path.join(HERE, tag, "P%d" % P)
        with open(os.path.join(HERE, tag, "queries.json")) as f:
            q = json.load(f)
        if tag not in done:
            done[tag] = eval_headers(tag, P, q["names"])
            with open(os.path.join(HERE, tag, "eval_headers.json"), "w") as f:
                json.dump(done[tag], f, indent=0)
        headers = done[tag]
        work = tempfile.mkdtemp(prefix="golden_eval_" + tag + "_")
        for r in range(P):
            shutil.copy(os.path.join(d, "%s.db_%d" % (tag, r)), work)
        write_fastq(os.path.join(work, "r1.fq"), headers, q["r1"])
        write_fastq(os.path.join(work, "r2.fq"), headers, q["r2"])
        base = ["/opt/conda/bin/mpiexec", "-n", str(P), os.path.join(REF, "metacache_mpi"),
                "query", tag, "r1.fq", "r2.fq", "-pairfiles", "-lowest", q["lowest"], "-threads", "2",
                "-maxcand", str(q["maxcand"]), "-hitmin", "4", "-hitdiff", "80", "-query-limit", "128"]
        out, plain = os.path.join(work, "out.txt"), os.path.join(work, "plain.txt")
        sh(base + ["-out", out] + extra, cwd=work)
        sh(base + ["-out", plain] + [x for x in extra if x not in ("-exclude", "species", "genus")], cwd=work)
        a, b = by_header(mapping_lines(out)), by_header(mapping_lines(plain))
        differ = sum(1 for h in a if a[h] != b.get(h))
        print("%s P=%d cli_excl_%s: %d mapping lines, %d differ from the run without -exclude" % (tag, P, name, len(a), differ))
        if set(a) != set(b) or differ * 10 < len(a):
            sys.exit("%s %s: exclusion touches fewer than one tenth of the mapping lines: choose another rank for this run" % (tag, name))
        gz(out, os.path.join(d, "cli_excl_%s.out.gz" % name))
        if (tag, name) == ("mini", "species"):           # what the MPI program keeps of the truth (defect b)
            ev = os.path.join(work, "eval.txt")
            sh(base + ["-out", ev, "-exclude", "species", "-precision", "-ground-truth"], cwd=work)
            text = open(ev).read()
            lines = mapping_lines(ev)
            cols = [l.split("\t|\t") for l in lines]
            print("mini -exclude species -precision -ground-truth: 'ground truth known' block: %s; 'ground truth' in the header line: %s; "
                  "columns per mapping line: %s; mapping lines that differ from the -exclude run: %d" %
                  ("yes" if "ground truth known" in text else "no",
                   "yes" if any("truth" in l for l in text.split("\n") if l.startswith("#")) else "no",
                   sorted(set(len(c) for c in cols)), sum(1 for c in cols if "\t|\t".join([c[0]] + c[-1:]) != a.get(c[0]))))
            for l in text.split("\n"):
                if l.startswith("#") and ("truth" in l or "precision" in l or "correct" in l or "known" in l or "TABLE_LAYOUT" in l):
                    print("    " + l)
            print("    first mapping line: " + (lines[0] if lines else ""))
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    if not os.path.isdir("/root/reference"):
        sys.exit("needs /root/reference (build container only)")
    ensure_mpilib()
    main()
