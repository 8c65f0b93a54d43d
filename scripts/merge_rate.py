#!/usr/bin/env python3
"""Rate of a merge of three result files of 2^22 lines each: mcq_merge_cli with its phases (read, parse + apply, finish, write), and,
where oracle/_ref/metacache_mpi exists (the build machine), the reference's merge of the same files.

The files are made here, seeded, in the form mcq_query_cli writes with -tophits -queryids -lowest species: every read once per file,
0-4 top_hits of a made-up taxonomy of 2000 species in 200 genera, hits descending.  (Not through mcq_query_cli on a table split three
ways: the merge reads text, and the text has the same form; the lines here are about 60 bytes, as those of short read names are.)

usage: python scripts/merge_rate.py --side ours|reference [--lines N] [--work DIR] [--out profiles/merge_rate.json]
The --out file is read, this side's numbers are put into it, and it is written back: both sides end up in one file.
"""
import argparse
import json
import os
import random
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_taxonomy(d):
    os.makedirs(d, exist_ok=True)
    nodes = [(1, 1, "no rank", "root"), (2, 1, "superkingdom", "Dom"), (10, 2, "phylum", "Phy"), (20, 10, "class", "Cls"), (30, 20, "order", "Ord"),
             (40, 30, "family", "Fam")]
    species = []
    for g in range(200):
        gid = 1000 + g * 100
        nodes.append((gid, 40, "genus", "Gen%d" % g))
        for s in range(1, 11):
            nodes.append((gid + s, gid, "species", "Gen%d sp%d" % (g, s)))
            species.append(gid + s)
    with open(os.path.join(d, "nodes.dmp"), "w") as f:
        for t, p, r, _ in nodes:
            f.write("%d\t|\t%d\t|\t%s\t|\t\t|\n" % (t, p, r))
    with open(os.path.join(d, "names.dmp"), "w") as f:
        for t, _, _, n in nodes:
            f.write("%d\t|\t%s\t|\t\t|\tscientific name\t|\n" % (t, n))
    return species


HEAD = ("# Reporting per-read mappings (non-mapping lines start with '# ').\n# Only the lowest matching rank will be reported.\n"
        "# Classification will be constrained to ranks from 'species' to 'domain'.\n# Classification hit threshold is 4 per query\n"
        "# At maximum 4 classification candidates will be considered per query.\n# Using 16 threads\n"
        "# TABLE_LAYOUT: query_id\t|\tquery_header\t|\ttop_hits\t|\trank:taxname\n# reads.fq\n")


def write_results(path, species, n_lines, seed):
    rng = random.Random(seed)
    pool = []
    for _ in range(8192):                                        # top_hits columns: near relatives, as a read's candidates are
        g = rng.randrange(200)
        near = [t for t in species[g * 10:g * 10 + 10]] + [rng.choice(species)]
        items = sorted(((rng.randrange(4, 40), t) for t in rng.sample(near, rng.randrange(0, 5))), reverse=True)
        pool.append(",".join("%d:%d" % (t, h) for h, t in items))
    with open(path, "w") as f:
        f.write(HEAD)
        for lo in range(1, n_lines + 1, 65536):
            ks = [rng.randrange(8192) for _ in range(lo, min(lo + 65536, n_lines + 1))]
            f.write("".join("%d\t|\tread_%d/1\t|\t%s\t|\tspecies:x\n" % (lo + i, lo + i, pool[k]) for i, k in enumerate(ks)))
    return os.path.getsize(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", choices=["ours", "reference"], required=True)
    ap.add_argument("--lines", type=int, default=1 << 22)
    ap.add_argument("--work", default="/tmp/mcq_merge_rate")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_rate.json"))
    a = ap.parse_args()
    os.makedirs(a.work, exist_ok=True)
    species = write_taxonomy(os.path.join(a.work, "tax"))
    files = ["res_%d.txt" % k for k in range(3)]
    nbytes = sum(write_results(os.path.join(a.work, f), species, a.lines, 100 + k) for k, f in enumerate(files))
    for f in files:                                              # into the page cache
        with open(os.path.join(a.work, f), "rb") as fh:
            while fh.read(1 << 24):
                pass
    opts = ["-taxonomy", "tax", "-hitmin", "4", "-maxcand", "4", "-lowest", "species", "-tophits", "-queryids", "-out", "merged_%s.txt" % a.side]
    if a.side == "ours":
        sys.path.insert(0, ROOT)
        import importlib
        pkg = importlib.import_module("metacache-mpi_amd")
        cmd = [pkg.merge_cli_path()] + files + opts + ["-threads", "16"]
        env = None
    else:
        ref = os.path.join(ROOT, "oracle", "_ref")
        cmd = ["/opt/conda/bin/mpiexec", "-n", "1", os.path.join(ref, "metacache_mpi"), "merge"] + files + opts
        env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ref, "mpilib"))
    t0 = time.time()
    r = subprocess.run(cmd, cwd=a.work, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    wall = time.time() - t0
    if r.returncode != 0:
        sys.exit("failed: %s\n%s" % (" ".join(cmd), r.stderr[-2000:]))
    side = {"command": " ".join(os.path.basename(c) if os.sep in c else c for c in cmd), "wall_s": round(wall, 3),
            "lines_per_s": round(3 * a.lines / wall), "MB_per_s": round(nbytes / wall / 1e6, 1)}
    if a.side == "ours":
        m = re.search(r"phases ms: read ([\d.e+]+), parse\+apply ([\d.e+]+), finish ([\d.e+]+), write ([\d.e+]+), all ([\d.e+]+)", r.stderr)
        side["phases_ms"] = dict(zip(["read", "parse_apply", "finish", "write", "all"], [float(x) for x in m.groups()]))
        side["chunks"] = re.search(r"chunks parsed on the GPU: \d+, on the host: \d+", r.stderr).group(0)
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc.update({"files": 3, "lines_per_file": a.lines, "bytes": nbytes})
    doc[a.side] = side
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc[a.side]))
    if a.side == "ours" and os.path.exists(os.path.join(a.work, "merged_reference.txt")):
        strip = lambda t: [l for l in t.split("\n") if not l.startswith(("# time:", "# speed:", "# Using"))]
        same = strip(open(os.path.join(a.work, "merged_ours.txt")).read()) == strip(open(os.path.join(a.work, "merged_reference.txt")).read())
        print("equal to the reference's output: %s" % same)


if __name__ == "__main__":
    main()
