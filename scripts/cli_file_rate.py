#!/usr/bin/env python3
"""mcq_query_cli from read files, this tree against the parent commit (run on the GPU box from the repo root).

Builds the table of scripts/reference_at_scale.py's defaults (50 species x 10 strains, 2 Gbp, built on the GPU and written
as the reference's shard files) or reuses one (--workdir with db.db_*), writes 2^22 read pairs of 150 bp as two FASTQ
files and reads them once into the page cache.  Then runs `mcq_query_cli db 2 r1.fq r2.fq -threads 16 -maxcand 2 ...` of
this tree and of the parent's build, alternating, --runs times each, every run under `timeout`.  Per run: the program's
own "# time:" (from the start of reading to the end of writing, as the reference times it), the peak RSS (os.wait4 of the
child), and whether its -out file equals the first run of the other tree once "# time:" / "# speed:" are masked.

The parent: --parent-cli PATH (a prebuilt mcq_query_cli with its libraries beside it), or --parent REV: a git worktree of
REV is built here.  Writes profiles/cli_file_rate.json, or the file --out names.

--interleaved: the same reads also as ONE interleaved file (il.fq: records 2q, 2q+1 are the mates of pair q) through this
tree's `-pairseq`, a third run in every round; its mapping lines (the lines that are no comments) are compared with the
parent's.  --kernel-stats: one more run of each form of this tree under `rocprofv3 --kernel-trace --stats`; the share of
the reader kernels (k_rd_*) in the kernel time goes into the result.
"""
import argparse
import hashlib
import importlib
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_table(a, dev):
    """the table of reference_at_scale.py (same generator, seed and taxonomy) -> <workdir>/db.db_0 .. db_{P-1}"""
    eng = importlib.import_module("metacache-mpi_amd.engine")
    host = importlib.import_module("metacache-mpi_amd.host")
    synth = importlib.import_module("metacache-mpi_amd.synth")
    P = a.ranks
    gb, goff, species = synth.make_genomes(a.species, a.strains, a.genome_min, a.genome_max, a.divergence, seed=3, device=dev)
    table = eng.Table(gb.data_ptr(), goff.data_ptr(), goff.numel() - 1, emulate_ranks=P, device=0)
    keys, loff, locs, _ = table.to_host()
    table.close()
    n_targets = goff.numel() - 1
    glen = np.diff(goff.cpu().numpy().astype(np.int64))
    sp = species.cpu().numpy().astype(np.int64)
    W, S = 128, 113
    nwin = np.where(glen <= W, 1, (glen - W) // S + 1 + (((glen - W) // S + 1) * S < glen))
    key_of = np.repeat(np.arange(len(keys), dtype=np.int64), np.diff(loff.astype(np.int64)))
    rank_of = (locs >> np.uint64(32)).astype(np.int64) % P
    for rk in range(P):
        taxa = [dict(id=-(t + 1), parent=1000 + int(sp[t]), rank=0, name="genome_%d strain" % t, file="genomes/all.fna", index=t + 1,
                     windows=int(nwin[t]) if t % P == rk else 0) for t in range(n_targets - 1, -1, -1)]
        taxa.append(dict(id=1, parent=1, rank=20, name="root", file="", index=0, windows=0))
        taxa.append(dict(id=2, parent=1, rank=19, name="Bacteria", file="", index=0, windows=0))
        for s_ in sorted(set(int(x) for x in sp)):
            taxa.append(dict(id=1000 + s_, parent=2, rank=4, name="Synthetica species%d" % s_, file="", index=0, windows=0))
        sel = rank_of == rk
        kk, cnt = np.unique(key_of[sel], return_counts=True)
        o = np.zeros(len(kk) + 1, np.uint64); o[1:] = np.cumsum(cnt)
        host.write_shard(os.path.join(a.workdir, "db.db_%d" % rk),
                         dict(k=16, sketch_size=16, winlen=W, winstride=S, q_k=16, q_sketch_size=16, q_winlen=W, q_winstride=S,
                              max_locs_per_feature=254),
                         taxa, n_targets, keys[kk], o, locs[sel])
    return gb, goff, int(glen.sum())


def write_reads(a, gb, goff):
    """2^k pairs sampled from the genomes (reference_at_scale.py's sampler), as r1.fq / r2.fq"""
    synth = importlib.import_module("metacache-mpi_amd.synth")
    n, L = a.pairs, a.read_len
    qual = np.full(L, ord("I"), np.uint8)
    with open(os.path.join(a.workdir, "r1.fq"), "wb") as f1, open(os.path.join(a.workdir, "r2.fq"), "wb") as f2:
        for b0 in range(0, n, 1 << 20):
            m = min(1 << 20, n - b0)
            r, _, _ = synth.sample_pairs(gb, goff, m, L, 300, 500, 0.005, 0.001, seed=1000 + b0)
            rb = r.cpu().numpy().reshape(m, 2, L)
            hdr = np.array([("@r%08d\n" % (b0 + i)).encode() for i in range(m)], dtype="S11").view(np.uint8).reshape(m, 11)
            for mate, f in ((0, f1), (1, f2)):
                rec = np.empty((m, 11 + L + 3 + L + 1), np.uint8)
                rec[:, :11] = hdr
                rec[:, 11:11 + L] = rb[:, mate, :]
                rec[:, 11 + L:14 + L] = np.frombuffer(b"\n+\n", np.uint8)
                rec[:, 14 + L:14 + 2 * L] = qual
                rec[:, -1] = ord("\n")
                f.write(rec.tobytes())


def build_parent(rev):
    wt = os.path.join(ROOT, "_parent_worktree")
    subprocess.check_call(["git", "-C", ROOT, "worktree", "add", "--detach", "--force", wt, rev])
    subprocess.check_call([sys.executable, "-c", "import importlib,sys; sys.path.insert(0,'.'); p=importlib.import_module('metacache-mpi_amd'); "
                           "p.build_hip(); p.build_host()"], cwd=wt)
    return os.path.join(wt, "metacache-mpi_amd", "mcq_query_cli")


# os.wait4's ru_maxrss counts what the child held before its exec -- a fork of this process, which holds the table -- so
# the program is started by a fresh small interpreter, which waits for it and reports its ru_maxrss
RSS_HELPER = ("import json, os, subprocess, sys\n"
              "p = subprocess.Popen(sys.argv[2:], stdout=subprocess.DEVNULL, stderr=open(sys.argv[1], 'wb'))\n"
              "_, status, ru = os.wait4(p.pid, 0)\n"
              "print(json.dumps([os.waitstatus_to_exitcode(status), ru.ru_maxrss * 1024]))\n")


def write_interleaved(a):
    """il.fq from r1.fq / r2.fq (records of one fixed size)"""
    rec = 11 + a.read_len + 3 + a.read_len + 1
    with open(os.path.join(a.workdir, "r1.fq"), "rb") as f1, open(os.path.join(a.workdir, "r2.fq"), "rb") as f2, \
            open(os.path.join(a.workdir, "il.fq"), "wb") as fo:
        while True:
            b1, b2 = f1.read(rec << 16), f2.read(rec << 16)
            if not b1:
                break
            m = len(b1) // rec
            both = np.empty((m, 2, rec), np.uint8)
            both[:, 0, :] = np.frombuffer(b1, np.uint8).reshape(m, rec)
            both[:, 1, :] = np.frombuffer(b2, np.uint8).reshape(m, rec)
            fo.write(both.tobytes())


def inputs(a, interleaved):
    if interleaved:
        return [os.path.join(a.workdir, "il.fq"), "-pairseq"]
    return [os.path.join(a.workdir, "r1.fq"), os.path.join(a.workdir, "r2.fq")]


def command(cli, a, out, interleaved=False):
    return [cli, os.path.join(a.workdir, "db"), str(a.ranks)] + inputs(a, interleaved) + ["-lowest", "species", "-maxcand", "2", "-hitmin", "4",
            "-hitdiff", "80", "-tophits", "-taxids-only", "-omit-ranks", "-threads", "16", "-out", out]


def kernel_stats(cli, a, interleaved, timeout_s):
    """one run under rocprofv3 --kernel-trace --stats -> (reader kernels' ns, all kernels' ns)"""
    import csv
    import glob
    d = os.path.join(a.workdir, "prof_il" if interleaved else "prof_files")
    subprocess.check_call(["timeout", "-k", "10", str(timeout_s), "rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run", "--output-format", "csv",
                           "--"] + command(cli, a, os.path.join(a.workdir, "prof.out"), interleaved), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    rd = total = 0
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                ns = int(float(row["TotalDurationNs"]))
                total += ns
                if "k_rd_" in row["Name"]:
                    rd += ns
    return rd, total


def run(cli, a, out, timeout_s, interleaved=False):
    cmd = ["timeout", "-k", "10", str(timeout_s)] + command(cli, a, out, interleaved)
    r = subprocess.run([sys.executable, "-c", RSS_HELPER, out + ".err"] + cmd, stdout=subprocess.PIPE, text=True)
    rc, rss = json.loads(r.stdout)
    if rc != 0:
        sys.exit("%s exited with %d: %s" % (cli, rc, open(out + ".err").read()[-2000:]))
    text = open(out).read()
    ms = int(re.search(r"^# time:    (\d+) ms$", text, flags=re.M).group(1))
    masked = re.sub(r"^# (time|speed): .*$", "# masked", text, flags=re.M)
    if interleaved:                                               # (its parameter lines and file line differ: the mapping lines)
        masked = "".join(l + "\n" for l in text.split("\n") if l and not l.startswith("#"))
    return ms, rss, hashlib.sha256(masked.encode()).hexdigest()


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "spread": max(xs) - min(xs), "runs": xs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--species", type=int, default=50)
    ap.add_argument("--strains", type=int, default=10)
    ap.add_argument("--genome-min", type=int, default=3_000_000)
    ap.add_argument("--genome-max", type=int, default=5_000_000)
    ap.add_argument("--divergence", type=float, default=0.02)
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=1 << 22)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--workdir", default=os.path.join(tempfile.gettempdir(), "mcq_cli_rate"))
    ap.add_argument("--parent", default="HEAD~1", help="git revision of the parent commit (built in a worktree)")
    ap.add_argument("--parent-cli", default="", help="a prebuilt mcq_query_cli of the parent instead")
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--interleaved", action="store_true", help="also run this tree on one interleaved file (-pairseq)")
    ap.add_argument("--kernel-stats", action="store_true", help="the reader kernels' share, from one rocprofv3 run of each form")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cli_file_rate.json"))
    a = ap.parse_args()

    pkg = importlib.import_module("metacache-mpi_amd")
    pkg.build_hip(); pkg.build_host()
    parent = a.parent_cli or build_parent(a.parent)
    os.makedirs(a.workdir, exist_ok=True)
    res = {"table": "%d species x %d strains" % (a.species, a.strains), "pairs": a.pairs, "reads": 2 * a.pairs, "read_len": a.read_len,
           "options": "-threads 16 -maxcand 2 -lowest species -hitmin 4 -hitdiff 80 -tophits -taxids-only -omit-ranks"}
    if not (os.path.exists(os.path.join(a.workdir, "db.db_0")) and os.path.exists(os.path.join(a.workdir, "r2.fq"))):
        import torch
        gb, goff, bp = build_table(a, torch.device("cuda", 0))
        write_reads(a, gb, goff)
        del gb, goff
        res["db_bp"] = bp
    res["file_bytes"] = sum(os.path.getsize(os.path.join(a.workdir, f)) for f in ("r1.fq", "r2.fq"))
    for f in ("r1.fq", "r2.fq"):                                  # into the page cache
        with open(os.path.join(a.workdir, f), "rb") as fh:
            while fh.read(1 << 26):
                pass
    trees = {"this": pkg.cli_path(), "parent": parent}
    if a.interleaved:
        if not os.path.exists(os.path.join(a.workdir, "il.fq")):
            write_interleaved(a)
        with open(os.path.join(a.workdir, "il.fq"), "rb") as fh:
            while fh.read(1 << 26):
                pass
        trees["this_interleaved"] = pkg.cli_path()
    runs = {k: {"ms": [], "rss": [], "digest": []} for k in trees}
    for i in range(a.runs):
        for k, cli in trees.items():
            ms, rss, dg = run(cli, a, os.path.join(a.workdir, "%s_%d.out" % (k, i)), a.timeout, k == "this_interleaved")
            runs[k]["ms"].append(ms); runs[k]["rss"].append(rss); runs[k]["digest"].append(dg)
            print("%-6s run %d: %d ms, peak RSS %.0f MB" % (k, i, ms, rss / 1e6), flush=True)
    ref = runs["parent"]["digest"][0]
    if a.interleaved:
        with open(os.path.join(a.workdir, "parent_0.out")) as f:
            ref_lines = hashlib.sha256("".join(l + "\n" for l in f.read().split("\n") if l and not l.startswith("#")).encode()).hexdigest()
        res["interleaved_mapping_lines_identical_to_parent"] = [d == ref_lines for d in runs["this_interleaved"]["digest"]]
    for k in trees:
        r = runs[k]
        res[k] = {"time_ms": summary(r["ms"]), "peak_rss_mb": summary([round(x / 1e6, 1) for x in r["rss"]]),
                  "out_identical_to_parent_first_run": [d == ref for d in r["digest"]],
                  "reads_per_s_median": round(2 * a.pairs / (statistics.median(r["ms"]) / 1000.0))}
    t, pa = res["this"]["time_ms"], res["parent"]["time_ms"]
    res["faster_beyond_spread"] = pa["median"] - t["median"] > max(t["spread"], pa["spread"])
    tr, pr = res["this"]["peak_rss_mb"], res["parent"]["peak_rss_mb"]         # the same rule turned round: a change meant to cost nothing
    res["slower_beyond_spread"] = t["median"] - pa["median"] > max(t["spread"], pa["spread"])
    res["more_rss_beyond_spread"] = tr["median"] - pr["median"] > max(tr["spread"], pr["spread"])
    res["identical_out_files"] = all(all(res[k]["out_identical_to_parent_first_run"]) for k in ("this", "parent"))
    if a.kernel_stats:
        for k in trees:
            if k != "parent":
                rd, total = kernel_stats(trees[k], a, k == "this_interleaved", a.timeout)
                res.setdefault("reader_kernels", {})[k] = {"k_rd_ns": rd, "all_kernels_ns": total, "share": round(rd / max(1, total), 4)}
    text = json.dumps(res, indent=1)
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
