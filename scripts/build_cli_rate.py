#!/usr/bin/env python3
"""mcq_build_cli on the genome set of bench.py's table (run on the GPU box from the repo root).

Writes the 50 species x 10 strains of bench.py's generator (2 Gbp, seed 3) as one FASTA file per genome, lines of 80, with
a taxonomy dump of root > Bacteria > species, reads the files once into the page cache, and runs
`mcq_build_cli db 2 genomes -taxonomy tax` --runs times, every run a child process under `timeout`.  Per run: the wall
time, the program's own phase times (MCQ_BUILD_TRACE=1: read, sketch + sort, rank split, write) and the peak RSS
(os.wait4 of the child).

The yardstick of the rank split is the host-side split of scripts/reference_at_scale.py (numpy: key index per location,
tgt % P, unique + counts per rank) on the same table -- built by mcq_build_table from the same bases -- alternating with the
device split (mcq_table_rank_split of every rank + the copies to the host, what the program's "rank split" phase holds).
Writes profiles/build_cli_rate.json, or the file --out names.
"""
import argparse
import importlib
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHILD = ("import json, os, subprocess, sys, time\n"
         "t0 = time.time()\n"
         "p = subprocess.Popen(sys.argv[2:], stdout=subprocess.DEVNULL, stderr=open(sys.argv[1], 'wb'))\n"
         "_, status, ru = os.wait4(p.pid, 0)\n"
         "print(json.dumps([os.waitstatus_to_exitcode(status), ru.ru_maxrss * 1024, time.time() - t0]))\n")


def write_inputs(a, gb, goff, species):
    acgt_lines = 80
    g = gb.cpu().numpy()
    off = goff.cpu().numpy().astype(np.int64)
    sp = species.cpu().numpy().astype(np.int64)
    os.makedirs(os.path.join(a.workdir, "genomes")); os.makedirs(os.path.join(a.workdir, "tax"))
    for t in range(len(off) - 1):
        s = g[off[t]:off[t + 1]]
        full = len(s) // acgt_lines * acgt_lines
        body = np.full((full // acgt_lines, acgt_lines + 1), 10, np.uint8)
        body[:, :acgt_lines] = s[:full].reshape(-1, acgt_lines)
        with open(os.path.join(a.workdir, "genomes", "g%05d.fna" % t), "wb") as f:
            f.write(b">NC_%06d.1 Synthetica species%d strain %d taxid|%d\n" % (t + 1, sp[t], t, 1000 + sp[t]))
            f.write(body.tobytes())
            if full < len(s):
                f.write(s[full:].tobytes() + b"\n")
    with open(os.path.join(a.workdir, "tax", "nodes.dmp"), "w") as nodes, open(os.path.join(a.workdir, "tax", "names.dmp"), "w") as names:
        rows = [(1, 1, "no rank", "root"), (2, 1, "superkingdom", "Bacteria")] + \
               [(1000 + int(s_), 2, "species", "Synthetica species%d" % s_) for s_ in sorted(set(int(x) for x in sp))]
        for tid, parent, rank, name in rows:
            nodes.write("%d\t|\t%d\t|\t%s\t|\t\t|\n" % (tid, parent, rank))
            names.write("%d\t|\t%s\t|\t\t|\tscientific name\t|\n" % (tid, name))


def host_split(keys, loff, locs, P):
    """the split of scripts/reference_at_scale.py: every rank's keys, offsets and locations"""
    key_of = np.repeat(np.arange(len(keys), dtype=np.int64), np.diff(loff.astype(np.int64)))
    rank_of = (locs >> np.uint64(32)).astype(np.int64) % P
    out = []
    for rk in range(P):
        sel = rank_of == rk
        kk, cnt = np.unique(key_of[sel], return_counts=True)
        o = np.zeros(len(kk) + 1, np.uint64); o[1:] = np.cumsum(cnt)
        out.append((keys[kk], o, locs[sel]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--species", type=int, default=50)
    ap.add_argument("--strains", type=int, default=10)
    ap.add_argument("--genome-min", type=int, default=3_000_000)
    ap.add_argument("--genome-max", type=int, default=5_000_000)
    ap.add_argument("--divergence", type=float, default=0.02)
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per run of the program")
    ap.add_argument("--workdir", default="/tmp/mcq_build_rate")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "build_cli_rate.json"))
    a = ap.parse_args()

    import torch
    pkg = importlib.import_module("metacache-mpi_amd")
    pkg.build_hip(); pkg.build_host()
    eng = importlib.import_module("metacache-mpi_amd.engine")
    synth = importlib.import_module("metacache-mpi_amd.synth")
    dev = torch.device("cuda", 0)
    P = a.ranks
    shutil.rmtree(a.workdir, ignore_errors=True)
    os.makedirs(a.workdir)
    gb, goff, species = synth.make_genomes(a.species, a.strains, a.genome_min, a.genome_max, a.divergence, seed=3, device=dev)
    write_inputs(a, gb, goff, species)
    n_targets = goff.numel() - 1
    res = {"table": "%d species x %d strains" % (a.species, a.strains), "targets": int(n_targets), "db_bp": int(goff[-1]), "ranks": P,
           "device": torch.cuda.get_device_name(0), "fasta_bytes": 0}
    for f in sorted(os.listdir(os.path.join(a.workdir, "genomes"))):          # once into the page cache
        with open(os.path.join(a.workdir, "genomes", f), "rb") as fh:
            while True:
                b = fh.read(1 << 24)
                if not b:
                    break
                res["fasta_bytes"] += len(b)

    # ---- the rank split alone: device against host, alternating, on the table built from the same bases
    table = eng.Table(gb.data_ptr(), goff.data_ptr(), n_targets, emulate_ranks=P, device=0)
    del gb
    torch.cuda.empty_cache()
    res.update(db_keys=table.n_keys, db_locations=table.n_locs)
    dev_s, host_s, same = [], [], True
    for _ in range(a.runs):
        torch.cuda.synchronize()
        t0 = time.time()
        parts = []
        for r in range(P):
            p = table.rank_split(P, r)
            parts.append(p.to_host()[:3])
            p.close()
        dev_s.append(time.time() - t0)
        t0 = time.time()
        keys, loff, locs, _ = table.to_host()
        ref = host_split(keys, loff, locs, P)
        host_s.append(time.time() - t0)
        same = same and all(np.array_equal(x, y) for pa, pb in zip(parts, ref) for x, y in zip(pa, pb))
        del parts, ref, keys, loff, locs
    table.close()
    res["rank_split"] = {"device_split_and_copies_s": [round(x, 3) for x in dev_s], "host_copy_and_numpy_split_s": [round(x, 3) for x in host_s],
                         "device_median_s": round(statistics.median(dev_s), 3), "host_median_s": round(statistics.median(host_s), 3),
                         "identical": bool(same)}

    # ---- the program
    runs = []
    for i in range(a.runs):
        err = os.path.join(a.workdir, "stderr_%d.txt" % i)
        r = subprocess.run([sys.executable, "-c", CHILD, err, "timeout", "-k", "10", str(a.timeout), pkg.build_cli_path(), "db", str(P), "genomes",
                            "-taxonomy", "tax"], cwd=a.workdir, env=dict(os.environ, MCQ_BUILD_TRACE="1"), stdout=subprocess.PIPE, text=True)
        rc, rss, wall = json.loads(r.stdout)
        text = open(err).read()
        if rc != 0:
            print(text[-3000:]); sys.exit("mcq_build_cli failed (status %d)" % rc)        # nothing more is started on the GPU
        ph = {m.group(1).strip(): float(m.group(2)) for m in re.finditer(r"^\[mcq_build_cli\] (.+?)\s+([0-9.]+) s$", text, flags=re.M)}
        runs.append({"wall_s": round(wall, 3), "peak_rss_bytes": rss, "phases_s": ph})
    res["runs"] = runs
    res["wall_median_s"] = round(statistics.median(x["wall_s"] for x in runs), 3)
    res["phases_median_s"] = {k: round(statistics.median(x["phases_s"].get(k, 0.0) for x in runs), 3) for k in ("read", "sketch + sort", "rank split", "write")}
    res["peak_rss_median_bytes"] = int(statistics.median(x["peak_rss_bytes"] for x in runs))
    res["shard_file_bytes"] = [os.path.getsize(os.path.join(a.workdir, "db.db_%d" % r)) for r in range(P)]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))
    shutil.rmtree(a.workdir, ignore_errors=True)


if __name__ == "__main__":
    main()
