#!/usr/bin/env python3
"""What pass 2 of mcq_annotate_cli -- the join of mapping text against the ids of a genome file -- costs (run
on the GPU box from the repo root).

A mapping text of --lines (default 2^24) strict lines `acc TAB acc.1 TAB taxid TAB gi` (about 40 bytes each) and a FASTA of --ids
(default 50 000) one-line records whose ids are drawn from it are generated.  Then, in the same session, --runs of each:

    mcq_annotate_cli taxid FASTA MAP -out OUT -mapper gpu  -timing      the join's milliseconds, and of them the time inside
    mcq_annotate_cli taxid FASTA MAP -out OUT -mapper host -timing      mcq_accmap_chunk (copy to the device and the five kernels)
    oracle/_ref/metacache_mpi annotate taxid FASTA MAP -out OUT         the reference, wall time, if the binary is there and runs

The outputs of the three are compared.  Nothing is tuned here: the numbers are what the first version does.  Writes --out (default
profiles/annotate_rate.json) and prints it."""
import argparse
import importlib
import json
import os
import random
import re
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def generate(workdir, n_lines, n_ids, seed):
    rng = random.Random(seed)
    path, fasta = os.path.join(workdir, "gen.accession2taxid"), os.path.join(workdir, "in.fa")
    picks = set(rng.sample(range(n_lines), n_ids - n_ids // 10))           # a tenth of the ids is named by no line
    n_bytes = 0
    with open(path, "wb") as f, open(fasta, "wb") as g:
        f.write(b"accession\taccession.version\ttaxid\tgi\n")
        block = 1 << 16
        for b in range(0, n_lines, block):
            text = b"".join(b"AB%09d\tAB%09d.1\t%d\t%d\n" % (i, i, 1 + (i * 2654435761) % 2000000, 100000000 + i) for i in range(b, min(n_lines, b + block)))
            f.write(text)
            n_bytes += len(text)
        for i in sorted(picks):
            g.write(b">AB%09d.1 generated\nACGTACGTACGTACGT\n" % i)
        for i in range(n_ids // 10):
            g.write(b">ZZ%09d.1 named by no line\nACGTACGTACGTACGT\n" % i)
    return path, fasta, n_bytes


def run_cli(cli, fasta, mapping, out, mapper):
    t0 = time.perf_counter()
    p = subprocess.run([cli, "taxid", fasta, mapping, "-out", out, "-mapper", mapper, "-timing"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    wall = time.perf_counter() - t0
    if p.returncode != 0:
        return {"error": p.stderr[-1000:]}
    res = {"wall_s": round(wall, 3)}
    m = re.search(r"phases ms: ids ([\d.e+]+), join ([\d.e+]+) \(gpu chunks ([\d.e+]+) in (\d+) calls, host parser ([\d.e+]+) in (\d+) files\), text ([\d.e+]+); ids (\d+)", p.stderr)
    if m:
        res.update(ids_ms=float(m.group(1)), join_ms=float(m.group(2)), gpu_chunk_calls_ms=float(m.group(3)), gpu_chunks=int(m.group(4)),
                   host_parser_ms=float(m.group(5)), host_parser_files=int(m.group(6)), text_ms=float(m.group(7)), distinct_ids=int(m.group(8)))
        if res["join_ms"] > 0:
            res["gpu_share_of_join"] = round(res["gpu_chunk_calls_ms"] / res["join_ms"], 3)
    return res


def run_reference(fasta, mapping, out):
    ref = os.path.join(ROOT, "oracle", "_ref", "metacache_mpi")
    if not os.path.exists(ref):
        return {"skipped": "oracle/_ref/metacache_mpi is not there"}
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(ROOT, "oracle", "_ref", "mpilib")
    t0 = time.perf_counter()
    try:
        p = subprocess.run([ref, "annotate", "taxid", fasta, mapping, "-out", out], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    except (OSError, subprocess.TimeoutExpired) as e:
        return {"error": str(e)[-500:]}
    if p.returncode != 0 or not os.path.exists(out):
        return {"error": (p.stdout + p.stderr)[-500:]}
    return {"wall_s": round(time.perf_counter() - t0, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=1 << 24)
    ap.add_argument("--ids", type=int, default=50000)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--seed", type=int, default=20261021)
    ap.add_argument("--workdir", default="/tmp/mcq_annotate_rate")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "annotate_rate.json"))
    a = ap.parse_args()
    pkg = importlib.import_module("metacache-mpi_amd")          # (built before: __graft_entry__.build())
    shutil.rmtree(a.workdir, ignore_errors=True)
    os.makedirs(a.workdir)
    t0 = time.perf_counter()
    mapping, fasta, n_bytes = generate(a.workdir, a.lines, a.ids, a.seed)
    res = {"mapping_lines": a.lines, "mapping_bytes": n_bytes, "ids": a.ids, "generated_in_s": round(time.perf_counter() - t0, 1),
           "note": "measured, nothing tuned; join_ms is pass 2 of the program, gpu_chunk_calls_ms the time inside mcq_accmap_chunk"}
    cli = pkg.annotate_cli_path()
    outs = {m: os.path.join(a.workdir, "out_%s.fa" % m) for m in ("gpu", "host", "reference")}
    res["mapper_gpu"] = [run_cli(cli, fasta, mapping, outs["gpu"], "gpu") for _ in range(a.runs)]
    res["mapper_host"] = [run_cli(cli, fasta, mapping, outs["host"], "host") for _ in range(a.runs)]
    res["reference"] = run_reference(fasta, mapping, outs["reference"])
    for k in ("mapper_gpu", "mapper_host"):
        best = min((r["join_ms"] for r in res[k] if "join_ms" in r), default=None)
        if best:
            res[k + "_best_join_GBps"] = round(n_bytes / best / 1e6, 3)

    def same(x, y):
        return os.path.exists(x) and os.path.exists(y) and open(x, "rb").read() == open(y, "rb").read()
    res["gpu_output_equals_host_output"] = same(outs["gpu"], outs["host"])
    if "wall_s" in res["reference"]:
        res["gpu_output_equals_reference_output"] = same(outs["gpu"], outs["reference"])
        res["host_output_equals_reference_output"] = same(outs["host"], outs["reference"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))
    shutil.rmtree(a.workdir, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
