#!/usr/bin/env python3
"""What `mcq_info_cli DB P statistics` costs on the benchmark's table (run on the GPU box from the repo root).

The benchmark's 2 Gbp table (50 species x 10 strains, 2 reference ranks) is built on the GPU and written as the reference's shard
files (scripts/tuned_load_rate.py's write_shards).  Then, in the same session:

    mcq_info_cli db 2 statistics -timing                                   wall time, and the program's own phases from stderr:
    mcq_info_cli db 2 statistics -max-locations-per-feature 8 -timing      record parsing (reader thread), the events around
                                                                           mcq_content_stats_add, all
    the streaming load of the same files (host.RefDb(meta_only).stream -> engine.PartsBuilder -> Parts.database), no rule

--runs of each.  The load is the yardstick: what reading the files costs anyway.  Writes --out (default profiles/info_rate.json)
and prints it."""
import argparse
import importlib
import json
import os
import re
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def run_info(cli, workdir, P, extra):
    t0 = time.perf_counter()
    p = subprocess.run([cli, os.path.join(workdir, "db"), str(P), "statistics", "-timing"] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=900)
    wall = time.perf_counter() - t0
    if p.returncode != 0:
        return {"error": p.stderr[-1000:]}
    m = re.search(r"phases ms: parse ([\d.e+]+), content statistics ([\d.e+]+), all ([\d.e+]+) \((\d+) chunks; buckets shrunk (\d+), removed (\d+)\)", p.stderr)
    out = {"wall_s": round(wall, 3)}
    if m:
        out.update(parse_ms=float(m.group(1)), content_stats_add_ms=float(m.group(2)), pass_ms=float(m.group(3)), chunks=int(m.group(4)),
                   buckets_shrunk=int(m.group(5)), buckets_removed=int(m.group(6)))
    block = [l for l in p.stdout.split("\n") if l.startswith(("buckets ", "bucket size   ", "features ", "locations "))]
    out["content"] = block
    return out


def stream_load(workdir, P, chunk):
    import torch
    eng = importlib.import_module("metacache-mpi_amd.engine")
    host = importlib.import_module("metacache-mpi_amd.host")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rdb = host.RefDb(os.path.join(workdir, "db"), P, meta_only=True)
    i = rdb.info
    pb = eng.PartsBuilder(rdb.tgt_windows(), k=i.k, sketch_size=i.q_sketch_size, winlen=i.q_winlen, winstride=i.q_winstride,
                          tgt_winstride=i.winstride, expected_locations=i.n_locs)
    t_parse = 0.0
    for rk in range(P):
        it = iter(rdb.stream(rk, chunk))
        while True:
            t1 = time.perf_counter()
            try:
                f, t, w = next(it)
            except StopIteration:
                break
            t_parse += time.perf_counter() - t1
            pb.add(f, t, w)
    parts = pb.finish()
    t2t = rdb.tgt2tax(4)
    db = parts.database(t2t.ctypes.data, n_shards=1, shard_id=0, device_ptrs=False)
    parts.close()
    torch.cuda.synchronize()
    s = time.perf_counter() - t0
    db.close()
    return {"load_s": round(s, 3), "of_it_record_parsing_s": round(t_parse, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--species", type=int, default=50)
    ap.add_argument("--strains", type=int, default=10)
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--batch", type=int, default=1 << 10)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--rule-n", type=int, default=8)
    ap.add_argument("--workdir", default="/tmp/mcq_info_rate")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "info_rate.json"))
    a = ap.parse_args()
    import torch
    import tuned_load_rate as tl
    pkg = importlib.import_module("metacache-mpi_amd")          # (built before: __graft_entry__.build())
    eng = importlib.import_module("metacache-mpi_amd.engine")
    host = importlib.import_module("metacache-mpi_amd.host")
    synth = importlib.import_module("metacache-mpi_amd.synth")
    shutil.rmtree(a.workdir, ignore_errors=True)
    os.makedirs(a.workdir)
    res = {"table": "%d species x %d strains" % (a.species, a.strains), "reference_ranks": a.ranks, "chunk_locations": tl.CHUNK}
    res.update(tl.write_shards(a, eng, host, synth, torch, torch.device("cuda", 0)))
    torch.cuda.empty_cache()
    cli = pkg.info_cli_path()
    res["statistics"] = [run_info(cli, a.workdir, a.ranks, []) for _ in range(a.runs)]
    res["statistics_with_rule"] = {"options": "-max-locations-per-feature %d" % a.rule_n,
                                   "runs": [run_info(cli, a.workdir, a.ranks, ["-max-locations-per-feature", str(a.rule_n)]) for _ in range(a.runs)]}
    res["streaming_load"] = [stream_load(a.workdir, a.ranks, tl.CHUNK) for _ in range(a.runs)]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))
    shutil.rmtree(a.workdir, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
