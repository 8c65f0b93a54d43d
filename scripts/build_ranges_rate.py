#!/usr/bin/env python3
"""mcq_build_cli in feature ranges against its one-piece route, on the genome set of bench.py's table (run on the GPU box from the
repo root).

The inputs are those of scripts/build_cli_rate.py (50 species x 10 strains, 2 Gbp, seed 3, one FASTA file per genome, a dump of
root > Bacteria > species), read once into the page cache.  The program runs three ways -- no option (the one-piece route: the
yardstick of the session), `-ranges 1`, `-ranges 4` -- alternating, --runs times each, every run a child process under `timeout`.
Per run: the wall time, the program's phases (MCQ_BUILD_TRACE=1), the peak RSS (os.wait4 of the child) and the device memory:
hipMemGetInfo's free bytes before and after the run and the least seen while it ran (polled from this process every 50 ms; the
difference to "before" is the program's peak on the device).  The files of the three ways are compared: `-ranges 1` byte for byte
with the default run's, `-ranges 4` by size.  Writes profiles/build_ranges_rate.json, or the file --out names: medians per way
and the ratios to the default run.  No rate is set in advance.
"""
import argparse
import filecmp
import importlib
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from build_cli_rate import CHILD, write_inputs      # noqa: E402

WAYS = (("default", []), ("ranges_1", ["-ranges", "1"]), ("ranges_4", ["-ranges", "4"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--species", type=int, default=50)
    ap.add_argument("--strains", type=int, default=10)
    ap.add_argument("--genome-min", type=int, default=3_000_000)
    ap.add_argument("--genome-max", type=int, default=5_000_000)
    ap.add_argument("--divergence", type=float, default=0.02)
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per run of the program")
    ap.add_argument("--workdir", default="/tmp/mcq_build_ranges_rate")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "build_ranges_rate.json"))
    a = ap.parse_args()

    import torch
    pkg = importlib.import_module("metacache-mpi_amd")
    pkg.build_hip(); pkg.build_host()
    synth = importlib.import_module("metacache-mpi_amd.synth")
    dev = torch.device("cuda", 0)
    P = a.ranks
    shutil.rmtree(a.workdir, ignore_errors=True)
    os.makedirs(a.workdir)
    gb, goff, species = synth.make_genomes(a.species, a.strains, a.genome_min, a.genome_max, a.divergence, seed=3, device=dev)
    write_inputs(a, gb, goff, species)
    res = {"table": "%d species x %d strains" % (a.species, a.strains), "targets": int(goff.numel() - 1), "db_bp": int(goff[-1]), "ranks": P,
           "device": torch.cuda.get_device_name(0), "fasta_bytes": 0}
    del gb, goff, species
    torch.cuda.empty_cache()
    for f in sorted(os.listdir(os.path.join(a.workdir, "genomes"))):          # once into the page cache
        with open(os.path.join(a.workdir, "genomes", f), "rb") as fh:
            while True:
                b = fh.read(1 << 24)
                if not b:
                    break
                res["fasta_bytes"] += len(b)

    runs = {name: [] for name, _ in WAYS}
    for i in range(a.runs):
        for name, extra in WAYS:
            err = os.path.join(a.workdir, "stderr_%s_%d.txt" % (name, i))
            free_before = torch.cuda.mem_get_info(0)[0]
            least, stop = [free_before], threading.Event()

            def poll():
                while not stop.is_set():
                    least[0] = min(least[0], torch.cuda.mem_get_info(0)[0])
                    stop.wait(0.05)
            th = threading.Thread(target=poll)
            th.start()
            r = subprocess.run([sys.executable, "-c", CHILD, err, "timeout", "-k", "10", str(a.timeout), pkg.build_cli_path(), name, str(P), "genomes",
                                "-taxonomy", "tax"] + extra, cwd=a.workdir, env=dict(os.environ, MCQ_BUILD_TRACE="1"), stdout=subprocess.PIPE, text=True)
            stop.set(); th.join()
            free_after = torch.cuda.mem_get_info(0)[0]
            rc, rss, wall = json.loads(r.stdout)
            text = open(err).read()
            if rc != 0:
                print(text[-3000:]); sys.exit("mcq_build_cli %s failed (status %d)" % (" ".join(extra), rc))     # nothing more is started on the GPU
            ph = {m.group(1).strip(): float(m.group(2)) for m in re.finditer(r"^\[mcq_build_cli\] (.+?)\s+([0-9.]+) s$", text, flags=re.M)}
            runs[name].append({"wall_s": round(wall, 3), "peak_rss_bytes": rss, "phases_s": ph, "device_free_before_bytes": free_before,
                               "device_free_least_bytes": least[0], "device_free_after_bytes": free_after,
                               "device_peak_bytes": free_before - least[0]})
            print("run %d %-9s %.2f s" % (i, name, wall), flush=True)
    res["runs"] = runs
    med = {}
    for name, _ in WAYS:
        rs = runs[name]
        phases = sorted({k for x in rs for k in x["phases_s"]})
        med[name] = {"wall_s": round(statistics.median(x["wall_s"] for x in rs), 3),
                     "peak_rss_bytes": int(statistics.median(x["peak_rss_bytes"] for x in rs)),
                     "device_peak_bytes": int(statistics.median(x["device_peak_bytes"] for x in rs)),
                     "phases_s": {k: round(statistics.median(x["phases_s"].get(k, 0.0) for x in rs), 3) for k in phases}}
    res["median"] = med
    res["ratio_to_default"] = {name: {k: round(med[name][k] / med["default"][k], 3) for k in ("wall_s", "peak_rss_bytes", "device_peak_bytes")
                                      if med["default"][k]} for name, _ in WAYS[1:]}
    files = {name: [os.path.join(a.workdir, "%s.db_%d" % (name, r)) for r in range(P)] for name, _ in WAYS}
    res["shard_file_bytes"] = {name: [os.path.getsize(p) for p in files[name]] for name in files}
    res["ranges_1_files_identical_to_default"] = all(filecmp.cmp(x, y, shallow=False) for x, y in zip(files["default"], files["ranges_1"]))
    res["ranges_4_files_same_size_as_default"] = res["shard_file_bytes"]["ranges_4"] == res["shard_file_bytes"]["default"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}, indent=1))
    shutil.rmtree(a.workdir, ignore_errors=True)


if __name__ == "__main__":
    main()
