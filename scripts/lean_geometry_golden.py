#!/usr/bin/env python3
"""tests/golden/lean_geometry_parent_stats.json: mcq_stats of the lean first wave stage on the first batch of
tests/test_gpu_lean_geometry.py, recorded from the library MCQ_HIP_LIB names -- a build of the commit BEFORE the lean form was
compiled for the default geometry.  MCQ_HIP_LIB=/path/to/parent/libmcq_hip.so python3 scripts/lean_geometry_golden.py [OUT]"""
import importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
t = importlib.import_module("test_gpu_lean_geometry")
eng = importlib.import_module("metacache-mpi_amd.engine")
dbbuild = importlib.import_module("dbbuild_torch")
synth = importlib.import_module("metacache-mpi_amd.synth")
print("library", importlib.import_module("metacache-mpi_amd.build").lib_path())
dev = torch.device("cuda", 0)
gb, goff, species = synth.make_genomes(6, 4, 150_000, 300_000, 0.02, seed=31, device=dev)
keys, off, locs, _ = dbbuild.build_table(gb, goff, emulate_ranks=2)
db = dbbuild.make_database(keys, off, locs, species)
rb, ro = t.boundary_reads(synth, gb, goff, t.NQ, seed=71)
ws = eng.Workspace(db, t.NQ, len(rb) + 64)
out = {}
for name, qf in (("lean", eng.MCQ_FORCE_LEAN_WAVE), ("full", eng.MCQ_FORCE_FULL_WAVE)):
    c, n = ws.query_host(rb, ro, False, max_cand=t.M, emulate_ranks=t.P, flags=qf)
    out[name] = ws.sync()
    print(name, out[name])
g = {k: out["lean"][k] for k in t.STATS}
g["_source"] = "scripts/lean_geometry_golden.py: the parent commit's library, MCQ_FORCE_LEAN_WAVE, boundary_reads(seed 71), P 2, M 2"
json.dump(g, open(sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN, "w"), indent=1)
print(json.dumps(g))
