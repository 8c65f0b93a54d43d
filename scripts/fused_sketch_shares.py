#!/usr/bin/env python3
"""Which path wave_sketch_two_windows (csrc/mcq_device.hpp) takes per read, restated in NumPy on the CPU: reads drawn like the
benchmark's configs[1] (150 bp, 0.5 % substitutions, 0.1 % N, half reverse-complemented) from genomes of the benchmark's generator
(a small set: the shares depend on the reads' hashes, not on the table), window A's hashes as the kernel computes them, and for a
range of E (MCQ_SKETCH_EXPECT_FUSED) the share of reads that end in the one-sort pass, in the 64-lane sort and in the exact
selection.  No GPU needed.   python3 scripts/fused_sketch_shares.py [reads, default 65536] [read length, default 150]"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
synth = importlib.import_module("metacache-mpi_amd.synth")
n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 16
L = int(sys.argv[2]) if len(sys.argv) > 2 else 150
assert 129 <= L <= 160
dev = torch.device("cpu")
gb, goff, _ = synth.make_genomes(5, 2, 200_000, 400_000, 0.02, seed=3, device=dev)
reads, _, _ = synth.sample_reads(gb, goff, n_reads, L, 0.005, 0.001, seed=1000)
r = reads.numpy().reshape(n_reads, L)

code = np.full(256, 4, np.uint8)
for i, ch in enumerate(b"ACGT"):
    code[ch] = i; code[ch | 0x20] = i
c = code[r[:, :128]]                                     # window A
amb = (c == 4)
c = np.where(amb, 0, c).astype(np.uint64)
kmer = np.zeros((n_reads, 113), np.uint64)
bad = np.zeros((n_reads, 113), bool)
for j in range(16):
    kmer = (kmer << np.uint64(2)) | c[:, j:j + 113]
    bad |= amb[:, j:j + 113]
kmer = kmer.astype(np.uint32)


def revcomp(s):
    s = ((s >> 2) & 0x33333333) | ((s & 0x33333333) << 2)
    s = ((s >> 4) & 0x0F0F0F0F) | ((s & 0x0F0F0F0F) << 4)
    s = s.byteswap()
    return np.uint32(0xFFFFFFFF) - s


def tmh(x):
    x = ((x >> 16) ^ x) * np.uint32(0x45d9f3b)
    x = ((x >> 16) ^ x) * np.uint32(0x45d9f3b)
    return (x >> 16) ^ x


h = tmh(np.minimum(kmer, revcomp(kmer)))
h = np.where(bad, np.uint32(0xFFFFFFFF), h)
cA = (~bad).sum(1)
hs = np.sort(h, axis=1)
print("%d reads of %d bases; window A has 113 valid k-mers in %.1f %% of them" % (n_reads, L, 100.0 * (cA == 113).mean()))
print("  E   one sort   64-lane sort   exact selection   (%)")
for E in range(21, 29):
    with np.errstate(divide="ignore"):
        thr = np.minimum(np.float32(1) / cA.astype(np.float32) * np.float32(4294967296.0 * E), np.float32(4294967040.0))
    thr = np.where(cA <= 32, 0xFFFFFFFF, thr.astype(np.uint64)).astype(np.uint64)
    below = hs.astype(np.uint64) < thr[:, None]
    cnt = below.sum(1)
    first = np.ones_like(below); first[:, 1:] = hs[:, 1:] != hs[:, :-1]
    D = (below & first).sum(1)
    enough = (cA <= 32) | (D >= 16)
    one = (cnt <= 32) & enough
    wide = (cnt > 32) & (cnt <= 64) & enough
    exact = ~one & ~wide
    print(" %2d   %7.2f   %12.2f   %15.2f" % (E, 100.0 * one.mean(), 100.0 * wide.mean(), 100.0 * exact.mean()))
