"""mcq_query_cli's input stage on the GPU: mcq_reads_prepare (one chunk of FASTQ / FASTA text per file -> the compacted batch,
header ranges and cut points) against the host parser, which tests/test_host_read_stream.py checks against the whole-file
reader; mcq_query on the prepared buffers; the CLI's -out file under chunk boundaries everywhere, both readers and any
-threads; and host memory bounded by the options, not by the input."""
import gzip
import importlib
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from golden_util import Fixture
from oracle import dbfile
from read_corpus import corpus, read_records
from reads_device import _check_chunk, _device_prepare

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    pkg = importlib.import_module("metacache-mpi_amd")
    pkg.build_host()
    return pkg, importlib.import_module("metacache-mpi_amd.engine"), importlib.import_module("metacache-mpi_amd.host")


def _write(tmp_path, files):
    paths = []
    for i, data in enumerate(files):
        p = tmp_path / ("r%d.fq" % (i + 1))
        p.write_bytes(data)
        paths.append(p)
    return paths


@pytest.mark.parametrize("name", sorted(corpus()))
def test_device_prepare_equals_the_host_parser(mods, name, tmp_path):
    """every chunk at several chunk sizes: sequences, mate interleave, header ranges, cut points and counts equal the host
    parser's; no chunk of a strict file is flagged, and a file that is not strict is flagged where it is not"""
    pkg, eng, host = mods
    dev = torch.device("cuda", 0)
    files, strict = corpus()[name]
    paths = _write(tmp_path, files)
    exp = [tuple(r[q][:2] for r in (read_records(f) for f in files)) for q in range(min(len(read_records(f)) for f in files))]
    for chunk in (1, 37, 97, 300, 4096, 1 << 20):
        seen = {"flagged": 0, "clean": 0}
        got = []
        prep = lambda t, f, mq, mb: _check_chunk(host, eng, dev, t, f, mq, mb, seen)
        for texts, info, bases, seq_off, hdr, _ in host.read_batches(paths, chunk, prepare=prep):
            n, mates = int(info[host.READS_N]), len(texts)
            for q in range(n):
                seqs = [bytes(bases[int(seq_off[q * mates + m]):int(seq_off[q * mates + m + 1])]) for m in range(mates)]
                got.append((texts[0][int(hdr[2 * q]):int(hdr[2 * q + 1])], seqs))
        assert [(g[0], g[1][0]) for g in got] == [(e[0][0], e[0][1]) for e in exp], (name, chunk)
        assert [g[1][1:] for g in got] == [[x[1] for x in e[1:]] for e in exp], (name, chunk)
        if strict:
            assert seen["flagged"] == 0, (name, chunk, seen)
        else:
            assert seen["flagged"] > 0, (name, chunk, seen)


@pytest.mark.parametrize("name", ["fq_lf", "fa_wrap60", "paired_fq", "paired_fa_fq", "long_record_fa", "fq_crlf"])
@pytest.mark.parametrize("max_q,max_b", [(1, 1 << 62), (3, 1 << 62), (1 << 40, 150), (4, 400), (1 << 40, 1), (7, 1000)])
def test_device_prepare_applies_the_batch_limits(mods, name, max_q, max_b):
    """max_queries / max_bases on a whole file in one chunk, aligned and unaligned: n, the bases, the cut points and the
    outputs equal the host parser's, including a single query over max_bases taken alone"""
    pkg, eng, host = mods
    dev = torch.device("cuda", 0)
    files, _ = corpus()[name]
    for shift in (0, 3):
        for flags in (0, host.READS_EOF1 | host.READS_EOF2):
            seen = {"flagged": 0, "clean": 0}
            info = _check_chunk(host, eng, dev, files, flags, max_q, max_b, seen, shift)[0]
            assert seen["clean"] == 1
            n = int(info[host.READS_N])
            assert 1 <= n <= max_q
            assert int(info[host.READS_BASES]) <= max_b or n == 1


def _reads_text(names, seqs, fmt):
    if fmt == "fastq":
        return "".join("@%s extra\n%s\n+\n%s\n" % (n, s, "I" * len(s)) for n, s in zip(names, seqs)).encode()
    return "".join(">%s extra\n%s" % (n, "".join(s[k:k + 60] + "\n" for k in range(0, len(s), 60))) for n, s in zip(names, seqs)).encode()


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
@pytest.mark.parametrize("P,M", [(1, 3), (2, 2)])
def test_query_on_prepared_buffers_equals_a_host_batch(mods, paired, fmt, P, M):
    from oracle import mc_oracle as orc
    pkg, eng, host = mods
    dev = torch.device("cuda", 0)
    fx = Fixture("mini", 2)
    keys, off, locs = dbfile.union_shards(fx.shards)
    p = fx.params
    db = eng.Database(keys, off, locs, fx.tgt2tax(), k=p["qk"], sketch_size=p["qs"], winlen=p["qwinlen"],
                      winstride=p["qwinstride"], tgt_winstride=p["winstride"])
    texts = [_reads_text(fx.names, fx.r1, fmt)] + ([_reads_text(fx.names, fx.r2, fmt)] if paired else [])
    nq = len(fx.names)
    info, bases, seq_off, hdr, qcap = _device_prepare(eng, dev, texts, host.READS_EOF1 | host.READS_EOF2, nq, 1 << 40)
    assert int(info[host.READS_N]) == nq and int(info[host.READS_STATUS]) == 0
    mates = 2 if paired else 1
    d_bases = torch.from_numpy(bases.copy()).to(dev)
    d_off = torch.from_numpy(seq_off.view(np.int64).copy()).to(dev)
    cands = torch.zeros((nq, M, 4), dtype=torch.int32, device=dev)
    ncand = torch.zeros(nq, dtype=torch.int32, device=dev)
    seqs = [s for ab in zip(fx.r1, fx.r2) for s in ab] if paired else list(fx.r1)
    hb, hso = orc.pack_reads(seqs)
    ws = eng.Workspace(db, nq, max(len(hb), 1))
    ws.query_device(d_bases.data_ptr(), d_off.data_ptr(), nq * mates, paired, cands.data_ptr(), ncand.data_ptr(), max_cand=M,
                    emulate_ranks=P, flags=eng.MCQ_QUIRK_SEQ_DROP, stream=torch.cuda.current_stream(dev).cuda_stream)
    ws.sync()
    hc, hn = ws.query_host(hb, hso, paired, max_cand=M, emulate_ranks=P, flags=eng.MCQ_QUIRK_SEQ_DROP)
    gn = ncand.cpu().numpy().view(np.uint32); gc = cands.cpu().numpy().view(np.uint32)
    assert np.array_equal(gn, hn)
    mask = np.arange(M)[None, :] < hn[:, None]
    assert np.array_equal(gc[mask], hc[mask])
    assert seq_off[: nq * mates + 1].tolist() == [int(x) for x in hso]


VARIANTS = {"default": [], "tophits": ["-tophits"], "lineage": ["-tophits", "-taxids", "-lineage"],
            "idsonly": ["-tophits", "-taxids-only", "-omit-ranks", "-mapped-only"]}


def _mask(text, threads_too=False):
    text = re.sub(r"^# time:    .*$", "# time:    T ms", text, flags=re.M)
    text = re.sub(r"^# speed:   .*$", "# speed:   S queries/min", text, flags=re.M)
    if threads_too:
        text = re.sub(r"^# Using \d+ threads$", "# Using N threads", text, flags=re.M)
    return text


@pytest.mark.parametrize("tag,P", [("mini", 4), ("tie", 2)])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_cli_out_file_under_chunk_boundaries_readers_and_threads(mods, tag, P, variant, fmt, tmp_path):
    """the golden -out file of tests/test_gpu_cli.py (compared as it compares: sorted, time and speed masked) for every
    -read-chunk in {97, 4096, default} and -reader gpu|host, with the reads as FASTQ and as FASTA wrapped at 60 columns; and
    the mapping lines in input order: the same file unsorted for -threads 1, 2 and 7"""
    pkg, eng, host = mods
    fx = Fixture(tag, P)
    (tmp_path / "r1.fq").write_bytes(_reads_text(fx.names, fx.r1, fmt))
    (tmp_path / "r2.fq").write_bytes(_reads_text(fx.names, fx.r2, fmt))
    prefix = fx.shard_paths[0][: -len(".db_0")]
    with gzip.open(os.path.join(os.path.dirname(fx.shard_paths[0]), "cli_%s.out.gz" % variant), "rt") as f:
        ref = f.read()
    runs = [(c, r, 2) for c in (97, 4096, None) for r in ("gpu", "host")] + [(97, "gpu", 1), (97, "gpu", 7), (None, "host", 7), (4096, "gpu", 7)]
    first = None
    for i, (chunk, reader, threads) in enumerate(runs):
        out = "out%d.txt" % i
        cmd = [pkg.cli_path(), prefix, str(P), "r1.fq", "r2.fq", "-lowest", fx.q["lowest"], "-maxcand", str(fx.maxcand),
               "-hitmin", str(fx.hitmin), "-hitdiff", str(fx.q["hitdiff"]), "-threads", str(threads), "-out", out,
               "-reader", reader] + (["-read-chunk", str(chunk)] if chunk else []) + VARIANTS[variant]
        r = subprocess.run(cmd, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert r.returncode == 0, (chunk, reader, threads, r.stderr)
        mine = (tmp_path / out).read_text()
        if threads == 2:
            assert sorted(_mask(mine).split("\n")) == sorted(_mask(ref).split("\n")), (chunk, reader)
        m = _mask(mine, threads_too=True)
        if first is None:
            first = m
        assert m == first, (chunk, reader, threads)


def _write_synthetic_pairs(path1, path2, n, rng):
    """n pairs of 150 bp, random bases, headers q%08d_g3 synthetic read"""
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    qual = b"I" * 150
    for path in (path1, path2):
        with open(path, "wb") as f:
            for b0 in range(0, n, 65536):
                m = min(65536, n - b0)
                seqs = lut[rng.integers(0, 4, size=(m, 150))]
                f.write(b"".join(b"@q%08d_g3 synthetic read\n%s\n+\n%s\n" % (b0 + i, seqs[i].tobytes(), qual) for i in range(m)))


# os.wait4's ru_maxrss counts what the child held before its exec -- a fork of this process, pytest with torch -- so the
# program is started by a fresh small interpreter, which waits for it and reports its ru_maxrss
RSS_HELPER = ("import json, os, subprocess, sys\n"
              "p = subprocess.Popen(sys.argv[2:], stdout=subprocess.DEVNULL, stderr=open(sys.argv[1], 'wb'))\n"
              "_, status, ru = os.wait4(p.pid, 0)\n"
              "print(json.dumps([os.waitstatus_to_exitcode(status), ru.ru_maxrss * 1024]))\n")


def _run_rss(cmd, cwd):
    """exit status, peak RSS in bytes (os.wait4 of the child), stderr"""
    import json
    import sys
    err = os.path.join(cwd, "stderr.txt")
    r = subprocess.run([sys.executable, "-c", RSS_HELPER, err] + cmd, cwd=cwd, stdout=subprocess.PIPE, text=True, timeout=900)
    rc, peak = json.loads(r.stdout)
    with open(err) as f:
        return rc, peak, f.read()


def test_cli_host_memory_is_bounded_by_the_options(mods, tmp_path):
    """2^20 read pairs of 150 bp (2 x 349 MB of FASTQ) through mcq_query_cli -batch 32768: the peak RSS above that of the
    first 1024 pairs is at most 1/4 of the two files' bytes (the whole-file reader needed 0.8 of them)"""
    pkg, eng, host = mods
    fx = Fixture("mini", 4)
    prefix = fx.shard_paths[0][: -len(".db_0")]
    n = 1 << 20
    rng = np.random.default_rng(2020)
    big1, big2 = tmp_path / "b1.fq", tmp_path / "b2.fq"
    _write_synthetic_pairs(big1, big2, n, rng)
    small1, small2 = tmp_path / "s1.fq", tmp_path / "s2.fq"
    for src, dst in ((big1, small1), (big2, small2)):
        with open(src, "rb") as f:
            dst.write_bytes(b"".join(f.readline() for _ in range(4 * 1024)))
    total = os.path.getsize(big1) + os.path.getsize(big2)
    rss = {}
    for tag, (a, b) in (("small", (small1, small2)), ("big", (big1, big2))):
        out = tmp_path / ("%s.out" % tag)
        rc, peak, err = _run_rss([pkg.cli_path(), prefix, "4", str(a), str(b), "-lowest", fx.q["lowest"], "-maxcand", str(fx.maxcand),
                                  "-hitmin", str(fx.hitmin), "-hitdiff", str(fx.q["hitdiff"]), "-batch", "32768", "-out", str(out)], tmp_path)
        assert rc == 0, (tag, err[-2000:])
        rss[tag] = peak
        summary = [l for l in out.read_text().split("\n") if l.startswith("# queries: ")]
        assert summary == ["# queries: %d" % (2 * (n if tag == "big" else 1024))], summary
    print("peak RSS: small %.1f MB, big %.1f MB, files %.1f MB, growth / bytes %.3f"
          % (rss["small"] / 1e6, rss["big"] / 1e6, total / 1e6, (rss["big"] - rss["small"]) / total))
    assert rss["big"] - rss["small"] <= total / 4
