"""Builds csrc/ into libmcq_hip.so (in-tree, so it travels with gpurun snapshots)."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

_HERE = os.path.dirname(os.path.abspath(__file__))
_HDR = os.path.join(os.path.dirname(_HERE), "include", "mcq.h")
_CSRC = os.path.join(_HERE, "csrc")
_INTERNAL = [os.path.join(_CSRC, h) for h in ("mcq_internal.hpp", "mcq_device.hpp", "mcq_classify.hpp")] + [_HDR]
# translation unit -> what it depends on besides itself; the library is linked in this order
_UNITS = {
    os.path.join(_CSRC, "mcq_engine.hip"): _INTERNAL,      # workspace, fused query, reduce
    os.path.join(_CSRC, "mcq_table.hip"): _INTERNAL,       # mcq_db_*
    os.path.join(_CSRC, "mcq_stages.hip"): _INTERNAL,      # staged and routing entry points, batch preparation
    os.path.join(_CSRC, "mcq_shard.hip"): _INTERNAL,       # mcq_shard_*
    os.path.join(_CSRC, "mcq_target_hits.hip"): _INTERNAL, # per-target window hit lists (-hits-per-seq)
    os.path.join(_CSRC, "mcq_align.hip"): _INTERNAL,       # read-to-candidate alignment (-align)
    os.path.join(_CSRC, "mcq_all_hits.hip"): _INTERNAL,    # all hits of a read, run-length compressed (-allhits)
    os.path.join(_CSRC, "mcq_coverage.hip"): _INTERNAL,    # window coverage per reference sequence over a run (mcq_coverage_*: -coverage, -cov-percentile)
    os.path.join(_CSRC, "mcq_accmap.hip"): _INTERNAL,      # *.accession2taxid text joined against the targets' names (mcq_accmap_*)
    os.path.join(_CSRC, "mcq_merge.hip"): _INTERNAL + [os.path.join(_CSRC, "mcq_classify_one.hpp")],   # merge of query result files (mcq_merge_*)
    os.path.join(_CSRC, "mcq_bucket_limit.hip"): _INTERNAL,   # the query-time bucket rules on a chunk of triples (mcq_bucket_limit)
    os.path.join(_CSRC, "mcq_content_stats.hip"): _INTERNAL,  # bucket size statistics and locations per target over chunks of triples (mcq_content_stats_*)
    os.path.join(_CSRC, "mcq_build.hip"): [_HDR],          # table construction (rocPRIM sorts)
    os.path.join(_CSRC, "mcq_classify.hip"): [os.path.join(_CSRC, h) for h in ("mcq_classify.hpp", "mcq_classify_one.hpp")] + [_HDR],   # classification + taxon counts
}
_OBJ = os.path.join(_HERE, "csrc", "_obj")


def lib_path():
    """MCQ_HIP_LIB (tuning knob): another build of the library, e.g. a variant for a same-box A/B (scripts/ab_libs.sh)"""
    return os.environ.get("MCQ_HIP_LIB") or os.path.join(_HERE, "libmcq_hip.so")


def host_lib_path():
    return os.path.join(_HERE, "libmcq_host.so")


def cli_path():
    return os.path.join(_HERE, "mcq_query_cli")


def build_cli_path():
    return os.path.join(_HERE, "mcq_build_cli")


def merge_cli_path():
    return os.path.join(_HERE, "mcq_merge_cli")


def info_cli_path():
    return os.path.join(_HERE, "mcq_info_cli")


def annotate_cli_path():
    return os.path.join(_HERE, "mcq_annotate_cli")


def mpi_cli_path():
    """mcq_query_mpi (one process per GPU under mpiexec); built only where an MPI is installed (/opt/conda: MPICH)"""
    return os.path.join(_HERE, "mcq_query_mpi")


_MPI_ROOT = os.environ.get("MCQ_MPI_ROOT", "/opt/conda")
_MPI_LIBS = ["libmpi.so.12", "libgfortran.so.4", "libquadmath.so.0", "libgomp.so.1"]


def mpi_lib_dir():
    """private directory with links to libmpi and what it needs, so that conda's old libstdc++ is not picked up at run time"""
    return os.path.join(_HERE, "_mpilib")


def source_digest():
    """sha256 (first 16 hex digits) over the kernel sources: profiles taken from one state of the kernels (PMC traffic,
    profiles/pmc_traffic_*.json) carry it, and bench.py refuses to quote them for another"""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(os.listdir(os.path.join(_HERE, "csrc"))):
        if f.endswith((".hip", ".hpp")):
            with open(os.path.join(_HERE, "csrc", f), "rb") as fh:
                h.update(f.encode()); h.update(fh.read())
    return h.hexdigest()[:16]


def build_host(force=False, verbose=False):
    """libmcq_host.so (shard reader and writer, taxonomy, classify, build inputs; g++, no GPU) and the
    mcq_query_cli, mcq_build_cli, mcq_merge_cli, mcq_info_cli and mcq_annotate_cli binaries (they link both libraries)."""
    srcs = [os.path.join(_HERE, "csrc", "host", f) for f in ("mcq_host.cpp", "mcq_host_build.cpp", "mcq_host_merge.cpp")]     # query side, build side, merge side
    hdr = os.path.join(os.path.dirname(_HERE), "include", "mcq_host.h")
    out = host_lib_path()
    if force or not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in srcs + [hdr, os.path.join(_HERE, "csrc", "host", "mcq_host_internal.hpp")]):
        cmd = ["g++", "-std=c++14", "-O2", "-ffp-contract=off", "-Wall", "-shared", "-fPIC"] + srcs + ["-o", out]   # (no contraction: the abundance estimate is float arithmetic restated op for op)
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    cli_src = os.path.join(_HERE, "csrc", "host", "mcq_query_cli.cpp")
    cli = cli_path()
    # what both programs depend on besides their own source: the two libraries and every header they include
    shared = [out, lib_path(), _HDR, hdr, os.path.join(os.path.dirname(_HERE), "include", "mcq_open.hpp")] + \
             [os.path.join(_HERE, "csrc", "host", h) for h in ("mcq_cli_common.hpp", "mcq_cli_buffers.hpp", "mcq_read_unit.hpp")]
    cli_deps = shared + [cli_src] + [os.path.join(_HERE, "csrc", "host", h) for h in ("mcq_read_batches.hpp", "mcq_align_subjects.hpp")]
    if force or not os.path.exists(cli) or os.path.getmtime(cli) < max(os.path.getmtime(f) for f in cli_deps):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        cmd = [hipcc, "-std=c++14", "-O2", "-pthread", cli_src, "-o", cli, "-L" + _HERE, "-lmcq_hip", "-lmcq_host", "-Wl,-rpath,$ORIGIN"]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    # mcq_build_cli: genome files + taxonomy dump -> the reference's shard files
    bcli_src = os.path.join(_HERE, "csrc", "host", "mcq_build_cli.cpp")
    bcli = build_cli_path()
    if force or not os.path.exists(bcli) or os.path.getmtime(bcli) < max(os.path.getmtime(f) for f in shared + [bcli_src]):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        cmd = [hipcc, "-std=c++14", "-O2", "-pthread", bcli_src, "-o", bcli, "-L" + _HERE, "-lmcq_hip", "-lmcq_host", "-Wl,-rpath,$ORIGIN"]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    # mcq_merge_cli: result files of several databases -> one classification per read
    mcli_src = os.path.join(_HERE, "csrc", "host", "mcq_merge_cli.cpp")
    mcli = merge_cli_path()
    if force or not os.path.exists(mcli) or os.path.getmtime(mcli) < max(os.path.getmtime(f) for f in shared + [mcli_src]):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        cmd = [hipcc, "-std=c++14", "-O2", "-pthread", mcli_src, "-o", mcli, "-L" + _HERE, "-lmcq_hip", "-lmcq_host", "-Wl,-rpath,$ORIGIN"]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    # mcq_info_cli: what a database was built with, what it holds, how full its buckets are
    icli_src = os.path.join(_HERE, "csrc", "host", "mcq_info_cli.cpp")
    icli = info_cli_path()
    icli_deps = [out, lib_path(), _HDR, hdr, os.path.join(os.path.dirname(_HERE), "include", "mcq_open.hpp"),
                 os.path.join(_HERE, "csrc", "host", "mcq_cli_buffers.hpp"), icli_src]
    if force or not os.path.exists(icli) or os.path.getmtime(icli) < max(os.path.getmtime(f) for f in icli_deps):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        cmd = [hipcc, "-std=c++14", "-O2", "-ffp-contract=off", "-pthread", icli_src, "-o", icli, "-L" + _HERE, "-lmcq_hip", "-lmcq_host",
               "-Wl,-rpath,$ORIGIN"]     # (no contraction: the moments are the reference's double arithmetic restated op for op)
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    # mcq_annotate_cli: taxid|N into the headers of genome files, from *.accession2taxid files
    acli_src = os.path.join(_HERE, "csrc", "host", "mcq_annotate_cli.cpp")
    acli = annotate_cli_path()
    acli_deps = [out, lib_path(), _HDR, hdr, os.path.join(_HERE, "csrc", "host", "mcq_cli_buffers.hpp"), acli_src]
    if force or not os.path.exists(acli) or os.path.getmtime(acli) < max(os.path.getmtime(f) for f in acli_deps):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        cmd = [hipcc, "-std=c++14", "-O2", "-pthread", acli_src, "-o", acli, "-L" + _HERE, "-lmcq_hip", "-lmcq_host", "-Wl,-rpath,$ORIGIN"]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    # the MPI program (multi-GPU host in C++): only where an MPI is installed
    mpi_src = os.path.join(_HERE, "csrc", "host", "mcq_query_mpi.cpp")
    mpi_h = os.path.join(_MPI_ROOT, "include", "mpi.h")
    mpi_so = os.path.join(_MPI_ROOT, "lib", _MPI_LIBS[0])
    if os.path.exists(mpi_h) and os.path.exists(mpi_so):
        os.makedirs(mpi_lib_dir(), exist_ok=True)
        for l in _MPI_LIBS:
            dst = os.path.join(mpi_lib_dir(), l)
            if not os.path.lexists(dst) and os.path.exists(os.path.join(_MPI_ROOT, "lib", l)):
                os.symlink(os.path.join(_MPI_ROOT, "lib", l), dst)
        mpi_cli = mpi_cli_path()
        newest = max(os.path.getmtime(f) for f in shared + [mpi_src])
        if force or not os.path.exists(mpi_cli) or os.path.getmtime(mpi_cli) < newest:
            rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
            # plain g++ (host code only; hipcc would take libmpi.so.12 for a source file)
            cmd = ["g++", "-std=c++14", "-O2", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(_MPI_ROOT, "include"),
                   mpi_src, "-o", mpi_cli, "-L" + _HERE, "-lmcq_hip", "-lmcq_host", "-L" + os.path.join(rocm, "lib"), "-lamdhip64", mpi_so,
                   "-Wl,-rpath-link," + os.path.join(_MPI_ROOT, "lib"), "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,$ORIGIN/_mpilib",
                   "-Wl,-rpath," + os.path.join(rocm, "lib")]
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd)
    return out


def build_hip(force=False, verbose=False):
    """hipcc every stale unit of csrc/ for gfx950 into csrc/_obj/*.o, link libmcq_hip.so"""
    if os.environ.get("MCQ_HIP_LIB"):          # a prebuilt variant was asked for: nothing to build
        return lib_path()
    out = lib_path()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(_OBJ, exist_ok=True)
    extra = os.environ.get("MCQ_HIPCC_FLAGS", "").split()      # tuning experiments, e.g. -DMCQ_WAVE_OCC=7
    force = force or bool(extra)
    objs, stale, relink = [], [], force or not os.path.exists(out)
    for src, deps in _UNITS.items():
        obj = os.path.join(_OBJ, os.path.basename(src) + ".o")
        objs.append(obj)
        newest = max(os.path.getmtime(f) for f in [src] + deps)
        if force or not os.path.exists(obj) or os.path.getmtime(obj) < newest:
            stale.append([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"] + extra + ["-c", src, "-o", obj])
        elif os.path.exists(out) and os.path.getmtime(out) < os.path.getmtime(obj):
            relink = True
    if stale:       # the stale units side by side, each in its own compiler process
        relink = True
        if verbose:
            for cmd in stale:
                print(" ".join(cmd))
        jobs = min(len(stale), int(os.environ.get("MAX_JOBS", 16)), 16)
        with ThreadPoolExecutor(jobs) as pool:
            list(pool.map(subprocess.check_call, stale))
    if relink:
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", out, "-ldl"]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    return out
