"""The input lists of the query programs on the GPU: several pairs of files (-pairfiles, names sorted and paired), an
interleaved file (-pairseq, parsed by mcq_reads_prepare with MCQ_READS_INTERLEAVED), a directory, and one output per unit
(-splitout).  Whatever way the reads of a fixture come in, their mapping lines, the summary and the abundance table must be
those of the one-pair run tests/test_gpu_cli.py compares with the reference's file; each unit's lines follow its own
"# f1 + f2" line, in input order."""
import importlib
import os
import re
import shutil
import subprocess

import pytest

from golden_util import Fixture

pytestmark = pytest.mark.gpu

GROUPS = ("c", "a", "b")            # the fixture's reads in three parts; their file names sort in another order than the reads


def _mask(text):
    text = re.sub(r"^# time:    .*$", "# time:    T ms", text, flags=re.M)
    return re.sub(r"^# speed:   .*$", "# speed:   S queries/min", text, flags=re.M)


class Case:
    """a fixture's reads as files in a directory of their own, and what every run is compared with: the one-pair run"""

    def __init__(self, tag, P, root):
        self.pkg = importlib.import_module("metacache-mpi_amd")
        self.pkg.build_host()
        self.fx = fx = Fixture(tag, P)
        self.P, self.root = P, root
        self.prefix = fx.shard_paths[0][: -len(".db_0")]
        n = len(fx.names)
        self.part = {g: range(n * i // 3, n * (i + 1) // 3) for i, g in enumerate(GROUPS)}
        self._fastq("r1.fq", fx.r1, range(n)); self._fastq("r2.fq", fx.r2, range(n))
        os.mkdir(os.path.join(root, "lanes"))
        for g in GROUPS:
            self._fastq("%s_1.fq" % g, fx.r1, self.part[g]); self._fastq("%s_2.fq" % g, fx.r2, self.part[g])
            for m in "12":
                shutil.copy(os.path.join(root, "%s_%s.fq" % (g, m)), os.path.join(root, "lanes"))
        with open(os.path.join(root, "il.fq"), "w") as f:
            for q in range(n):
                f.write("@%s\n%s\n+\n%s\n@%s/2\n%s\n+\n%s\n" % (fx.names[q], fx.r1[q], "I" * len(fx.r1[q]), fx.names[q], fx.r2[q], "I" * len(fx.r2[q])))
        self.base = self.parse(self.run(["r1.fq", "r2.fq"]))
        assert [u for u, _ in self.base[1]] == ["# r1.fq + r2.fq"] and len(self.base[1][0][1]) == n

    def _fastq(self, name, seqs, idx):
        with open(os.path.join(self.root, name), "w") as f:
            for q in idx:
                f.write("@%s\n%s\n+\n%s\n" % (self.fx.names[q], seqs[q], "I" * len(seqs[q])))

    def options(self):
        fx = self.fx
        return ["-lowest", fx.q["lowest"], "-maxcand", str(fx.maxcand), "-hitmin", str(fx.hitmin), "-hitdiff", str(fx.q["hitdiff"]),
                "-threads", "2", "-abundance-per", "species"]

    def run(self, inputs, extra=(), out="out.txt", program=None, env=None):
        """the program's -out file (or, with out=None, nothing)"""
        cmd = (program or [self.pkg.cli_path()]) + [self.prefix, str(self.P)] + list(inputs) + self.options() + list(extra) + (["-out", out] if out else [])
        r = subprocess.run(cmd, cwd=self.root, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert r.returncode == 0, (cmd, r.stdout[-1500:], r.stderr[-1500:])
        if out:
            with open(os.path.join(self.root, out)) as f:
                return _mask(f.read())

    def parse(self, text):
        """(head, [(unit line, mapping lines)], tail): the head up to TABLE_LAYOUT, the tail from the abundance table on"""
        lines = text.split("\n")
        at = next(i for i, l in enumerate(lines) if l.startswith("# TABLE_LAYOUT"))
        end = next(i for i, l in enumerate(lines) if l.startswith("# estimated abundance"))
        units = []
        for l in lines[at + 1:end]:
            if l.startswith("# "):
                units.append((l, []))
            else:
                assert l.split("\t|\t")[0] in self.fx.final, l
                units[-1][1].append(l)
        return lines[:at + 1], units, lines[end:]

    def lines_of(self, group):
        return [self.base[1][0][1][q] for q in self.part[group]]


_cases = {}


def _case(tag, P, tmp_path_factory):
    if (tag, P) not in _cases:
        _cases[(tag, P)] = Case(tag, P, str(tmp_path_factory.mktemp("inputs_" + tag)))
    return _cases[(tag, P)]


@pytest.fixture(scope="module", params=[("mini", 4), ("tie", 2)], ids=["mini-P4", "tie-P2"])
def case(request, tmp_path_factory):
    return _case(*request.param, tmp_path_factory)


SHUFFLED = ["b_2.fq", "c_1.fq", "a_2.fq", "b_1.fq", "a_1.fq", "c_2.fq"]


def _check_three_pairs(case, text):
    head, units, tail = case.parse(text)
    assert head == case.base[0] and tail == case.base[2]                       # parameter lines; abundance table and summary
    assert [u for u, _ in units] == ["# %s_1.fq + %s_2.fq" % (g, g) for g in sorted(GROUPS)]
    for g, (_, lines) in zip(sorted(GROUPS), units):
        assert lines == case.lines_of(g), g


@pytest.mark.parametrize("reader", ["gpu", "host"])
def test_three_pairs_of_files_given_out_of_order(case, reader):
    """-pairfiles sorts the names and pairs them; each "# a + b" line is followed by exactly that pair's mapping lines, and
    the lines, the summary and the abundance table are those of the one-pair run over all reads"""
    _check_three_pairs(case, case.run(SHUFFLED, ["-pairfiles", "-reader", reader, "-read-chunk", "4096"]))


def test_three_pairs_of_files_equal_the_references_out_file(tmp_path_factory):
    """the file the reference wrote for this command line under mpiexec -n 2 on `tie` (tests/golden/make_golden_inputs.py),
    byte for byte after sorting (its line order within a unit depends on its threads), time and speed masked, and its
    non-mapping lines in its order.  (`mini` at P = 4 has no such file: the reference's ranks write over each other's lines
    there, see the generator; its runs are pinned by the one-pair file, which the reference did write whole.)"""
    import gzip
    case = _case("tie", 2, tmp_path_factory)
    with gzip.open(os.path.join(os.path.dirname(case.fx.shard_paths[0]), "cli_inputs_three_pairs.out.gz"), "rt") as f:
        ref = _mask(f.read())
    mine = case.run(SHUFFLED, ["-pairfiles"])
    assert sorted(mine.split("\n")) == sorted(ref.split("\n"))
    assert [l for l in mine.split("\n") if l.startswith("#")] == [l for l in ref.split("\n") if l.startswith("#")]


def _mpi(case):
    """mcq_query_mpi at one rank (the RCCL path with a communicator of one), as tests/test_gpu_cli.py starts it"""
    mpiexec = shutil.which("mpiexec") or "/opt/conda/bin/mpiexec"
    if not os.path.exists(case.pkg.mpi_cli_path()) or not os.path.exists(mpiexec):
        pytest.skip("no MPI on this box")
    env = dict(os.environ, LD_LIBRARY_PATH=case.pkg.mpi_lib_dir() + ":" + os.environ.get("LD_LIBRARY_PATH", ""), HSA_ENABLE_IPC_MODE_LEGACY="0",
               MCQ_SHARD_FORCE_RCCL="1")
    return dict(program=[mpiexec, "-n", "1", case.pkg.mpi_cli_path()], env=env)


def test_three_pairs_of_files_through_the_mpi_program(case):
    _check_three_pairs(case, case.run(SHUFFLED, ["-pairfiles"], **_mpi(case)))


def test_interleaved_file_through_the_mpi_program(case):
    """... where the host parser pairs the records"""
    head, units, tail = case.parse(case.run(["il.fq"], ["-pairseq"], **_mpi(case)))
    assert [u for u, _ in units] == ["# il.fq"] and units[0][1] == case.base[1][0][1] and tail == case.base[2]


def test_interleaved_file(case):
    """-pairseq: the same mapping lines and tables as the two files of the same reads, whatever the chunk size; the head
    names the pairing mode as show_query_parameters does"""
    outs = [case.run(["il.fq"], ["-pairseq", "-read-chunk", str(c)]) for c in (97, 4096)]
    assert outs[0] == outs[1]
    assert outs[0] == case.run(["il.fq"], ["-pairseq", "-reader", "host"])
    head, units, tail = case.parse(outs[0])
    assert [u for u, _ in units] == ["# il.fq"]
    assert units[0][1] == case.base[1][0][1] and tail == case.base[2]
    files_mode = ["# File based paired-end mode:", "#   Reads from two consecutive files will be interleaved."]
    seq_mode = ["# Per file paired-end mode:", "#   Reads from two consecutive sequences in each file will be paired up."]
    assert [seq_mode[files_mode.index(l)] if l in files_mode else l for l in case.base[0]] == head and seq_mode[0] in head


def test_two_interleaved_files(case):
    """exactly two names with -pairseq are two interleaved units, not a pair of files"""
    with open(os.path.join(case.root, "il.fq")) as f:
        lines = f.read().split("\n")[:-1]
    cut = 8 * (len(case.fx.names) // 2)                            # 8 lines per pair
    for name, part in (("il_z.fq", lines[:cut]), ("il_a.fq", lines[cut:])):
        with open(os.path.join(case.root, name), "w") as f:
            f.write("".join(l + "\n" for l in part))
    head, units, tail = case.parse(case.run(["il_z.fq", "il_a.fq"], ["-pairseq", "-read-chunk", "4096"]))
    assert [u for u, _ in units] == ["# il_z.fq", "# il_a.fq"]
    assert units[0][1] + units[1][1] == case.base[1][0][1] and len(units[0][1]) == cut // 8 and tail == case.base[2]


def test_splitout_refuses_a_missing_file_before_anything_is_written(case):
    cmd = [case.pkg.cli_path(), case.prefix, str(case.P)] + SHUFFLED[:4] + ["a_1.fq", "no_such_file.fq", "-pairfiles", "-splitout", "early"] + case.options()
    r = subprocess.run(cmd, cwd=case.root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode != 0 and "no_such_file.fq" in r.stderr
    assert not [f for f in os.listdir(case.root) if f.startswith("early")]


def test_a_directory_stands_for_its_files(case):
    assert case.run(["lanes"], ["-pairfiles"]) == case.run(["lanes/" + f for f in SHUFFLED], ["-pairfiles"], out="listed.txt")


def test_splitout_writes_one_output_per_unit(case):
    case.run(SHUFFLED, ["-pairfiles", "-splitout", "split"], out=None)
    for g in GROUPS:
        with open(os.path.join(case.root, "split_%s_1.fq_%s_2.fq.txt" % (g, g))) as f:
            head, units, tail = case.parse(_mask(f.read()))
        assert head == case.base[0]
        assert [u for u, _ in units] == ["# %s_1.fq + %s_2.fq" % (g, g)] and units[0][1] == case.lines_of(g)
        assert "# queries: %d" % (2 * len(case.part[g])) in tail
    assert not os.path.exists(os.path.join(case.root, "split"))
