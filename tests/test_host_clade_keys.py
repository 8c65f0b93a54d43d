"""mcq_taxa_clade_keys: the targets' clade keys from the inputs of a build (genome files + taxonomy dump), before any database
exists -- what mcq_build_cli hands to mcq_table_remove_ambiguous for -remove-ambig-features RANK.  They must be the keys
mcq_refdb_clade_keys gives on the database the reference built from the same inputs (tests/golden/<tag>/P*/)."""
import importlib

import numpy as np
import pytest

import build_inputs as bi
from golden_util import Fixture

SUBSPECIES, SPECIES, FAMILY, ROOT = 3, 4, 10, 20
TAGS = sorted(t for t in bi.FIXTURES if bi.has_build_inputs(t))


@pytest.fixture(scope="module")
def host():
    pkg = importlib.import_module("metacache-mpi_amd")
    pkg.build_host()
    return importlib.import_module("metacache-mpi_amd.host")


@pytest.fixture(scope="module")
def inputs(host, tmp_path_factory):
    """per fixture: (target records, dump records, golden database), read once"""
    out = {}
    for tag in TAGS:
        work = bi.lay_out(tag, str(tmp_path_factory.mktemp(tag) / "w"))
        files = host.genome_files([work + "/genomes"])
        _, targets, _, _ = host.read_genomes(files, 1 << 16)
        P = bi.FIXTURES[tag][0][0]
        gold = host.RefDb(Fixture(tag, P).shard_paths[0][: -len(".db_0")], P, meta_only=True)
        out[tag] = (targets, host.read_taxdump(work + "/tax"), gold)
    return out


def test_every_fixture_with_build_inputs_is_covered():
    assert set(TAGS) >= {"mini", "tie", "noanc", "overpop", "wide"}


@pytest.mark.parametrize("rank", range(SUBSPECIES, ROOT + 1))
@pytest.mark.parametrize("tag", TAGS)
def test_keys_equal_those_of_the_golden_database(host, inputs, tag, rank):
    targets, dump, gold = inputs[tag]
    assert len(targets) == gold.info.n_targets
    got = host.taxa_clade_keys(targets, dump, rank)
    want = gold.clade_keys(rank)
    assert got.dtype == np.uint32 and np.array_equal(got, want), (tag, rank, got[:8], want[:8])
    assert (got == host.NO_TAXON).all() or got[got != host.NO_TAXON].max() < len(targets) + len(dump)


def test_targets_without_an_ancestor_get_the_none_key(host, inputs):
    targets, dump, _ = inputs["noanc"]
    k = host.taxa_clade_keys(targets, dump, SPECIES)
    assert len(k) == 4 and int((k == host.NO_TAXON).sum()) == 2
    targets, dump, _ = inputs["tie"]
    k = host.taxa_clade_keys(targets, dump, FAMILY)
    assert len(k) == 4 and (k == host.NO_TAXON).all()


def test_bad_arguments(host, inputs):
    targets, dump, _ = inputs["mini"]
    with pytest.raises(RuntimeError):
        host.taxa_clade_keys(targets, dump, 21)                       # rank none
    with pytest.raises(RuntimeError):
        host.taxa_clade_keys(targets + targets[:1], [], SPECIES)      # a target more than there are sequence-level taxa
