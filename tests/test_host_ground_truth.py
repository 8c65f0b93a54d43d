"""Ground truth from a read header and clade keys (mcq_refdb_ground_truth / mcq_refdb_clade_keys / mcq_refdb_taxon_clade), no GPU.

The reference: ground_truth (src/classification.cpp:111-131) tries, in this order, the header's accession.version as a
sequence name, its accession without version as the beginning of one (taxon_with_similar_name: upper_bound, so the first name
AFTER it), the id behind "taxid" + one character, and the whole header as a sequence name; the hit goes through
next_ranked_ancestor (src/sketch_database.h:724-737).  mini's targets are named 'NC_0000NN.1 taxid' (the accession ends at the
header's first '|', src/sequence_io.cpp:576-598) and hang under species 101, 102, 201, 202, 301; noanc has two targets that
hang under a genus directly."""
import importlib
import json
import os

import numpy as np
import pytest

from golden_util import GOLDEN, Fixture
from oracle import dbfile

NONE, KEEP_ALL = 0xFFFFFFFF, 0xFFFFFFFE
SPECIES, GENUS = 4, 6


@pytest.fixture(scope="module")
def mini():
    host = importlib.import_module("metacache-mpi_amd.host")
    fx = Fixture("mini", 4)
    return host, fx, host.RefDb(fx.shard_paths[0][: -len(".db_0")], 4)


def _parent_of_target(fx, t):
    return fx.tax.taxa[fx.tax.by_id[-(t + 1)]]["parent"]


def _target_named(fx, name):
    return next(-t["id"] - 1 for t in fx.tax.taxa if t["id"] < 0 and t["name"] == name)


def test_header_resolution(mini):
    host, fx, db = mini
    tid = lambda h: db.taxon_id(db.ground_truth(h))
    t3 = _target_named(fx, "NC_000003.1 taxid")
    sp3 = _parent_of_target(fx, t3)
    # 1. accession with version: the sequence name itself ('NC_000003.1 taxid|...' cuts at the '|' as the build did)
    assert tid("NC_000003.1 taxid|%d read 5" % 999999) == sp3
    # 2. accession without version: no name equals 'NC_000003', the first name after it begins with it
    assert tid("read_7 NC_000003 simulated") == sp3
    assert tid("NC_0000 x") == _parent_of_target(fx, _target_named(fx, "NC_000001.1 taxid"))     # (the FIRST name after the prefix)
    # 3. taxid|N followed by '|', by a space, at the end of the line
    assert tid("r1 taxid|201|more") == 201
    assert tid("r1 taxid|201 more") == 201
    assert tid("r1 taxid|201") == 201
    assert tid("r1 taxid=202") == 202                                  # "taxid" + ONE separator character, whatever it is
    assert tid("r1 taxid|100") == 100                                  # a ranked taxon above species is its own truth
    # ... with junk after it: stoull takes the leading digits, none = 0 = no taxon
    assert tid("r1 taxid|201abc") == 201
    assert db.ground_truth("r1 taxid|abc") == NONE
    assert db.ground_truth("r1 taxid|999999") == NONE                  # not in the taxonomy
    assert db.ground_truth("r1 taxid") == NONE
    # 4. the whole header is a target name (no '.', no prefix, no taxid: only this step can find it) -- mini has no such name,
    # so the step is pinned on its miss and on a database that has one below (test_whole_header_name)
    assert db.ground_truth("q0001_g7") == NONE
    assert db.ground_truth("") == NONE
    # order: the accession wins over a taxid in the same header
    assert tid("NC_000003.1 taxid|%d" % (301 if sp3 != 301 else 101)) == sp3


def test_whole_header_name(tmp_path):
    """step 4 on a database written with a target whose name is a plain word"""
    host = importlib.import_module("metacache-mpi_amd.host")
    fx = Fixture("tie", 2)
    taxa = []
    for t in fx.tax.taxa:
        name = "plainword" if t["id"] == -1 else t["name"]
        taxa.append(dict(t, name=name))
    p = fx.params
    params = dict(k=p["k"], sketch_size=p["s"], winlen=p["winlen"], winstride=p["winstride"], q_k=p["qk"], q_sketch_size=p["qs"],
                  q_winlen=p["qwinlen"], q_winstride=p["qwinstride"], max_locs_per_feature=p["maxlocs"])
    for r in range(2):
        s = fx.shards[r]
        locs = (s["tgt"].astype(np.uint64) << np.uint64(32)) | s["win"].astype(np.uint64)
        host.write_shard(str(tmp_path / ("w.db_%d" % r)), params, taxa, fx.n_targets, s["keys"], s["off"], locs)
    db = host.RefDb(str(tmp_path / "w"), 2)
    assert db.taxon_id(db.ground_truth("plainword")) == _parent_of_target(fx, 0)
    assert db.ground_truth("plainwor") == NONE


@pytest.mark.parametrize("tag,P", [("mini", 4), ("noanc", 2)])
def test_clade_keys(tag, P):
    host = importlib.import_module("metacache-mpi_amd.host")
    fx = Fixture(tag, P)
    db = host.RefDb(fx.shard_paths[0][: -len(".db_0")], P)
    for rank in (SPECIES, GENUS):
        want = np.array([fx.tax.lineage[fx.tax.by_id[-(t + 1)], rank] for t in range(fx.n_targets)], np.uint32)
        got = db.clade_keys(rank)
        assert np.array_equal(got, want)
        assert KEEP_ALL not in got
    if tag == "noanc":                                                # targets under a genus directly: no species, but a genus
        sp, ge = db.clade_keys(SPECIES), db.clade_keys(GENUS)
        assert (sp == NONE).sum() == 2 and (ge == NONE).sum() == 0
    # a truth's key: its ancestor at the rank; none above the rank; KEEP_ALL without a truth
    with open(os.path.join(GOLDEN, tag, "eval_headers.json")) as f:
        headers = json.load(f)
    kinds = set()
    for h in headers:
        t = db.ground_truth(h)
        k = db.taxon_clade(t, SPECIES)
        if t == NONE:
            assert k == KEEP_ALL; kinds.add("none")
        elif db.taxon_rank(t) > SPECIES:
            assert k == NONE; kinds.add("above")
        else:
            assert k == t and db.taxon_rank(t) == SPECIES; kinds.add("species")
        assert db.taxon_clade(t, GENUS) == (KEEP_ALL if t == NONE else db.ancestor(t, GENUS))
    assert kinds == {"none", "above", "species"}, kinds


# ---- the statistics: classification_statistics::assign_known_correct (src/classification_statistics.h:91-123) restated, and the
# summary lines of show_taxon_statistics (src/printing.cpp:522-600) from their quoted templates
ROOT, RNONE = 20, 21
SHOWN = [0, 3, 4, 6, 10, 12, 14, 16, 18, 19, 20]      # the `ranks` array of src/printing.cpp:526-534
NAMES = {0: "sequence", 3: "subspecies", 4: "species", 6: "genus", 10: "family", 12: "order", 14: "class", 16: "phylum",
         18: "kingdom", 19: "domain", 20: "root"}
# (assigned, truth, lca) ranks: right at the rank of the truth; assigned below a truth it agrees with; wrong at species, right from
# genus; wrong at every rank (no LCA); unclassified with a known truth; classified without a truth; neither; an LCA BELOW the
# assigned rank (the plausibility check lifts it); truth above the assignment; sequence-level assignment that is right
TRIPLES = [(4, 4, 4), (4, 6, 6), (4, 4, 6), (4, 4, RNONE), (RNONE, 4, RNONE), (6, RNONE, RNONE), (RNONE, RNONE, RNONE),
           (10, 4, 4), (4, 10, 10), (0, 4, 4), (4, 4, 4), (6, 4, 19), (0, 0, 0), (3, 4, 6)]


def _restated(triples):
    asg, kn, co, wr = ([0] * 22 for _ in range(4))
    for assigned, known, correct in triples:
        if assigned == RNONE:                                        # assign, :70-78
            asg[RNONE] += 1
        else:
            for r in range(assigned, ROOT + 1): asg[r] += 1
        if correct < assigned: correct = assigned                    # :96-97
        if correct < known: correct = known
        if known == RNONE:                                           # :100-101
            kn[RNONE] += 1
            continue
        for r in range(known, ROOT + 1): kn[r] += 1                  # :104
        if correct == RNONE: co[RNONE] += 1                          # :106-111
        else:
            for r in range(correct, ROOT + 1): co[r] += 1
        if correct > known and correct > assigned:                   # :114-118
            for r in range(0, correct): wr[r] += 1
    return asg, kn, co, wr


def _g(x):
    return "%g" % x                                                  # ostream's default formatting of a double


def _summary(asg, kn, co, wr, prefix):
    total = asg[ROOT] + asg[RNONE]
    rows = [r for r in SHOWN if asg[r] > 0]
    rn = lambda r: NAMES[r].ljust(11)
    if asg[ROOT] < 1:
        return "None of the input sequences could be classified.\n"
    t = ""
    if asg[RNONE] > 0:
        t += prefix + "unclassified: " + _g(100 * (asg[RNONE] / total)) + "% (" + str(asg[RNONE]) + ")\n"
    t += prefix + "classified:\n"
    for r in rows: t += prefix + "  " + rn(r) + _g(100 * (asg[r] / total)) + "% (" + str(asg[r]) + ")\n"
    if kn[ROOT] > 0:                                                 # :557
        if kn[RNONE] > 0:
            t += prefix + "ground truth unknown: " + _g(100 * (kn[RNONE] / total)) + "% (" + str(kn[RNONE]) + ")\n"
        t += prefix + "ground truth known:\n"
        for r in rows: t += prefix + "  " + rn(r) + _g(100 * (kn[r] / total)) + "% (" + str(kn[r]) + ")\n"
        t += prefix + "correctly classified:\n"
        for r in rows: t += prefix + "  " + rn(r) + str(co[r]) + "\n"
        t += prefix + "precision (correctly classified / classified) if ground truth known:\n"
        for r in rows:
            tot = float(co[r] + wr[r])
            t += prefix + "  " + rn(r) + _g(100 * (co[r] / tot if tot > 0 else 0)) + "%\n"
        t += prefix + "sensitivity (correctly classified / all) if ground truth known:\n"
        for r in rows: t += prefix + "  " + rn(r) + _g(100 * (co[r] / kn[r] if kn[r] > 0 else 0)) + "%\n"
    return t


def test_statistics_and_summary_text():
    host = importlib.import_module("metacache-mpi_amd.host")
    st, half = host.EvalStats(), host.EvalStats()
    for t in TRIPLES[:5]: st.assign_known_correct(*t)
    for t in TRIPLES[5:]: half.assign_known_correct(*t)
    st.add(half)                                                     # (the writer threads' partial counts are added up)
    asg, kn, co, wr = _restated(TRIPLES)
    assert list(st.rec.assigned) == asg and list(st.rec.known) == kn and list(st.rec.correct) == co and list(st.rec.wrong) == wr
    total = len(TRIPLES)
    assert st.total() == total and st.unknown() == kn[RNONE] and st.unassigned() == asg[RNONE]
    assert st.known() == kn[ROOT] and st.correct() == co[ROOT] and st.wrong() == wr[ROOT] and st.assigned() == asg[ROOT]
    for r in range(ROOT + 1):
        assert (st.known(r), st.correct(r), st.wrong(r), st.assigned(r)) == (kn[r], co[r], wr[r], asg[r])
        assert st.known_rate(r) == kn[r] / total and st.classification_rate(r) == asg[r] / total
        tot = float(co[r] + wr[r])
        assert st.precision(r) == (co[r] / tot if tot > 0 else 0)
        assert st.sensitivity(r) == (co[r] / kn[r] if kn[r] > 0 else 0)
    assert st.unknown_rate() == kn[RNONE] / total and st.unclassified_rate() == asg[RNONE] / total
    assert wr[4] > 0 and co[RNONE] > 0 and kn[RNONE] > 0            # the list reaches the wrong, never-right and unknown branches
    text = st.text("# ")
    assert text == _summary(asg, kn, co, wr, "# ")
    assert "# ground truth unknown: " in text and "# precision (correctly classified / classified) if ground truth known:\n" in text
    assert st.text("%%") == _summary(asg, kn, co, wr, "%%")          # the prefix is the caller's comment string

    only = host.EvalStats()                                          # no truth known: the block of src/printing.cpp:557 is not written
    for a in (4, RNONE, 6): only.assign_known_correct(a, RNONE, RNONE)
    plain = host.EvalStats()
    for a in (4, RNONE, 6): plain.assign(a)
    assert only.text() == plain.text() and "ground truth" not in only.text()
    none = host.EvalStats()
    none.assign_known_correct(RNONE, 4, RNONE)
    assert none.text() == "None of the input sequences could be classified.\n"
    empty = host.EvalStats()
    assert (empty.total(), empty.known_rate(4), empty.precision(4), empty.sensitivity(4), empty.unknown_rate()) == (0, 0, 0, 0, 0)


def test_ranked_lca(mini):
    host, fx, db = mini
    lin = fx.tax.lineage
    keys = [db.ground_truth("r taxid|%d" % i) for i in (101, 102, 201, 301, 100, 200)]
    assert NONE not in keys
    for a in keys:
        assert db.ranked_lca(a, NONE) == NONE and db.ranked_lca(NONE, a) == NONE
        for b in keys:
            want = next((int(lin[a, r]) for r in range(ROOT + 1) if lin[a, r] != NONE and lin[a, r] == lin[b, r]), NONE)
            assert db.ranked_lca(a, b) == want
    assert db.ranked_lca(keys[0], keys[0]) == keys[0]
    assert db.taxon_rank(db.ranked_lca(keys[0], keys[1])) == GENUS   # 101 and 102: two species of genus 100
