"""The `accmap` fixture (tests/golden/accmap, made by tests/golden/make_golden_taxmap.py) laid out as the reference's build was given
it, and what the mapping tests share: the targets of a genome layout through the Python restatements, and the golden parents."""
import gzip
import os
import shutil

import build_inputs as bi
import taxmap_ref as ref

GOLDEN = os.path.join(bi.GOLDEN, "accmap")
MAPS = ("nucl_gb.accession2taxid", "nucl_wgs.accession2taxid", "extra.accession2taxid")


def lay_out(work, genome_dirs=("a", "b"), summaries=True, maps=True):
    """work/genomes/<dir>/... and work/tax/...: the directory `metacache build accmap genomes -taxonomy tax` ran in.  genome_dirs:
    which of the two genome directories; summaries / maps: with the assembly_summary.txt files / the *.accession2taxid files"""
    for d in genome_dirs:
        dst = os.path.join(work, "genomes", d)
        os.makedirs(dst)
        for n in sorted(os.listdir(os.path.join(GOLDEN, "genomes", d))):
            src = os.path.join(GOLDEN, "genomes", d, n)
            if n.endswith(".gz"):
                with gzip.open(src, "rb") as f, open(os.path.join(dst, n[:-3]), "wb") as o:
                    o.write(f.read())
            elif summaries:
                shutil.copy(src, dst)
    os.makedirs(os.path.join(work, "tax"))
    for n in sorted(os.listdir(os.path.join(GOLDEN, "tax"))):
        if maps or n not in MAPS:
            shutil.copy(os.path.join(GOLDEN, "tax", n), os.path.join(work, "tax", n))
    return work


def genome_files(work):
    """the genome files below work/genomes, relative to work, in the reference's reading order"""
    out = []
    for d, _, names in os.walk(os.path.join(work, "genomes")):
        out += [os.path.relpath(os.path.join(d, n), work) for n in names]
    return sorted(out)


def expected_targets(work, taxdir="tax", postmap=None, before=()):
    """[(name, parent)] per target of the layout in `work`, by the restatements alone: the pre-mapping of the genome directories,
    the headers, then the *.accession2taxid files in the order the issue sets (postmap, the four standard names, the others by
    name).  before: the (name, parent) of a database the genomes are added to (`modify`): they come first and take part"""
    targets = [list(t) for t in before] + premapped_targets(work)
    rank_with_files(work, targets, taxdir, postmap)
    return [tuple(t) for t in targets]


def premapped_targets(work):
    """[[name, parent]] per target as the genome reader leaves them: assembly summaries, then the header"""
    files = genome_files(work)
    m = {}
    for d in ref.unique_directories(files):
        p = os.path.join(work, d, "assembly_summary.txt")
        if os.path.isfile(p):
            ref.read_mapping(open(p, "rb").read(), m)
    targets = []
    for name, hdr_parent, fname, _, _ in bi.read_genomes([(f, open(os.path.join(work, f), "rb").read()) for f in files]):
        parent = ref.find_taxon_id(m, name)
        if not parent:
            parent = ref.find_taxon_id(m, _file_id(fname.encode()))
        if not parent:
            parent = hdr_parent
        targets.append([name, max(parent, 0)])
    return targets


def map_file_order(work, taxdir, postmap):
    order = [postmap] if postmap else []
    if taxdir:
        order += [os.path.join(taxdir, n + ".accession2taxid") for n in ("nucl_gb", "nucl_wgs", "nucl_est", "nucl_gss")]
        more = []
        for d, _, names in os.walk(os.path.join(work, taxdir)):
            more += [os.path.relpath(os.path.join(d, n), work) for n in names]
        order += [f for f in sorted(more, key=os.fsencode) if ".accession2taxid" in f and f not in order]
    return order


def rank_with_files(work, targets, taxdir="tax", postmap=None):
    """targets: [[name, parent]], updated: the unranked ones through the mapping files that open"""
    names = ref.Names([t[0] for t in targets])
    unranked, parent = [t[1] == 0 for t in targets], [t[1] for t in targets]
    for f in map_file_order(work, taxdir, postmap):
        p = os.path.join(work, f)
        if os.path.isfile(p):
            ref.accmap(open(p, "rb").read(), names, unranked, parent)
    for t, p in zip(targets, parent):
        t[1] = p


def _file_id(fname):
    """extract_accession_string of a file name: as a target's name, but without the fall-back to the whole text"""
    n = bi.target_name(fname)
    if n != fname:
        return n
    # target_name returned its argument: either nothing was found, or the accession IS the whole text -- tell them apart
    return fname if bi.target_name(fname + b" ") != fname + b" " else b""


def golden_targets(host):
    """[(name, parent)] per target from the reference's own files"""
    return targets_of(host, os.path.join(GOLDEN, "P2", "accmap"), 2)


def targets_of(host, prefix, P):
    """[(name, parent)] per target of the database <prefix>.db_0 .. _<P-1>"""
    db = host.RefDb(prefix, P, meta_only=True)
    recs = [t for t in bi.taxon_list(db) if t["id"] < 0]
    recs.sort(key=lambda t: -t["id"])
    return [(t["name"].encode("latin-1") if isinstance(t["name"], str) else t["name"], t["parent"]) for t in recs]
