"""Per-read classification by the LCA of the near-best hits (k_read_lca, k_lca_count, the roll-up of dsb_*_lca_counts; classify
--kraken-out / --kraken-report).  The model of tests/lca_lib.py over the same hits is the hard assertion, record for
record and exact; the reports are held against it and against hand-typed expected texts (tests/golden/lca)."""
import gzip
import os
import subprocess

import pytest

import lca_lib as M
from conftest import GOLDEN, ROOT

CLI = os.path.join(ROOT, "desamba_amd", "bin", "deSAMBA")
SYNTH = os.path.join(GOLDEN, "synth")
NODES = os.path.join(GOLDEN, "analysis", "nodes.dmp")
LCA = os.path.join(GOLDEN, "lca")
NAMES = os.path.join(LCA, "names.dmp")


# ---------------------------------------------------------------- without a GPU

# a hand-built tree: 1 - 2 - {3 - {5, 6}, 4 - 7}, 1 - 8; an unrooted chain 20 -> 21 -> (22, not listed); max_tid 30
TREE = {1: 0, 2: 1, 3: 2, 4: 2, 5: 3, 6: 3, 7: 4, 8: 1, 20: 21, 21: 22}
TREE_MAX = 30


def lca_of(tids, scores=None, permille=1000):
    ref_tid = list(tids)
    hits = [(r, scores[r] if scores else 100) for r in range(len(ref_tid))]
    return M.read_lca(hits, ref_tid, TREE, TREE_MAX, permille)


def test_model_on_a_hand_built_tree():
    C, N, A = M.CLASSIFIED, M.NO_TAXON, M.AMBIGUOUS
    assert lca_of([5]) == (5, 100, 1, 3, C)
    assert lca_of([5, 5, 5]) == (5, 100, 3, 3, C)                       # the same node: hits count, taxids do not
    assert lca_of([5, 3]) == (3, 100, 2, 2, C | A)                      # ancestor and descendant
    assert lca_of([3, 5]) == (3, 100, 2, 2, C | A)
    assert lca_of([5, 6]) == (3, 100, 2, 2, C | A)                      # siblings
    assert lca_of([5, 7]) == (2, 100, 2, 1, C | A)                      # cousins
    assert lca_of([5, 8]) == (1, 100, 2, 0, C | A)
    assert lca_of([5, 1]) == (1, 100, 2, 0, C | A)
    assert lca_of([1]) == (1, 100, 1, 0, C)
    assert lca_of([5, 20]) == (5, 100, 2, 3, C)                         # an unrooted chain is left out (and is not a second taxid)
    assert lca_of([5, 0, 31, M.NONE]) == (5, 100, 4, 3, C)              # taxid 0, above max_tid, an odd reference name
    assert lca_of([20, 21, 0, 22]) == (0, 100, 4, 0, C | N)             # all candidates unrooted
    assert lca_of([]) == (0, 0, 0, 0, 0)
    # the threshold: AS * 1000 >= S_max * permille
    assert lca_of([5, 7], [100, 95], 950) == (2, 100, 2, 1, C | A)
    assert lca_of([5, 7], [100, 94], 950) == (5, 100, 1, 3, C)
    assert lca_of([20, 7], [100, 94], 950) == (0, 100, 1, 0, C | N)     # the best hit passes alone and is unrooted
    # hits beyond the index are skipped before S_max
    assert M.read_lca([(0, 50), (3, 900)], [5], TREE, TREE_MAX, 1000) == (5, 50, 1, 3, C)
    assert M.read_lca([(3, 900)], [5], TREE, TREE_MAX, 1000) == (0, 0, 0, 0, 0)
    rows, summ = M.counts([lca_of([5]), lca_of([5, 6]), lca_of([5, 7]), lca_of([20]), lca_of([])], TREE, TREE_MAX, 1000)
    assert rows == [(1, 3, 0), (2, 3, 1), (3, 2, 1), (5, 1, 1)]
    assert summ == dict(reads=5, classified=3, no_taxon=1, ambiguous=2, min_permille=1000)
    assert M.ref_taxid("tid|562|x") == 562 and M.ref_taxid("plain") == 0 and M.ref_taxid("*x|5|") == M.NONE and M.ref_taxid("a\t|5|") == M.NONE


def small_rows():
    import numpy as np
    import desamba_amd as D
    rows = [tuple(int(x) for x in ln.split()) for ln in open(os.path.join(LCA, "small_rows.tsv"))]
    arr = np.zeros(len(rows), dtype=D.TAXON_COUNT_DTYPE)
    for k, (t, c, d) in enumerate(rows):
        arr[k] = (t, 0, c, d)
    return rows, arr


def test_lca_report_format(built):
    import desamba_amd as D
    T = D.Taxonomy(os.path.join(LCA, "small_nodes.dmp"))
    names = D.TaxNames(os.path.join(LCA, "small_names.dmp"))
    parent, rank, max_tid = M.load_nodes(os.path.join(LCA, "small_nodes.dmp"))
    mnames = M.load_names(os.path.join(LCA, "small_names.dmp"))
    rows, arr = small_rows()
    summ = dict(reads=100, classified=90, no_taxon=3, ambiguous=40, min_permille=950)
    want = open(os.path.join(LCA, "small_report_names.txt"), "rb").read()
    got = D.format_lca_report(T, arr, summ, names)
    assert got == want == M.report(rows, summ, parent, rank, mnames)
    for code in (b"\tR\t", b"\tR1\t", b"\tD\t2\t", b"\tD\t4\t", b"\tK\t", b"\tP\t", b"\tC\t", b"\tO\t", b"\tF\t", b"\tG\t", b"\tS\t", b"\tS1\t", b"\tS2\t", b"\tU\t"):
        assert code in got, code
    assert got.index(b"\tS\t11\t") < got.index(b"\tS\t14\t")           # the tie in clade_reads: taxid ascending
    # rows in another order give the same text
    assert D.format_lca_report(T, arr[::-1], summ, names) == want
    # without names: the decimal taxid
    plain = open(os.path.join(LCA, "small_report_plain.txt"), "rb").read()
    assert D.format_lca_report(T, arr, summ) == plain == M.report(rows, summ, parent, rank)
    # no unclassified reads: no U line
    s90 = dict(summ, reads=90)
    allc = open(os.path.join(LCA, "small_report_all_classified.txt"), "rb").read()
    assert D.format_lca_report(T, arr, s90, names) == allc == M.report(rows, s90, parent, rank, mnames)
    assert not allc.startswith(b" 10.00") and b"unclassified" not in allc
    # zero reads: empty; no row at all but reads: the U line alone
    assert D.format_lca_report(T, arr[:0], dict(summ, reads=0, classified=0)) == b""
    assert D.format_lca_report(T, arr[:0], dict(summ, reads=7, classified=0)) == b"100.00\t7\t7\tU\t0\tunclassified\n"
    # a short buffer gives -1
    s = D.DsbLcaSummary(**{f: summ[f] for f in D.LCA_SUMMARY_FIELDS})
    L = D.lib()
    args = (T.h, names.h, arr.ctypes.data_as(D.C.c_void_p), len(arr), D.C.byref(s))
    assert L.dsb_lca_report_format(*args, D.C.create_string_buffer(len(want)), len(want)) == -1
    assert L.dsb_lca_report_format(*args, D.C.create_string_buffer(len(want) + 1), len(want) + 1) == len(want)
    names.close(); T.close()


def test_format_kraken(built):
    import numpy as np
    import desamba_amd as D
    reads = D.make_reads([("r1 extra", b"ACGT" * 10, None), ("r2", b"A" * 7, b"5" * 7)])
    lca = np.zeros(2, dtype=D.LCA_DTYPE)
    lca[0] = (562, 1234, 3, 5, M.CLASSIFIED | M.AMBIGUOUS, 0)
    lca[1] = (0, 77, 1, 0, M.CLASSIFIED | M.NO_TAXON, 0)
    got = D.format_kraken(reads, lca)
    assert got == b"C\tr1 extra\t562\t40\t1234:3\nU\tr2\t0\t7\t77:1\n"
    assert got == M.kraken_line("r1 extra", 40, (562, 1234, 3, 5, 5)) + M.kraken_line("r2", 7, (0, 77, 1, 0, 3))
    line = b"C\tr1 extra\t562\t40\t1234:3\n"
    L = D.lib()
    assert L.dsb_format_kraken(D.C.byref(reads[0]), lca[0:1].ctypes.data_as(D.C.c_void_p), D.C.create_string_buffer(len(line)), len(line)) == -1
    assert L.dsb_format_kraken(D.C.byref(reads[0]), lca[0:1].ctypes.data_as(D.C.c_void_p), D.C.create_string_buffer(len(line) + 1), len(line) + 1) == len(line)
    assert D.C.sizeof(D.DsbReadLca) == 16 == np.dtype(D.LCA_DTYPE).itemsize and np.dtype(D.TAXON_COUNT_DTYPE).itemsize == 24


def test_lca_null_handles_and_ranges(built, tmp_path):
    import desamba_amd as D
    L = D.lib()
    n = D.C.c_size_t(0)
    assert L.dsb_ctx_enable_lca(None, 1, 950) == D.DSB_EINVAL
    assert L.dsb_ctx_reset_lca(None) == D.DSB_EINVAL
    assert L.dsb_batch_lca(None, None) == D.DSB_EINVAL
    assert L.dsb_ctx_lca_counts(None, None, 0, D.C.byref(n), None) == D.DSB_EINVAL
    assert L.dsb_multi_enable_lca(None, 1, 950) == D.DSB_EINVAL
    assert L.dsb_multi_lca(None, None) == D.DSB_EINVAL
    assert L.dsb_multi_lca_counts(None, None, 0, D.C.byref(n), None) == D.DSB_EINVAL
    assert L.dsb_format_kraken(None, None, None, 0) == -1
    assert L.dsb_lca_report_format(None, None, None, 0, None, None, 0) == -1
    h = D.C.c_void_p()
    assert L.dsb_taxnames_load(None, D.C.byref(h)) == D.DSB_EINVAL
    assert L.dsb_taxnames_load(os.fsencode(str(tmp_path / "missing.dmp")), D.C.byref(h)) == D.DSB_EIO
    L.dsb_taxnames_close(None)
    with pytest.raises(D.DsbError) as e:
        D.TaxNames(str(tmp_path / "missing.dmp"))
    assert e.value.code == D.DSB_EIO


def test_cli_refuses_lca_flags_without_taxonomy_and_bad_min_frac(built, tmp_path):
    for flags in (["--kraken-report", str(tmp_path / "k.txt")], ["--kraken-out", str(tmp_path / "k.out")], ["--names", NAMES], ["--lca-min-frac", "0.9"]):
        p = subprocess.run([CLI, "classify"] + flags + ["nowhere", os.path.join(SYNTH, "ngs150.fq")], stderr=subprocess.PIPE, stdout=subprocess.PIPE)
        assert p.returncode != 0 and b"--taxonomy" in p.stderr, flags                  # (refused before the index is opened)
    for bad in ("0", "1.5", "abc", "-0.1", "0.95x", "0.0001"):
        p = subprocess.run([CLI, "classify", "--taxonomy", NODES, "--kraken-report", str(tmp_path / "k.txt"), "--lca-min-frac", bad, "nowhere", "nothing.fq"],
                           stderr=subprocess.PIPE, stdout=subprocess.PIPE)
        assert p.returncode != 0 and b"--lca-min-frac" in p.stderr, bad
    p = subprocess.run([CLI, "classify", "-h"], stderr=subprocess.PIPE, stdout=subprocess.PIPE)
    for opt in (b"--kraken-out", b"--kraken-report", b"--names", b"--lca-min-frac"):
        assert opt in p.stderr


def test_loader_keeps_depth_and_rootedness(built):
    """the model's chains against dsb_taxonomy_parent over the small tree (the depth table itself is seen through the GPU tests)"""
    import desamba_amd as D
    T = D.Taxonomy(os.path.join(LCA, "small_nodes.dmp"))
    parent, rank, max_tid = M.load_nodes(os.path.join(LCA, "small_nodes.dmp"))
    assert T.max_tid == max_tid
    for t in list(parent) + [0, 40, 99]:
        assert T.parent(t) == (parent[t] if t in parent else M.NONE)
    assert M.depth(parent, max_tid, 13) == 11 and M.depth(parent, max_tid, 30) is None and M.depth(parent, max_tid, 1) == 0
    T.close()


# ---------------------------------------------------------------- on the GPU

def permille(frac):
    return int(frac * 1000 + 0.5)


def ref_tids(idx):
    return [M.ref_taxid(idx.ref_name(r)) for r in range(idx.n_ref)]


@pytest.fixture(scope="module")
def env(demo):
    import desamba_amd as D
    idx = D.Index(demo["index"])
    T = D.Taxonomy(NODES)
    parent, rank, max_tid = M.load_nodes(NODES)
    yield D, idx, T, (parent, rank, max_tid)
    T.close(); idx.close()


def lca_ctx(D, idx, T, frac=0.95, **kw):
    ctx = D.Ctx(idx, 0, **kw)
    ctx.set_taxonomy(T)
    ctx.enable_lca(min_frac=frac)
    return ctx


def check_run(D, ctx_or_multi, T, tax, res, n, rtids, frac, label, names=None, mnames=None):
    """records, rows, summary and report of a run against the model over the run's own hits"""
    parent, rank, max_tid = tax
    want = M.records(res, n, rtids, parent, max_tid, permille(frac))
    got = M.as_tuples(ctx_or_multi.lca())
    assert len(got) == n, label
    for i in range(n):
        assert got[i] == want[i], (label, i, got[i], want[i])
    return want


def check_counts(D, runner, T, tax, want, frac, label, names=None, mnames=None):
    parent, rank, max_tid = tax
    rows, summ = runner.lca_counts()
    wrows, wsumm = M.counts(want, parent, max_tid, permille(frac))
    assert M.rows_as_tuples(rows) == wrows, label
    assert summ == wsumm, label
    assert D.format_lca_report(T, rows, summ, names) == M.report(wrows, wsumm, parent, rank, mnames), label
    clade1 = next((c for t, c, d in wrows if t == 1), 0)
    assert summ["reads"] - summ["classified"] + clade1 == summ["reads"], label
    return rows, summ


def golden_desfull_hits(name, names):
    """every read's (ref_ID, AS) hits from the reference's DES_FULL golden output"""
    ref_id = {n: r for r, n in enumerate(names)}
    out, cur = [], None
    for line in open(os.path.join(SYNTH, name + ".desfull.ubfree.txt"), "rb").read().splitlines():
        if not line.strip():
            if cur is not None:
                out.append(cur)
            cur = None
            continue
        if cur is None:
            cur = []
            continue
        f = line.split()
        cur.append((ref_id[f[3].decode()], int(f[8])))
    if cur is not None:
        out.append(cur)
    return out


@pytest.mark.gpu
def test_lca_equals_the_model_on_the_reference_s_hits(env):
    D, idx, T, tax = env
    parent, rank, max_tid = tax
    names = [idx.ref_name(r) for r in range(idx.n_ref)]
    rtids = ref_tids(idx)
    recs = D.read_fastq(os.path.join(SYNTH, "ngs150.fq"))
    hits = golden_desfull_hits("ngs150", names)
    assert len(hits) == len(recs) == 400
    differ = {}
    for frac in (1.0, 0.95, 0.9):
        ctx = lca_ctx(D, idx, T, frac)
        ctx.classify(D.make_reads(recs))
        got = M.as_tuples(ctx.lca())
        want = [M.read_lca(h, rtids, parent, max_tid, permille(frac)) for h in hits]
        assert got == want, frac
        assert all(r[0] for r in got)
        differ[frac] = sum(1 for h, r in zip(hits, want) if r[0] != rtids[h[0][0]])
        check_counts(D, ctx, T, tax, want, frac, "ngs150 %g" % frac)
        ctx.close()
    print("ngs150: reads whose LCA is not the primary's taxid:", differ)
    assert differ == {1.0: 0, 0.95: 2, 0.9: 3}


@pytest.mark.gpu
def test_lca_equals_the_model_on_own_hits(env, strain):
    D, idx, T, tax = env
    rtids = ref_tids(idx)
    names = D.TaxNames(NAMES)
    mnames = M.load_names(NAMES)
    ctx = lca_ctx(D, idx, T)
    for name in ("pb", "ont20k", "heavy"):
        recs = D.read_fastq(os.path.join(SYNTH, name + ".fq"))
        for frac in (1.0, 0.95, 0.9):
            ctx.enable_lca(min_frac=frac)                        # (on again: new threshold, counts zeroed)
            ctx.reset_history()
            res = ctx.classify(D.make_reads(recs), strict=False)
            want = check_run(D, ctx, T, tax, res, len(recs), rtids, frac, "%s %g" % (name, frac))
            check_counts(D, ctx, T, tax, want, frac, "%s %g" % (name, frac), names, mnames)
    ctx.close()
    sidx = D.Index(strain["index"])
    recs = D.read_fastq(strain["fastq"])
    ctx = lca_ctx(D, sidx, T, max_sec_N=0)                       # (-r 0: the hits do not depend on it)
    res = ctx.classify(D.make_reads(recs), strict=False)
    want = check_run(D, ctx, T, tax, res, len(recs), ref_tids(sidx), 0.95, "strain")
    check_counts(D, ctx, T, tax, want, 0.95, "strain", names, mnames)
    ctx.close(); sidx.close(); names.close()


def decode(codes):
    import numpy as np
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.asarray(codes, dtype=np.int64)].tobytes()


def write_fasta(path, recs):
    with open(path, "wb") as f:
        for name, codes in recs:
            seq = decode(codes)
            f.write(b">" + name.encode() + b"\n")
            for k in range(0, len(seq), 80):
                f.write(seq[k:k + 80] + b"\n")


def truth_tree():
    """1 - 2 (superkingdom) - 2 families (10, 11) - 4 genera (20 ..) - 8 species (30 ..) - 16 strains (100 .., no rank)"""
    nodes = [(1, 1, "no rank"), (2, 1, "superkingdom")]
    fam = [10, 11]; gen = [20 + g for g in range(4)]; spe = [30 + s for s in range(8)]; strain = [100 + k for k in range(16)]
    nodes += [(f, 2, "family") for f in fam]
    nodes += [(g, fam[i // 2], "genus") for i, g in enumerate(gen)]
    nodes += [(s, gen[i // 2], "species") for i, s in enumerate(spe)]
    nodes += [(k, spe[i // 2], "no rank") for i, k in enumerate(strain)]
    text = "".join("%d\t|\t%d\t|\t%s\t|\t\t|\n" % n for n in nodes)
    return text, fam, gen, spe, strain


@pytest.mark.gpu
def test_lca_known_truth(built, tmp_path):
    """16 genomes, each the concatenation of its family's, genus's, species's and own random 40-kbp segment; reads lie wholly
    inside one segment: the truth is the segment's node.  Shares measured on an MI355X are recorded in DESIGN 2.11."""
    import numpy as np
    import desamba_amd as D
    from test_abundance import mutate, revcomp
    rng = np.random.default_rng(20261016)
    text, fam, gen, spe, strain = truth_tree()
    (tmp_path / "nodes.dmp").write_text(text)
    SEG = 40000
    seg = {t: rng.integers(0, 4, SEG).astype(np.uint8) for t in fam + gen + spe + strain}
    genomes = []
    for i, k in enumerate(strain):
        genomes.append(("tid|%d|strain%d" % (k, i), np.concatenate([seg[fam[i // 8]], seg[gen[i // 4]], seg[spe[i // 2]], seg[k]])))
    write_fasta(str(tmp_path / "g.fa"), genomes)
    D.build_index(str(tmp_path / "g.fa"), str(tmp_path / "index"))
    recs, truth, level = [], [], []
    for lv, nodes_ in (("family", fam), ("genus", gen), ("species", spe), ("strain", strain)):
        for t in nodes_:
            for j in range(12):
                st = int(rng.integers(500, SEG - 3000 - 500))
                s = mutate(rng, seg[t][st:st + 3000], 0.08)
                if rng.random() < 0.5:
                    s = revcomp(s)
                recs.append(("%s_%d_%d" % (lv, t, j), decode(s), b"5" * len(s))); truth.append(t); level.append(lv)
    order = rng.permutation(len(recs))
    recs = [recs[i] for i in order]; truth = [truth[i] for i in order]; level = [level[i] for i in order]
    idx = D.Index(str(tmp_path / "index"))
    T = D.Taxonomy(str(tmp_path / "nodes.dmp"))
    tax = M.load_nodes(str(tmp_path / "nodes.dmp"))
    rtids = ref_tids(idx)
    shares = {}
    taxon_hits = None
    for frac in (1.0, 0.95, 0.9):
        ctx = lca_ctx(D, idx, T, frac, max_sec_N=100)
        res = ctx.classify(D.make_reads(recs), strict=False)
        want = check_run(D, ctx, T, tax, res, len(recs), rtids, frac, "truth %g" % frac)
        check_counts(D, ctx, T, tax, want, frac, "truth %g" % frac)
        if taxon_hits is None:
            taxa = ctx.taxa()
            taxon_hits = {lv: sum(1 for i in range(len(recs)) if level[i] == lv and int(taxa[i]) == truth[i]) for lv in ("family", "genus", "species")}
        for lv in ("family", "genus", "species", "strain"):
            k = [i for i in range(len(recs)) if level[i] == lv]
            shares[(frac, lv)] = sum(1 for i in k if want[i][0] == truth[i]) / len(k)
        ctx.close()
    for frac in (1.0, 0.95, 0.9):
        print("known truth, min_frac %.2f: LCA = truth node for " % frac + ", ".join("%s %.3f" % (lv, shares[(frac, lv)]) for lv in ("family", "genus", "species", "strain")))
    print("k_read_taxon = truth node:", taxon_hits)
    assert taxon_hits == {"family": 0, "genus": 0, "species": 0}          # it is always a strain
    for lv in ("family", "genus", "species"):
        assert shares[(1.0, lv)] > 0.5, lv                                  # identical copies tie by construction
    T.close(); idx.close()


@pytest.mark.gpu
def test_lca_identical_copies(built, tmp_path):
    """80 identical copies under 80 taxids spread over the known-truth tree: more than 64 passing hits (the strided lanes)"""
    import numpy as np
    import desamba_amd as D
    from test_abundance import sample
    rng = np.random.default_rng(77)
    text, fam, gen, spe, strain = truth_tree()
    # 80 taxids: the 16 strains, and 64 more strains (200 ..) hung under the 8 species in turn -- all below family 10 or 11
    extra = [200 + k for k in range(64)]
    text += "".join("%d\t|\t%d\t|\tno rank\t|\t\t|\n" % (t, spe[k % 8]) for k, t in enumerate(extra))
    (tmp_path / "nodes.dmp").write_text(text)
    tids = strain + extra
    G = rng.integers(0, 4, 20000).astype(np.uint8)
    other = rng.integers(0, 4, 40000).astype(np.uint8)
    write_fasta(str(tmp_path / "copies.fa"), [("tid|%d|copy%d" % (t, i), G) for i, t in enumerate(tids)] + [("tid|100|other", other)])
    D.build_index(str(tmp_path / "copies.fa"), str(tmp_path / "index"))
    recs = sample(rng, G, 60, 3000, 0.05, "G") + sample(rng, other, 20, 3000, 0.05, "O")
    idx = D.Index(str(tmp_path / "index"))
    T = D.Taxonomy(str(tmp_path / "nodes.dmp"))
    tax = M.load_nodes(str(tmp_path / "nodes.dmp"))
    ctx = lca_ctx(D, idx, T, 0.95, max_sec_N=100)
    res = ctx.classify(D.make_reads(recs), strict=False)
    want = check_run(D, ctx, T, tax, res, len(recs), ref_tids(idx), 0.95, "copies")
    check_counts(D, ctx, T, tax, want, 0.95, "copies")
    big = [r for r in want if r[2] > 64]
    print("reads with more than 64 passing hits: %d, largest n_pass %d" % (len(big), max(r[2] for r in want)))
    assert len(big) >= 30
    assert all(r[0] == 2 and r[4] & M.AMBIGUOUS for r in big)              # the copies' common node: the superkingdom over both families
    assert sum(1 for r in want if r[0] == 100 and not r[4] & M.AMBIGUOUS) >= 15
    ctx.close(); T.close(); idx.close()


def det_reads():
    import desamba_amd as D
    return D.read_fastq(os.path.join(SYNTH, "pb.fq")) + D.read_fastq(os.path.join(SYNTH, "ngs150.fq")) + D.read_fastq(os.path.join(SYNTH, "ont20k.fq"))


@pytest.mark.gpu
def test_lca_identical_across_batches_slots_contexts(env, monkeypatch):
    import numpy as np
    D, idx, T, tax = env
    recs = det_reads()
    hist = lambda s: max([len(x[1]) for x in recs[:s]], default=0)

    def text(runner):
        rows, summ = runner.lca_counts()
        return rows.tobytes(), summ, D.format_lca_report(T, rows, summ)
    ctx = D.Ctx(idx, 0)
    with pytest.raises(D.DsbError) as e:
        ctx.enable_lca()                                          # no taxonomy attached
    assert e.value.code == D.DSB_EINVAL
    ctx.set_taxonomy(T)
    for call in (ctx.lca, ctx.lca_counts, ctx.reset_lca):
        with pytest.raises(D.DsbError) as e:
            call()
        assert e.value.code == D.DSB_EINVAL
    assert D.lib().dsb_ctx_enable_lca(ctx.h, 1, 0) == D.DSB_EINVAL and D.lib().dsb_ctx_enable_lca(ctx.h, 1, 1001) == D.DSB_EINVAL
    ctx.enable_lca()
    res = ctx.classify(D.make_reads(recs))
    one = ctx.lca()
    want = check_run(D, ctx, T, tax, res, len(recs), ref_tids(idx), 0.95, "one batch")
    base = text(ctx)
    assert base[1]["reads"] == len(recs) and base[1]["classified"] > 100
    assert text(ctx) == base                                      # fetching twice gives the same rows
    n = D.C.c_size_t(0)                                           # a short row buffer: DSB_ECAP, the count all the same
    short = np.zeros(1, dtype=D.TAXON_COUNT_DTYPE)
    assert D.lib().dsb_ctx_lca_counts(ctx.h, short.ctypes.data_as(D.C.c_void_p), 1, D.C.byref(n), None) == D.DSB_ECAP
    assert n.value == len(base[0]) // 24 > 1 and short.tobytes() == base[0][:24]
    # three batches
    ctx.reset_lca()
    rows, summ = ctx.lca_counts()
    assert len(rows) == 0 and summ == dict(reads=0, classified=0, no_taxon=0, ambiguous=0, min_permille=950)
    cuts = [0, 41, 230, len(recs)]
    parts = []
    for a, b in zip(cuts, cuts[1:]):
        ctx.set_history(hist(a))
        ctx.classify(D.make_reads(recs[a:b]))
        parts.append(ctx.lca())
    assert np.concatenate(parts).tobytes() == one.tobytes() and text(ctx) == base
    # another threshold: counts zeroed, other records
    ctx.enable_lca(min_frac=0.5)
    assert ctx.lca_counts()[1] == dict(reads=0, classified=0, no_taxon=0, ambiguous=0, min_permille=500)
    ctx.reset_history()
    res = ctx.classify(D.make_reads(recs))
    check_run(D, ctx, T, tax, res, len(recs), ref_tids(idx), 0.5, "0.5")
    assert ctx.lca().tobytes() != one.tobytes()
    # set_taxonomy(None) while on: off, and freed
    ctx.set_taxonomy(None)
    for call in (ctx.lca, ctx.lca_counts, ctx.reset_lca, ctx.enable_lca):
        with pytest.raises(D.DsbError) as e:
            call()
        assert e.value.code == D.DSB_EINVAL
    ctx.close()
    # a second identical run
    ctx = lca_ctx(D, idx, T)
    ctx.classify(D.make_reads(recs))
    assert ctx.lca().tobytes() == one.tobytes() and text(ctx) == base
    ctx.enable_lca(False)
    with pytest.raises(D.DsbError):
        ctx.lca_counts()
    ctx.close()
    # two input slots, fetched between them
    ctx = D.Ctx(idx, 0, input_slots=2)
    ctx.set_taxonomy(T); ctx.enable_lca()
    parts = [D.make_reads(recs[:150]), D.make_reads(recs[150:])]
    ctx.select_slot(0); ctx.set_history(0); ctx.upload(parts[0])
    ctx.select_slot(1); ctx.set_history(hist(150)); ctx.upload(parts[1])
    ctx.select_slot(0); ctx.run(); ctx.fetch()
    first = ctx.lca()
    assert ctx.lca_counts()[1]["reads"] == 150
    ctx.select_slot(1); ctx.run(); ctx.fetch()
    assert np.concatenate([first, ctx.lca()]).tobytes() == one.tobytes() and text(ctx) == base
    ctx.close()
    # two contexts on one device, many chunks on both
    monkeypatch.setenv("DSB_SHARD_CHUNK_READS", "30")
    m = D.Multi(idx, [0, 0])
    with pytest.raises(D.DsbError) as e:
        m.enable_lca()
    assert e.value.code == D.DSB_EINVAL
    m.set_taxonomy(T)
    with pytest.raises(D.DsbError) as e:
        m.lca_counts()
    assert e.value.code == D.DSB_EINVAL
    m.enable_lca()
    m.classify(D.make_reads(recs))
    assert min(m.last_calls()) > 0
    assert m.lca().tobytes() == one.tobytes() and text(m) == base
    m.reset_lca()
    assert m.lca_counts()[1]["reads"] == 0
    m.close()


def cli(tmp_path, files, extra=(), tag="run", env=None, index=None):
    out = tmp_path / (tag + ".out")
    e = dict(os.environ); e.update(env or {})
    p = subprocess.run([CLI, "classify"] + list(extra) + [index or os.path.join(ROOT, "data", "demo", "index")] + [str(f) for f in files] + ["-o", str(out)],
                       stderr=subprocess.PIPE, env=e)
    assert p.returncode == 0, p.stderr
    return out.read_bytes()


@pytest.mark.gpu
def test_cli_kraken_outputs_and_unchanged_outputs(env, tmp_path):
    D, idx, T, tax = env
    names_ = ["ont20k", "ngs_e14", "pb", "appc", "wrapq", "ngs150"]
    files = []
    for i, n in enumerate(names_):
        src = os.path.join(SYNTH, n + ".fq")
        if i % 2:
            dst = tmp_path / (n + ".fq.gz")
            with gzip.open(dst, "wb") as f:
                f.write(open(src, "rb").read())
            files.append(dst)
        else:
            files.append(src)
    e = {"DSB_CLI_BATCH_KB": "128"}
    old = lambda tag: ["--taxonomy", NODES, "--report", str(tmp_path / (tag + ".report")), "--coverage", str(tmp_path / (tag + ".cov")),
                       "--abundance", str(tmp_path / (tag + ".tsv"))]
    new = lambda tag: ["--kraken-out", str(tmp_path / (tag + ".kraken")), "--kraken-report", str(tmp_path / (tag + ".kreport"))]
    plain = cli(tmp_path, files, old("plain"), "plain", e)
    g0 = cli(tmp_path, files, old("g0") + new("g0") + ["--names", NAMES], "g0", e)
    g00 = cli(tmp_path, files, ["-g", "0,0"] + old("g00") + new("g00") + ["--names", NAMES], "g00", e)
    assert plain == g0 == g00 == open(os.path.join(SYNTH, "multi6.ubfree.sam"), "rb").read()
    for ext in (".report", ".cov", ".tsv"):
        assert (tmp_path / ("plain" + ext)).read_bytes() == (tmp_path / ("g0" + ext)).read_bytes() == (tmp_path / ("g00" + ext)).read_bytes() != b"", ext
    for ext in (".kraken", ".kreport"):
        assert (tmp_path / ("g0" + ext)).read_bytes() == (tmp_path / ("g00" + ext)).read_bytes() != b"", ext
    again = cli(tmp_path, files, old("again") + new("again") + ["--names", NAMES], "again", e)   # a repeated run
    assert again == g0 and all((tmp_path / ("again" + x)).read_bytes() == (tmp_path / ("g0" + x)).read_bytes() for x in (".kraken", ".kreport"))
    des = cli(tmp_path, files, ["-f", "DES_FULL"], "des", e)
    des_k = cli(tmp_path, files, ["-f", "DES_FULL", "--taxonomy", NODES, "--lca-min-frac", "1", "-r", "0"] + new("des"), "desk", e)
    assert des == des_k
    # the texts are the library's rendering of the library's numbers: the same reads through the Python API
    recs = []
    for n in names_:
        recs += D.read_fastq(os.path.join(SYNTH, n + ".fq"))
    names = D.TaxNames(NAMES)
    for frac, tag, nm in ((0.95, "g0", names), (1.0, "des", None)):
        ctx = lca_ctx(D, idx, T, frac)
        reads = D.make_reads(recs)
        res = ctx.classify(reads, strict=False)
        want = check_run(D, ctx, T, tax, res, len(recs), ref_tids(idx), frac, tag)
        assert (tmp_path / (tag + ".kraken")).read_bytes() == D.format_kraken(reads, ctx.lca()) == b"".join(
            M.kraken_line(r[0], len(r[1]), w) for r, w in zip(recs, want))
        rows, summ = ctx.lca_counts()
        rep = (tmp_path / (tag + ".kreport")).read_bytes()
        assert rep == D.format_lca_report(T, rows, summ, nm)
        # the bookkeeping: unclassified + the root's clade = reads
        lines = [ln.split(b"\t") for ln in rep.splitlines()]
        u = sum(int(ln[1]) for ln in lines if ln[3] == b"U")
        root = sum(int(ln[1]) for ln in lines if ln[3] == b"R")
        assert u + root == summ["reads"] == len(recs)
        ctx.close()
    assert b"Taxon " in (tmp_path / "g0.kreport").read_bytes() and b"Taxon " not in (tmp_path / "des.kreport").read_bytes()
    names.close()


@pytest.mark.gpu
def test_lca_edge_cases(env, tmp_path):
    import numpy as np
    D, idx, T, tax = env
    k = lambda tag: ["--taxonomy", NODES, "--kraken-out", str(tmp_path / (tag + ".kraken")), "--kraken-report", str(tmp_path / (tag + ".kreport"))]
    # an empty input
    (tmp_path / "empty.fq").write_bytes(b"")
    cli(tmp_path, [tmp_path / "empty.fq"], k("empty"), "empty")
    assert (tmp_path / "empty.kraken").read_bytes() == b"" and (tmp_path / "empty.kreport").read_bytes() == b""
    # every read unclassified
    rng = np.random.default_rng(5)
    recs = [("u%d" % i, decode(rng.integers(0, 4, 3000)), b"5" * 3000) for i in range(40)]
    with open(tmp_path / "rand.fq", "wb") as f:
        for n, s, q in recs:
            f.write(b"@" + n.encode() + b"\n" + s + b"\n+\n" + q + b"\n")
    cli(tmp_path, [tmp_path / "rand.fq"], k("rand"), "rand")
    assert (tmp_path / "rand.kreport").read_bytes() == b"100.00\t40\t40\tU\t0\tunclassified\n"
    assert (tmp_path / "rand.kraken").read_bytes() == b"".join(b"U\tu%d\t0\t3000\t0:0\n" % i for i in range(40))
    # a nodes.dmp trimmed so that some references are unrooted: every species line dropped whose taxid is odd
    lines = open(NODES).read().splitlines(True)
    kept = [ln for ln in lines if not ("species" in ln and int(ln.split("|")[0]) % 2)]
    assert len(kept) < len(lines)
    kept.append(lines[-1]) if kept[-1] != lines[-1] else None    # (the last line sets max_tid)
    (tmp_path / "trim.dmp").write_text("".join(kept))
    T2 = D.Taxonomy(str(tmp_path / "trim.dmp"))
    tax2 = M.load_nodes(str(tmp_path / "trim.dmp"))
    recs = det_reads()
    ctx = lca_ctx(D, idx, T2)
    res = ctx.classify(D.make_reads(recs))
    want = check_run(D, ctx, T2, tax2, res, len(recs), ref_tids(idx), 0.95, "trimmed")
    rows, summ = check_counts(D, ctx, T2, tax2, want, 0.95, "trimmed")
    assert summ["no_taxon"] > 0 and summ["classified"] > 0
    ctx.close(); T2.close()


@pytest.mark.gpu
def test_lca_reference_names_without_a_taxid(built, tmp_path):
    import numpy as np
    import desamba_amd as D
    from test_abundance import sample
    rng = np.random.default_rng(9)
    A, B, Cg = (rng.integers(0, 4, 30000).astype(np.uint8) for _ in range(3))
    write_fasta(str(tmp_path / "n.fa"), [("plain_name", A), ("tid|10239|virus", B), ("x|notanumber|y", Cg)])
    D.build_index(str(tmp_path / "n.fa"), str(tmp_path / "index"))
    recs = sample(rng, A, 10, 3000, 0.05, "A") + sample(rng, B, 10, 3000, 0.05, "B") + sample(rng, Cg, 10, 3000, 0.05, "C")
    idx = D.Index(str(tmp_path / "index"))
    T = D.Taxonomy(NODES)
    tax = M.load_nodes(NODES)
    ctx = lca_ctx(D, idx, T)
    res = ctx.classify(D.make_reads(recs), strict=False)
    want = check_run(D, ctx, T, tax, res, len(recs), ref_tids(idx), 0.95, "names")
    rows, summ = check_counts(D, ctx, T, tax, want, 0.95, "names")
    assert summ["no_taxon"] >= 15 and sum(1 for r in want if r[0] == 10239) >= 8
    ctx.close(); T.close(); idx.close()


# one row per forced classify path (tests/test_run_reductions.py's matrix): a launch placed too early would change these records
@pytest.mark.gpu
@pytest.mark.parametrize("row", ["baseline", "hout_cap", "step_limit", "heavy_mw"])
def test_lca_on_every_classify_path(env, tmp_path_factory, monkeypatch, row):
    from test_run_reductions import readsim
    D, idx, T, tax = env
    knobs = {"baseline": {}, "hout_cap": {"DSB_HOUT_CAP": "8"}, "step_limit": {"DSB_STEP_LIMIT_RT": "3000"},
             "heavy_mw": {"DSB_HEAVY_FIRST": "16", "DSB_HEAVY_MW": "8"}}[row]
    d = tmp_path_factory.mktemp("lca_paths")
    readsim(os.path.join(ROOT, "data", "demo", "index"), d / "ont.fq", 4096, 20000, 0.15, 8642, "ont")
    ont = D.read_fastq(str(d / "ont.fq"))
    recs = D.read_fastq(os.path.join(SYNTH, "heavy.fq")) + ont[:2000] + D.read_fastq(os.path.join(SYNTH, "manyanchors.fq")) + ont[2000:]
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    ctx = lca_ctx(D, idx, T)
    res = ctx.classify(D.make_reads(recs))
    t = ctx.timing()
    if row == "baseline":
        assert t.n_regrow == 0 and t.n_early > 0
    elif row == "hout_cap":
        assert t.n_regrow > 0                                      # the run after a regrown hit buffer
    elif row == "step_limit":
        assert t.n_retry > 0                                       # the second run
    else:
        assert t.n_early == 16 and t.n_heavy_mw == 8               # the early launch
    want = check_run(D, ctx, T, tax, res, len(recs), ref_tids(idx), 0.95, row)
    check_counts(D, ctx, T, tax, want, 0.95, row)
    ctx.close()


@pytest.mark.gpu
def test_lca_at_scale(strain, tmp_path):
    """65536 reads of 50 kbp on the strain collection: the per-read records against the model"""
    import desamba_amd as D
    from test_run_reductions import readsim
    fq = tmp_path / "scale.fq"
    readsim(strain["index"], fq, 65536, 50000, 0.12, 777, "ont")
    idx = D.Index(strain["index"])
    # a taxonomy over the collection's reference names: the k-th taxid a strain under genus 5000000 + k / 4 under family 6000000 + k / 32;
    # every seventh taxid is left out (unrooted references among the rooted ones)
    tids = sorted(set(ref_tids(idx)))
    assert len(tids) > 8 and 1 < tids[0] and tids[-1] < 5000000
    rows = {1: (1, "no rank")}
    for k, t in enumerate(tids):
        if k % 7 != 6:
            rows[t] = (5000000 + k // 4, "no rank"); rows[5000000 + k // 4] = (6000000 + k // 32, "genus"); rows[6000000 + k // 32] = (1, "family")
    (tmp_path / "nodes.dmp").write_text("".join("%d\t|\t%d\t|\t%s\t|\t\t|\n" % (t, rows[t][0], rows[t][1]) for t in sorted(rows)))
    T = D.Taxonomy(str(tmp_path / "nodes.dmp"))
    tax = M.load_nodes(str(tmp_path / "nodes.dmp"))
    ctx = D.Ctx(idx, 0, max_read_len=60000, max_batch_reads=65536)
    ctx.set_taxonomy(T); ctx.enable_lca()
    n = ctx.upload_fastq(str(fq))
    assert n == 65536
    ctx.run()
    res = ctx.fetch()
    want = check_run(D, ctx, T, tax, res, n, ref_tids(idx), 0.95, "scale")
    check_counts(D, ctx, T, tax, want, 0.95, "scale")
    print("scale: %d reads, %d with hits, %d ambiguous, %d without a taxon, largest n_pass %d" % (
        n, sum(1 for r in want if r[4]), sum(1 for r in want if r[4] & M.AMBIGUOUS), sum(1 for r in want if r[4] & M.NO_TAXON), max(r[2] for r in want)))
    assert sum(1 for r in want if r[0]) > n // 2 and sum(1 for r in want if r[4] & M.NO_TAXON) > 0
    ctx.close(); T.close(); idx.close()
