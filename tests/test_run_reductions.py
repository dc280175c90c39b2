"""The run-wide results of classify -- per-read taxa (k_read_taxon), per-reference coverage (k_ref_cover / k_cover_count) and
abundance (k_em_collect and the EM chain) -- on every classify path of dsb_batch_run, and the EM at scale.

All three read the hit buffer after the batch's classify launches, under the same rule as dsb_batch_fetch (counters[1] and
cap_hout).  A path that launched one of them too early, or handed it a stale capacity, would change their results but not the
SAM.  So each row of the matrix forces one path (and asserts, by its counter, that the path was taken), and checks all three
against the host yardsticks of tests/reductions_lib.py over the run's own hits, and bitwise against the baseline row."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from reductions_lib import (accumulate, check_against, classes_of, counted_records, em, nodes_table,
                            sets_from_result, walk_golden_sam)

SYNTH = os.path.join(GOLDEN, "synth")
NODES = os.path.join(GOLDEN, "analysis", "nodes.dmp")
CLI = os.path.join(ROOT, "desamba_amd", "bin", "deSAMBA")
FIELDS = ("numreads", "covbases", "aligned_bases", "mapq_sum")


def as_tuples(cov):
    return [tuple(int(x[f]) for f in FIELDS) for x in cov]


def ref_table(idx):
    n = idx.n_ref
    return [idx.ref_name(r) for r in range(n)], [idx.ref_len(r) for r in range(n)]


# ---------------------------------------------------------------- deterministic generators (tested on the CPU below)

def _decode(codes):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.asarray(codes, dtype=np.int64)].tobytes()


def _family(rng, K, with_core):
    """a 900-bp core and K members, each a random interval of >= 150 bp of it between random flanks (300 - 900 bp in all); with_core:
    the core itself is a member too (the hub: every subset of members that tie on a read of the core holds it)"""
    core = rng.integers(0, 4, 900).astype(np.uint8)
    out = [core] if with_core else []
    for _ in range(K):
        a = int(rng.integers(0, 751))
        b = a + int(rng.integers(150, 900 - a + 1))
        lo = max(0, 300 - (b - a))
        f = int(rng.integers(lo, 900 - (b - a) + 1))
        left = int(rng.integers(0, f + 1))
        out.append(np.concatenate([rng.integers(0, 4, left).astype(np.uint8), core[a:b], rng.integers(0, 4, f - left).astype(np.uint8)]))
    return core, out


def scale_refs(seed=20261016, n_solo=78200, n_fam=200, fam_k=8, hub_k=200):
    """-> (refs: [(kind, codes)], cores: {family number: core}); kind: ("solo", i) / ("fam", f, k) / ("hub", 0, k); family 0 is the hub
    family (its member 0 is the core).  Solo lengths 300 - 900, skewed short (many references to a 1024-word coverage chunk)."""
    rng = np.random.default_rng(seed)
    refs, cores = [], {}
    core, mem = _family(rng, hub_k, True)
    cores[0] = core
    refs += [(("hub", 0, k), m) for k, m in enumerate(mem)]
    for f in range(1, n_fam + 1):
        core, mem = _family(rng, fam_k, False)
        cores[f] = core
        refs += [(("fam", f, k), m) for k, m in enumerate(mem)]
    lens = 300 + (600 * rng.random(n_solo) ** 2).astype(np.int64)
    for i in range(n_solo):
        refs.append((("solo", i), rng.integers(0, 4, int(lens[i])).astype(np.uint8)))
    order = rng.permutation(len(refs))                  # (families spread over the ref_ID range)
    return [refs[i] for i in order], cores


def scale_taxids(refs, seed=7):
    """-> (taxid per reference, nodes.dmp text).  Two chains of 2600 taxa under the root; hub-family and family members sit on
    them (a few deep, most near the top), solo references on leaves hung off them; 5 % of the family members carry a taxid
    above max_tid (= the last line's taxid + 1 000 000)."""
    rng = np.random.default_rng(seed)
    D = 2600
    lines = ["1\t|\t1\t|\tno rank\t|\n"]
    chain = [[100000 + c * 10000 + i for i in range(D)] for c in range(2)]
    for c in range(2):
        for i, t in enumerate(chain[c]):
            lines.append("%d\t|\t%d\t|\tno rank\t|\n" % (t, 1 if i == 0 else chain[c][i - 1]))
    leaf = 300000
    tids = []
    for kind, _ in refs:
        if kind[0] == "solo":
            c, d = int(rng.integers(0, 2)), int(rng.integers(0, D))
            lines.append("%d\t|\t%d\t|\tspecies\t|\n" % (leaf, chain[c][d]))
            tids.append(leaf); leaf += 1
            continue
        u = rng.random()
        c = 0 if kind[0] == "hub" else int(rng.integers(0, 2))
        if u < 0.05:
            tids.append(3000000 + len(tids))                    # above max_tid
        elif u < 0.15 or (kind[0] == "hub" and kind[2] == 0):
            tids.append(chain[c][int(rng.integers(2000, D))])   # deep: walks of thousands of steps
        else:
            tids.append(chain[c][int(rng.integers(0, 12))])
    return tids, "".join(lines)


def write_scale_fasta(path, refs, tids):
    with open(path, "wb") as f:
        for r, ((kind, codes), t) in enumerate(zip(refs, tids)):
            f.write(b">tid|%d|%s\n" % (t, "_".join(str(x) for x in kind).encode()))
            s = _decode(codes)
            for k in range(0, len(s), 80):
                f.write(s[k:k + 80] + b"\n")


def scale_reads(refs, cores, seed=11, hub_reads=1000, fam_reads=5):
    """150-bp exact reads, either strand: one per solo reference, fam_reads from each family core, hub_reads from the hub core"""
    rng = np.random.default_rng(seed)
    out = []

    def take(codes, tag):
        s = int(rng.integers(0, len(codes) - 150 + 1))
        c = codes[s:s + 150]
        if rng.random() < 0.5:
            c = 3 - c[::-1]
        out.append(("%s_%d" % (tag, len(out)), _decode(c), b"5" * 150))
    for kind, codes in refs:
        if kind[0] == "solo":
            take(codes, "solo")
    for f, core in sorted(cores.items()):
        for _ in range(hub_reads if f == 0 else fam_reads):
            take(core, "fam%d" % f)
    order = rng.permutation(len(out))
    return [out[i] for i in order]


def chunk_spans(lens, words=1024):
    """the most references one k_cover_count chunk of `words` bitmap words touches (each reference from a word boundary)"""
    off = np.concatenate([[0], np.cumsum([(L + 63) // 64 for L in lens])])
    first = off[:-1] // words
    last = (off[1:] - 1) // words
    cnt = np.zeros(int(last.max()) + 1, dtype=np.int64)
    np.add.at(cnt, first, 1)
    spans = last > first
    for a, b in zip(first[spans], last[spans]):
        cnt[a + 1:b + 1] += 1
    return int(cnt.max())


# ---------------------------------------------------------------- host side (no GPU)

def test_scale_generators_are_deterministic_and_shaped():
    a, ca = scale_refs(n_solo=2000, n_fam=6)
    b, cb = scale_refs(n_solo=2000, n_fam=6)
    h = lambda refs: hashlib.md5(b"".join(_decode(c) + repr(k).encode() for k, c in refs)).hexdigest()
    assert h(a) == h(b) and all((ca[f] == cb[f]).all() for f in ca)
    assert all(300 <= len(c) <= 900 for _, c in a)
    by = {k: c for k, c in a}
    assert (by[("hub", 0, 0)] == ca[0]).all()
    # every family member holds an interval of >= 150 bp of its core
    for (kind, codes) in a:
        if kind[0] in ("hub", "fam") and not (kind[0] == "hub" and kind[2] == 0):
            core, dm = _decode(ca[kind[1]]), _decode(codes)
            assert any(core[s:s + 150] in dm for s in range(0, 751)), kind
    tids, nodes = scale_taxids(a)
    assert (tids, nodes) == scale_taxids(b)
    r1, r2 = scale_reads(a, ca), scale_reads(b, cb)
    assert r1 == r2 and len(r1) == 2000 + 1000 + 6 * 5 and all(len(s) == 150 for _, s, _ in r1)
    assert chunk_spans([64] * 3000) == 1024 and chunk_spans([65] * 10) == 10 and chunk_spans([100, 64 * 1024, 7]) == 2


def test_scale_taxonomy_shape(built, tmp_path):
    import desamba_amd as D
    refs, _ = scale_refs(n_solo=3000, n_fam=20)
    tids, nodes = scale_taxids(refs)
    (tmp_path / "nodes.dmp").write_text(nodes)
    T = D.Taxonomy(str(tmp_path / "nodes.dmp"))           # (no cycle: the loader refuses one)
    table = nodes_table(str(tmp_path / "nodes.dmp"))
    assert T.max_tid == int(nodes.splitlines()[-1].split("|")[0]) + 1000000

    def depth(t):
        d = 0
        while t != 1:
            t = table[t]; d += 1
        return d
    known = [t for t in tids if t <= T.max_tid]
    assert all(T.parent(t) == table[t] for t in known[:500])
    assert max(depth(t) for t in known) >= 2000
    assert sum(t > T.max_tid for t in tids) > 0
    T.close()


def test_walker_on_a_run_s_sam_and_deep_chains():
    """walk_golden_sam on SAM bytes: ties in AS walk to the deepest descendant; a taxid above max_tid is skipped (first record: 0)"""
    D = 2500
    table = {1: 1}
    for i in range(D):
        table[10 + i] = 1 if i == 0 else 9 + i
    table[5000] = 1
    rec = lambda q, tid, score, flag=0: b"%s\t%d\ttid|%d|x\t1\t30\t150M\t*\t0\t0\t*\t*\tAS:i:%d\n" % (q, flag, tid, score)
    sam = (rec(b"a", 10 + 100, 200) + rec(b"a", 10 + 2400, 200, 256) + rec(b"a", 5000, 200, 256) +      # deeper on the chain: taken
           rec(b"b", 10 + 2400, 200) + rec(b"b", 10 + 100, 200, 256) +                                   # an ancestor: not taken
           rec(b"c", 10 + 50, 200) + rec(b"c", 10 + 2000, 199, 256) +                                    # lower score: not taken
           rec(b"d", 9000000, 200) + rec(b"d", 10, 200, 256) +                                           # above max_tid first: 0
           rec(b"e", 10, 0) + rec(b"e", 10 + 9, 0, 256) +                                                # no score: no walk
           b"f\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\tAS:i:0\n")
    assert walk_golden_sam(sam, table, 1000000) == [10 + 2400, 10 + 2400, 10 + 50, 0, 10, 0]


def stop_tols(chg, js):
    """{j: tol} such that the first iteration whose change is below tol is j (1-based), tol at the geometric mean of that change
    and the smallest change before it; j's that no tol isolates by a clear margin are left out"""
    out = {}
    for j in js:
        if j > len(chg):
            continue
        prev = min(chg[:j - 1]) if j > 1 else 2.0 * chg[0]
        if chg[j - 1] > 0 and prev > chg[j - 1] * (1 + 1e-6):
            out[j] = (prev * chg[j - 1]) ** 0.5
    return out


def test_stop_tols():
    chg = [8.0, 4.0, 4.0, 1.0, 2.0, 0.5]
    t = stop_tols(chg, [1, 2, 3, 4, 5, 6, 7])
    assert sorted(t) == [1, 2, 4, 6]
    for j, tol in t.items():
        assert next(i + 1 for i, c in enumerate(chg) if c < tol) == j
    assert t[4] == 2.0 and t[6] == (1.0 * 0.5) ** 0.5


# ---------------------------------------------------------------- on the GPU: every classify path, all three consumers

def readsim(index, path, n, length, err, seed, prof):
    subprocess.check_call([os.path.join(ROOT, "tools", "readsim"), index, str(path), str(n), str(length), str(err), str(seed), prof])


@pytest.fixture(scope="module")
def sets_(demo, tmp_path_factory):
    """long: heavy.fq first (its golden SAM is the first lines), 4096 fresh ONT 20-kbp reads, manyanchors.fq among them;
    short: ngs150.fq first, then 6000 fresh 150-bp reads"""
    import desamba_amd as D
    d = tmp_path_factory.mktemp("reductions")
    readsim(demo["index"], d / "ont.fq", 4096, 20000, 0.15, 8642, "ont")
    readsim(demo["index"], d / "ngs.fq", 6000, 150, 0.02, 8643, "ngs")
    ont = D.read_fastq(str(d / "ont.fq"))
    heavy = D.read_fastq(os.path.join(SYNTH, "heavy.fq"))
    many = D.read_fastq(os.path.join(SYNTH, "manyanchors.fq"))
    long_ = heavy + ont[:2000] + many + ont[2000:]
    short = D.read_fastq(os.path.join(SYNTH, "ngs150.fq")) + D.read_fastq(str(d / "ngs.fq"))
    assert len(long_) >= 4096 and len(short) >= 6000
    return {"long": (long_, "heavy"), "short": (short, "ngs150")}


@pytest.fixture(scope="module")
def env(demo):
    import desamba_amd as D
    idx = D.Index(demo["index"])
    T = D.Taxonomy(NODES)
    yield D, idx, T, nodes_table(NODES)
    T.close(); idx.close()


def make_ctx(D, idx, T, max_sec_N=5, **kw):
    ctx = D.Ctx(idx, 0, max_sec_N=max_sec_N, **kw)
    ctx.set_taxonomy(T); ctx.enable_coverage(); ctx.enable_abundance(min_frac=0.95)
    return ctx


def outputs(D, idx, runner, reads, res, max_sec_N=5):
    cov = runner.coverage()
    ab, summ = runner.abundance(max_iter=200, tol=0)
    return {"sam": D.format_sam(idx, reads, res, max_sec_N), "cov": cov, "ab": ab, "summ": summ, "taxa": runner.taxa(), "res": res}


def check_outputs(idx, lens, table, T, o, n, label, max_sec_N=5):
    """3. - 5.: coverage, abundance and taxa against the host yardsticks over the run's own hits and SAM"""
    res = o["res"]
    assert as_tuples(o["cov"]) == accumulate(idx.n_ref, counted_records(res, n), lens), label
    check_against(o["ab"], o["summ"], sets_from_result(res, n, idx.n_ref, 950), lens, label)
    assert o["summ"]["reads"] == n, label
    assert len(o["taxa"]) == n and list(o["taxa"]) == walk_golden_sam(o["sam"], table, T.max_tid), label


def same_as(o, base, label):
    """2. and 6.: the SAM, and the three results bitwise, equal the baseline row's"""
    assert o["sam"] == base["sam"], label
    assert o["cov"].tobytes() == base["cov"].tobytes(), label
    assert o["ab"].tobytes() == base["ab"].tobytes() and o["summ"] == base["summ"], label
    assert o["taxa"].tobytes() == base["taxa"].tobytes(), label


def run_ctx(D, idx, T, recs, max_sec_N=5, **kw):
    ctx = make_ctx(D, idx, T, max_sec_N, **kw)
    reads = D.make_reads(recs)
    res = ctx.classify(reads)
    o = outputs(D, idx, ctx, reads, res, max_sec_N)
    o["t"] = ctx.timing()
    o["ctx"] = ctx                                    # (the hits live in the ctx: closed by the caller)
    return o


@pytest.fixture(scope="module")
def baseline(env, sets_):
    D, idx, T, table = env
    names, lens = ref_table(idx)
    out = {}
    for key, (recs, gold) in sets_.items():
        o = run_ctx(D, idx, T, recs)
        check_outputs(idx, lens, table, T, o, len(recs), key + " baseline")
        g = open(os.path.join(SYNTH, gold + ".ubfree.sam"), "rb").read()
        assert o["sam"][:len(g)] == g, key
        t = o["t"]
        assert t.seed_scan == 1, key
        if key == "long":
            assert t.n_early > 0 and t.anc_pool_asked > 0          # the early launch and k_anchor are real on this set
        else:
            assert t.anc_pool_asked == 0                             # group mode: its own anchor stage, no k_anchor
        assert o["summ"]["classes"] > 10 and sum(o["cov"]["numreads"]) > len(recs) // 2
        o["ctx"].close(); o.pop("ctx")
        out[key] = o
    return out


# (row, knobs, taken(t, b)): t the row's timing, b the baseline's -- each check fails if the knobs were ignored
ROWS = [
    ("hout_cap", {"DSB_HOUT_CAP": "8"}, lambda t, b: t.n_regrow > 0 == b.n_regrow),
    ("step_limit", {"DSB_STEP_LIMIT_RT": "3000"}, lambda t, b: t.n_retry > b.n_retry),   # (300 and 96: 20-kbp reads outgrow even the second run)
    ("anc_cap", {"DSB_ANC_CAP_RT": "64"}, lambda t, b: t.n_retry > b.n_retry),
    ("sms_cap", {"DSB_SMS_CAP": "4096"}, lambda t, b: t.n_retry > b.n_retry),
    ("heavy_mw", {"DSB_HEAVY_FIRST": "16", "DSB_HEAVY_MW": "8"},                          # (by default n / 64 early, 16 of them on eight wavefronts)
     lambda t, b: t.n_early == 16 != b.n_early and t.n_heavy_mw == 8 != b.n_heavy_mw),
    ("heavy_preds", {"DSB_HEAVY_PREDS": "5000"}, lambda t, b: t.n_requeue > b.n_requeue),
    ("no_anchor_kernel", {"DSB_ANCHOR_KERNEL": "0"}, lambda t, b: t.anc_pool_asked == 0 < b.anc_pool_asked and t.seed_scan == 1),
    ("anchor_pool", {"DSB_ANC_POOL_RT": "20000"}, lambda t, b: t.anc_pool_cap == 20000 != b.anc_pool_cap and t.anc_pool_asked > 20000),
    ("hit_bits", {"DSB_SEED_SCAN": "0"}, lambda t, b: t.seed_scan == 0 != b.seed_scan),
]


@pytest.mark.gpu
@pytest.mark.parametrize("row", [r[0] for r in ROWS])
def test_path_row(env, sets_, baseline, monkeypatch, row):
    D, idx, T, table = env
    _, knobs, taken = next(r for r in ROWS if r[0] == row)
    names, lens = ref_table(idx)
    recs = sets_["long"][0]
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    o = run_ctx(D, idx, T, recs)
    try:
        assert taken(o["t"], baseline["long"]["t"]), row
        check_outputs(idx, lens, table, T, o, len(recs), row)
        same_as(o, baseline["long"], row)
    finally:
        o["ctx"].close()


@pytest.mark.gpu
def test_seed_lists_row(env, sets_, baseline, monkeypatch):
    """DSB_SEED_SCAN=1 on batches below 2048 reads, which take the hit bits by default: three batches whose results add up to the
    baseline's single batch"""
    D, idx, T, table = env
    names, lens = ref_table(idx)
    recs = sets_["long"][0]
    monkeypatch.setenv("DSB_SEED_SCAN", "1")
    ctx = make_ctx(D, idx, T)
    try:
        cuts = [0, 1400, 2800, len(recs)]
        assert max(b - a for a, b in zip(cuts, cuts[1:])) < 2048
        sam, taxa, records, sets = [], [], [], []
        for a, b in zip(cuts, cuts[1:]):
            ctx.set_history(max([len(x[1]) for x in recs[:a]], default=0))
            reads = D.make_reads(recs[a:b])
            res = ctx.classify(reads)
            assert ctx.timing().seed_scan == 1, a
            sam.append(D.format_sam(idx, reads, res, 5))
            tx = ctx.taxa()
            assert list(tx) == walk_golden_sam(sam[-1], table, T.max_tid), a
            taxa.append(tx)
            records += counted_records(res, b - a)
            sets += sets_from_result(res, b - a, idx.n_ref, 950)
        cov = ctx.coverage()
        ab, summ = ctx.abundance(max_iter=200, tol=0)
        assert as_tuples(cov) == accumulate(idx.n_ref, records, lens)
        check_against(ab, summ, sets, lens, "seed_lists")
        o = {"sam": b"".join(sam), "cov": cov, "ab": ab, "summ": summ, "taxa": np.concatenate(taxa)}
        same_as(o, baseline["long"], "seed_lists")
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("row", ["baseline", "hout_cap"])
def test_taxa_for_other_max_sec(env, sets_, monkeypatch, row):
    """k_read_taxon walks the first max_sec_N + 1 records of a read (c->opts.max_sec_N): 0, 1, 5 and 100 against the walker over the
    SAM of that max_sec_N"""
    D, idx, T, table = env
    recs = sets_["long"][0]
    if row == "hout_cap":
        monkeypatch.setenv("DSB_HOUT_CAP", "8")
    for ms in (0, 1, 5, 100):
        ctx = D.Ctx(idx, 0, max_sec_N=ms)
        ctx.set_taxonomy(T)
        reads = D.make_reads(recs)
        res = ctx.classify(reads)
        if row == "hout_cap":
            assert ctx.timing().n_regrow > 0
        got = list(ctx.taxa())
        assert got == walk_golden_sam(D.format_sam(idx, reads, res, ms), table, T.max_tid), (row, ms)
        ctx.close()


@pytest.mark.gpu
def test_group_mode_row(env, sets_, baseline, monkeypatch):
    D, idx, T, table = env
    names, lens = ref_table(idx)
    recs = sets_["short"][0]
    monkeypatch.setenv("DSB_NO_GROUP", "1")
    o = run_ctx(D, idx, T, recs)
    try:
        assert o["t"].seed_scan == 1 and o["t"].anc_pool_asked > 0       # one read per wavefront: k_anchor runs
        check_outputs(idx, lens, table, T, o, len(recs), "no_group")
        same_as(o, baseline["short"], "no_group")
    finally:
        o["ctx"].close()


@pytest.mark.gpu
def test_input_slots_row(env, sets_, baseline, monkeypatch):
    """two batches staged at once, the hit buffer regrown in the first (the second runs in the buffer it grew); coverage and
    abundance fetched between the slots"""
    D, idx, T, table = env
    names, lens = ref_table(idx)
    recs = sets_["long"][0]
    monkeypatch.setenv("DSB_HOUT_CAP", "8")
    ctx = make_ctx(D, idx, T, input_slots=2)
    try:
        cut = 1500
        parts = [D.make_reads(recs[:cut]), D.make_reads(recs[cut:])]
        ctx.select_slot(0); ctx.set_history(0); ctx.upload(parts[0])
        ctx.select_slot(1); ctx.set_history(max(len(x[1]) for x in recs[:cut])); ctx.upload(parts[1])
        ctx.select_slot(0); ctx.run(); r0 = ctx.fetch()
        assert ctx.timing().n_regrow > 0
        mid_cov = ctx.coverage()
        mid_ab, mid_s = ctx.abundance(max_iter=200, tol=0)
        t0 = list(ctx.taxa())
        o0 = {"res": r0, "cov": mid_cov, "ab": mid_ab, "summ": mid_s, "taxa": np.array(t0, dtype=np.uint32), "sam": D.format_sam(idx, parts[0], r0, 5)}
        check_outputs(idx, lens, table, T, o0, cut, "slot 0")
        sam0 = o0["sam"]
        ctx.select_slot(1); ctx.run(); r1 = ctx.fetch()
        sam1 = D.format_sam(idx, parts[1], r1, 5)
        t1 = list(ctx.taxa())
        assert sam0 + sam1 == baseline["long"]["sam"]
        assert t0 + t1 == list(baseline["long"]["taxa"])
        assert ctx.coverage().tobytes() == baseline["long"]["cov"].tobytes()
        ab, s = ctx.abundance(max_iter=200, tol=0)
        assert ab.tobytes() == baseline["long"]["ab"].tobytes() and s == baseline["long"]["summ"]
        assert mid_cov.tobytes() != baseline["long"]["cov"].tobytes()
    finally:
        ctx.close()


def multi(D, idx, T):
    m = D.Multi(idx, [0, 0])
    m.set_taxonomy(T); m.enable_coverage(); m.enable_abundance(min_frac=0.95)
    return m


def ctx_timing(D, m, i):
    t = D.DsbTiming()
    D.lib().dsb_batch_timing(D.lib().dsb_multi_ctx(m.h, i), D.C.byref(t))
    return t


@pytest.mark.gpu
def test_multi_row(env, sets_, baseline, monkeypatch):
    D, idx, T, table = env
    names, lens = ref_table(idx)
    recs = sets_["long"][0]
    monkeypatch.setenv("DSB_SHARD_CHUNK_READS", "30"); monkeypatch.setenv("DSB_HOUT_CAP", "8")
    m = multi(D, idx, T)
    try:
        reads = D.make_reads(recs)
        res = m.classify(reads)
        assert min(m.last_calls()) > 0
        assert all(ctx_timing(D, m, i).n_regrow > 0 for i in range(2))
        o = outputs(D, idx, m, reads, res)
        check_outputs(idx, lens, table, T, o, len(recs), "multi")
        same_as(o, baseline["long"], "multi")
    finally:
        m.close()


@pytest.mark.gpu
def test_multi_one_read_row(env, sets_):
    """one read for two contexts: the other context's store, bitmap and taxa stay empty and change nothing"""
    D, idx, T, table = env
    names, lens = ref_table(idx)
    recs = sets_["long"][0][5:6]
    one = run_ctx(D, idx, T, recs)
    one["ctx"].close()
    m = multi(D, idx, T)
    try:
        reads = D.make_reads(recs)
        res = m.classify(reads)
        assert sorted(m.last_calls()) == [0, 1]
        o = outputs(D, idx, m, reads, res)
        check_outputs(idx, lens, table, T, o, 1, "multi one read")
        assert o["summ"]["classified"] == 1
        same_as(o, one, "multi one read")
    finally:
        m.close()


@pytest.mark.gpu
def test_strain_hand_over_row(strain, monkeypatch):
    """the hand-over to k_classify_heavy<8> where its multi-wave DP pass does real work: against the same reads without it"""
    import desamba_amd as D
    idx = D.Index(strain["index"])
    T = D.Taxonomy(NODES)
    table = nodes_table(NODES)
    names, lens = ref_table(idx)
    recs = D.read_fastq(strain["fastq"])
    try:
        monkeypatch.setenv("DSB_HEAVY_PREDS", "0")                      # (some reads of this set are handed over by default)
        base = run_ctx(D, idx, T, recs)
        assert base["t"].n_requeue == 0 and base["sam"] == open(strain["sam"], "rb").read()
        check_outputs(idx, lens, table, T, base, len(recs), "strain")
        base["ctx"].close()
        monkeypatch.setenv("DSB_HEAVY_PREDS", "20000"); monkeypatch.setenv("DSB_HEAVY_FIRST", "8"); monkeypatch.setenv("DSB_HEAVY_MW", "4")
        o = run_ctx(D, idx, T, recs)
        assert o["t"].n_requeue > len(recs) // 4 and o["t"].n_heavy_mw > 0
        check_outputs(idx, lens, table, T, o, len(recs), "strain hand-over")
        o["ctx"].close()
        same_as(o, base, "strain hand-over")
    finally:
        T.close(); idx.close()


# ---------------------------------------------------------------- on the GPU: the EM's stop rule and forced hash collisions

@pytest.mark.gpu
def test_em_stop_rule_at_the_block_boundaries(built, tmp_path):
    """the state after the first iteration that met tol, whatever EM_ITER_BLOCK (16) host round trips it took.  A, B = A with its
    last fifth replaced, and C: most reads of A and B tie, so the EM's change shrinks slowly, iteration after iteration"""
    import desamba_amd as D
    from test_abundance import sample, write_fasta
    rng = np.random.default_rng(424242)
    A = rng.integers(0, 4, 100000).astype(np.uint8)
    B = A.copy(); B[80000:] = rng.integers(0, 4, 20000)
    Cg = rng.integers(0, 4, 60000).astype(np.uint8)
    write_fasta(str(tmp_path / "abc.fa"), [("tid|101|A", A), ("tid|102|B", B), ("tid|103|C", Cg)])
    D.build_index(str(tmp_path / "abc.fa"), str(tmp_path / "index"))
    recs = sample(rng, A, 1400, 5000, 0.08, "A") + sample(rng, B, 600, 5000, 0.08, "B") + sample(rng, Cg, 150, 5000, 0.08, "C")
    idx = D.Index(str(tmp_path / "index"))
    names, lens = ref_table(idx)
    ctx = D.Ctx(idx, 0)
    ctx.enable_abundance(min_frac=0.95)
    try:
        res = ctx.classify(D.make_reads(recs), strict=False)
        cl = classes_of(sets_from_result(res, len(recs), idx.n_ref, 950))
        N = sum(cl.values())
        chg = []
        em(cl, lens, max_iter=40, tol=0.0, trace=chg)
        tols = stop_tols(chg, [1, 15, 16, 17, 31, 32, 33])
        assert len({15, 16, 17, 31, 32, 33} & set(tols)) >= 4, chg
        for j, tol in sorted(tols.items()):
            a, it, conv, c = em(cl, lens, max_iter=10000, tol=tol)
            assert it == j and conv
            ab, s = ctx.abundance(max_iter=10000, tol=tol)
            assert s["iterations"] == j and s["converged"] == 1, (j, s)
            assert abs(s["max_change"] - c) <= 1e-9 * c + 1e-300, (j, s["max_change"], c)
            got, exp = ab["est_reads"], N * a
            assert np.all(np.abs(got - exp) <= 1e-9 * np.abs(exp) + 1e-12), j
        for mi in (1, 15, 16, 17):
            a, it, conv, c = em(cl, lens, max_iter=mi, tol=0.0)
            ab, s = ctx.abundance(max_iter=mi, tol=0)
            assert s["iterations"] == mi and s["converged"] == 0, (mi, s)
            assert abs(s["max_change"] - c) <= 1e-9 * c + 1e-300, mi
            assert np.all(np.abs(ab["est_reads"] - N * a) <= 1e-9 * np.abs(N * a) + 1e-12), mi
    finally:
        ctx.close(); idx.close()


def hash_bits_runs(D, idx, recs, monkeypatch, max_sec_N=5, with_splits=True):
    """{bits: (ab, summ)} of one ctx per DSB_EM_HASH_BITS; for 1 and 4 bits also a three-way batch split and Multi([0, 0]), which
    must be bitwise the same; plus the hits of the 64-bit run"""
    out, res64 = {}, None
    for bits in (64, 4, 1):
        monkeypatch.setenv("DSB_EM_HASH_BITS", str(bits))
        ctx = D.Ctx(idx, 0, max_sec_N=max_sec_N)
        ctx.enable_abundance(min_frac=0.95)
        res = ctx.classify(D.make_reads(recs))
        out[bits] = ctx.abundance(max_iter=200, tol=0)
        if bits == 64:
            res64 = (ctx, sets_from_result(res, len(recs), idx.n_ref, 950))
        else:
            ctx.close()
        if bits != 64 and with_splits:
            ctx = D.Ctx(idx, 0, max_sec_N=max_sec_N)
            ctx.enable_abundance(min_frac=0.95)
            cuts = [0, len(recs) // 5, len(recs) // 2, len(recs)]
            for a, b in zip(cuts, cuts[1:]):
                ctx.set_history(max([len(x[1]) for x in recs[:a]], default=0))
                ctx.classify(D.make_reads(recs[a:b]))
            ab, s = ctx.abundance(max_iter=200, tol=0)
            ctx.close()
            assert ab.tobytes() == out[bits][0].tobytes() and s == out[bits][1], ("split", bits)
            m = D.Multi(idx, [0, 0], max_sec_N=max_sec_N)
            m.enable_abundance(min_frac=0.95)
            m.classify(D.make_reads(recs))
            ab, s = m.abundance(max_iter=200, tol=0)
            m.close()
            assert ab.tobytes() == out[bits][0].tobytes() and s == out[bits][1], ("multi", bits)
    monkeypatch.delenv("DSB_EM_HASH_BITS")
    return out, res64


def check_hash_bits(out, sets, lens, label, tiny=None):
    cl = classes_of(sets)
    for bits, (ab, s) in out.items():
        check_against(ab, s, sets, lens, "%s %d bits" % (label, bits), tiny)       # classes = distinct sets, counts exact, 1e-9 of numpy
        assert s["classes"] == len(cl)
    e64 = out[64][0]["est_reads"]
    for bits in (1, 4):
        e = out[bits][0]["est_reads"]
        assert (out[bits][0]["numreads"] == out[64][0]["numreads"]).all()
        assert np.all(np.abs(e - e64) <= 1e-12 * np.abs(e64)), (label, bits)


@pytest.mark.gpu
def test_em_forced_hash_collisions_demo(env, monkeypatch):
    D, idx, T, table = env
    names, lens = ref_table(idx)
    recs = []
    for n in ("pb", "ngs150", "ont20k", "heavy"):
        recs += D.read_fastq(os.path.join(SYNTH, n + ".fq"))
    out, (ctx, sets) = hash_bits_runs(D, idx, recs, monkeypatch)
    ctx.close()
    assert len(classes_of(sets)) > 20
    check_hash_bits(out, sets, lens, "demo")


# ---------------------------------------------------------------- on the GPU: the scale index

@pytest.fixture(scope="module")
def scale(built, tmp_path_factory):
    import desamba_amd as D
    d = tmp_path_factory.mktemp("scale")
    refs, cores = scale_refs()
    tids, nodes = scale_taxids(refs)
    write_scale_fasta(str(d / "ref.fa"), refs, tids)
    (d / "nodes.dmp").write_text(nodes)
    D.build_index(str(d / "ref.fa"), str(d / "index"))
    return {"index": str(d / "index"), "nodes": str(d / "nodes.dmp"), "reads": scale_reads(refs, cores), "dir": d}


@pytest.mark.gpu
def test_scale_index(scale, tmp_path, monkeypatch):
    import desamba_amd as D
    import oracle_lib
    from test_taxonomy_report import analysis
    idx = D.Index(scale["index"])
    T = D.Taxonomy(scale["nodes"])
    table = nodes_table(scale["nodes"])
    names, lens = ref_table(idx)
    recs = scale["reads"]
    n = len(recs)
    try:
        ctx = D.Ctx(idx, 0, max_sec_N=100)
        ctx.set_taxonomy(T); ctx.enable_coverage()
        reads = D.make_reads(recs)
        res = ctx.classify(reads)
        sets = sets_from_result(res, n, idx.n_ref, 950)
        # the shape first: of the index, of the candidate sets of its reads, and of the taxonomy
        cl = classes_of(sets)
        per_ref = np.bincount(np.concatenate([np.array(k, dtype=np.int64) for k in cl]), minlength=idx.n_ref)
        assert idx.n_ref >= 80000 and idx.n_ref > 1 << 16
        assert len(cl) > 1 << 16
        assert per_ref.max() >= 200
        assert max(len(k) for k in cl) > 64
        assert chunk_spans(lens) >= 100
        ref_tids = [int(nm.split("|")[1]) for nm in names]

        def depth(t):
            d = 0
            while t != 1:
                t = table[t]; d += 1
            return d
        assert max(depth(t) for t in set(ref_tids) if t <= T.max_tid) >= 2000
        assert sum(t > T.max_tid for t in ref_tids) > 0
        # abundance (1, 4 and 64 bits) against numpy
        out, (c64, sets64) = hash_bits_runs(D, idx, recs, monkeypatch, max_sec_N=100)
        c64.close()
        assert sets64 == sets and out[64][1]["classes"] == len(cl)
        check_hash_bits(out, sets, lens, "scale", tiny=1e-200)
        # coverage, taxa and the report of the first run
        assert as_tuples(ctx.coverage()) == accumulate(idx.n_ref, counted_records(res, n), lens)
        sam = D.format_sam(idx, reads, res, 100)
        taxa = list(ctx.taxa())
        assert taxa == walk_golden_sam(sam, table, T.max_tid)
        assert sum(1 for t in taxa if t == 0) < n // 10
        rep = D.Report(T)
        rep.add(idx, reads, res, ctx.taxa(records=True), 100)
        (tmp_path / "run.sam").write_bytes(sam)
        assert rep.text() == analysis(str(tmp_path / "run.sam"), scale["nodes"], False)
        assert rep.text(by_base=True) == analysis(str(tmp_path / "run.sam"), scale["nodes"], True)
        rep.close()
        # k_read_taxon with other max_sec_N: the hub's reads tie on dozens of references, so the walk depends on it
        seen = {100: tuple(taxa)}
        for ms in (0, 1, 5):
            c2 = D.Ctx(idx, 0, max_sec_N=ms)
            c2.set_taxonomy(T)
            r2 = c2.classify(reads)
            seen[ms] = tuple(c2.taxa())
            assert list(seen[ms]) == walk_golden_sam(D.format_sam(idx, reads, r2, ms), table, T.max_tid), ms
            c2.close()
        assert any(seen[ms] != seen[5] for ms in (0, 1, 100))
        # a sample of the hits against the oracle on this index
        import random
        ora = oracle_lib.Oracle(scale["index"])
        for i in random.Random(5).sample(range(n), 300):
            rr = res.reads[i]
            got = [res.hits[rr.first + k].key() for k in range(rr.n)]
            assert got == ora.classify(recs[i][1], 150 if i else 0), recs[i][0]
        ctx.close()
    finally:
        T.close(); idx.close()
