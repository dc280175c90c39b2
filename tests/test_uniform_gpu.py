"""The scalarised control flow of the classify kernels (DSB_UNI, desamba_amd/csrc/dsb_classify_dev.h) on the GPU, where a DSB_UNI is a
v_readfirstlane: the golden sets under the schedules that reach the launch forms (k_classify, k_classify_early + k_classify_heavy<8>
from the start, the hand-over to k_classify_heavy, k_classify_second after a spent loop budget, the walk inside k_classify without
k_anchor, seeds from the hit bits without k_seed_scan), partial-wave sections and lane-0 serial sections in front of a scalarised read.
Under every schedule each read's hit table equals the CPU oracle's and the SAM equals the set's golden file.

A schedule that the library ignored would pass unchanged, so the run's counters (ctx.timing()) are asserted wherever a set reaches the
form: TAKEN below.  What the golden sets cannot show -- a batch of a few reads takes neither k_seed_scan nor k_anchor by itself, so
DSB_SEED_SCAN=0 and DSB_ANCHOR_KERNEL=0 change nothing for them -- is shown twice more: the golden sets with the seed-list path forced
(SEED_LIST), and a batch of 4099 reads (heavy.fq, 4096 fresh 20-kbp reads, manyanchors.fq) that takes every path by itself, each
schedule with its counter and the default schedule's records."""
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

SETS = ["heavy", "manyanchors", "ont5k_e25", "ngs150"]
SCHEDULES = {
    "default": {},
    "heavy_first": {"DSB_HEAVY_FIRST": "16", "DSB_HEAVY_MW": "8"},
    "heavy_handover": {"DSB_HEAVY_PREDS": "20000", "DSB_HEAVY_FIRST": "8", "DSB_HEAVY_MW": "4"},
    "second_run": {"DSB_STEP_LIMIT_RT": "3000"},
    "no_anchor_kernel": {"DSB_ANCHOR_KERNEL": "0"},
    "no_seed_scan": {"DSB_SEED_SCAN": "0"},
}
# the seed-list path forced on the small sets: k_seed_scan and k_anchor in front of k_classify (ngs150: 64 reads per work item), and
# k_seed_scan alone
SEED_LIST = {
    "seed_lists": {"DSB_SEED_SCAN": "1"},
    "seed_lists_no_anchor_kernel": {"DSB_SEED_SCAN": "1", "DSB_ANCHOR_KERNEL": "0"},
}
# (schedule, set) -> what the run's counters must show: the sets that reach the form (a batch of one read has no early launch; the
# short and the 5-kbp reads neither run out of 3000 loop steps nor scan 20000 predecessors)
TAKEN = {
    ("heavy_first", "heavy"): lambda t: t.n_early > 0 and t.n_heavy_mw > 0,
    ("heavy_first", "ont5k_e25"): lambda t: t.n_early > 0 and t.n_heavy_mw == 8,
    ("heavy_first", "ngs150"): lambda t: t.n_early == 16 and t.n_heavy_mw == 8,
    ("heavy_handover", "heavy"): lambda t: t.n_requeue > 0,
    ("heavy_handover", "manyanchors"): lambda t: t.n_requeue > 0,
    ("second_run", "heavy"): lambda t: t.n_retry > 0,
    ("second_run", "manyanchors"): lambda t: t.n_retry > 0,
}
for _s in SETS:
    TAKEN[("seed_lists", _s)] = lambda t: t.seed_scan == 1
    TAKEN[("seed_lists_no_anchor_kernel", _s)] = lambda t: t.seed_scan == 1 and t.anc_pool_asked == 0
    TAKEN[("no_seed_scan", _s)] = lambda t: t.seed_scan == 0
    TAKEN[("no_anchor_kernel", _s)] = lambda t: t.anc_pool_asked == 0


@pytest.fixture(scope="module")
def gpu(demo):
    import desamba_amd as D
    idx = D.Index(demo["index"])
    ctx = D.Ctx(idx, 0)
    yield D, idx, ctx
    ctx.close(); idx.close()


@pytest.fixture(scope="module")
def expected(oracle):
    """per set, once: the reads, the oracle's hit table of every read and the golden SAM"""
    import desamba_amd as D
    out = {}
    for name in SETS:
        recs = D.read_fastq(os.path.join(GOLDEN, "synth", name + ".fq"))
        hits, hist = [], 0
        for rname, seq, q in recs:
            hits.append(oracle.classify(seq, hist))
            hist = max(hist, len(seq))
        out[name] = (recs, hits, open(os.path.join(GOLDEN, "synth", name + ".ubfree.sam"), "rb").read())
    return out


def run_under(D, ctx, recs, env, monkeypatch):
    """-> (hit table per read, records, SAM, the run's counters)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        ctx.reset_history(); ctx.reload_env()
        res = ctx.classify(D.make_reads(recs))
        t = ctx.timing()
        hits = [[res.hits[res.reads[i].first + k].key() for k in range(res.reads[i].n)] for i in range(len(recs))]
        rows = [(res.reads[i].status, res.reads[i].n_anc) for i in range(len(recs))]
        sam = ctx.sam(res)
    finally:
        for k in env:
            monkeypatch.delenv(k)
        ctx.reload_env()
    return hits, rows, sam, t


@pytest.mark.parametrize("schedule", list(SCHEDULES) + list(SEED_LIST))
@pytest.mark.parametrize("name", SETS)
def test_golden_set_under_schedule(gpu, expected, name, schedule, monkeypatch):
    D, idx, ctx = gpu
    recs, exp_hits, exp_sam = expected[name]
    got, rows, sam, t = run_under(D, ctx, recs, {**SCHEDULES, **SEED_LIST}[schedule], monkeypatch)
    print("%s %s: n_early %d n_heavy_mw %d n_retry %d n_requeue %d seed_scan %d anc_pool_asked %d" % (name, schedule, t.n_early, t.n_heavy_mw, t.n_retry, t.n_requeue, t.seed_scan, t.anc_pool_asked))
    if (schedule, name) in TAKEN:
        assert TAKEN[(schedule, name)](t), (schedule, name)
    for i in range(len(recs)):
        assert got[i] == exp_hits[i], (name, schedule, recs[i][0])
    assert sam == exp_sam


@pytest.fixture(scope="module")
def long_batch(gpu, demo, tmp_path_factory):
    """heavy.fq, 4096 fresh ONT 20-kbp reads, manyanchors.fq among them (the early launch and the seed-list path need a batch of 4096 reads),
    and the default schedule's result: the reference of the other schedules, computed once"""
    D, idx, ctx = gpu
    fq = tmp_path_factory.mktemp("uniform") / "ont.fq"
    subprocess.check_call([os.path.join(ROOT, "tools", "readsim"), demo["index"], str(fq), "4096", "20000", "0.15", "8642", "ont"], stdout=subprocess.DEVNULL)
    ont = D.read_fastq(str(fq))
    synth = os.path.join(GOLDEN, "synth")
    recs = D.read_fastq(os.path.join(synth, "heavy.fq")) + ont[:2000] + D.read_fastq(os.path.join(synth, "manyanchors.fq")) + ont[2000:]
    ctx.reset_history(); ctx.reload_env()
    res = ctx.classify(D.make_reads(recs))
    t = ctx.timing()
    assert t.seed_scan == 1 and t.anc_pool_asked > 0 and t.n_early > 0       # by itself: k_seed_scan, k_anchor, the early launch
    hits = [[res.hits[res.reads[i].first + k].key() for k in range(res.reads[i].n)] for i in range(len(recs))]
    assert sum(1 for h in hits if h) > 4000
    return recs, hits, ctx.sam(res)


LONG_TAKEN = {
    "heavy_first": lambda t: t.n_early == 16 and t.n_heavy_mw == 8,
    "heavy_handover": lambda t: t.n_requeue > 0,
    "second_run": lambda t: t.n_retry > 0,
    "no_anchor_kernel": lambda t: t.seed_scan == 1 and t.anc_pool_asked == 0,
    "no_seed_scan": lambda t: t.seed_scan == 0 and t.anc_pool_asked == 0,
}


@pytest.mark.parametrize("schedule", list(LONG_TAKEN))
def test_long_batch_under_schedule(gpu, long_batch, schedule, monkeypatch):
    """every schedule takes effect (its counter) and gives the default schedule's hit tables and SAM"""
    D, idx, ctx = gpu
    recs, exp_hits, exp_sam = long_batch
    got, rows, sam, t = run_under(D, ctx, recs, SCHEDULES[schedule], monkeypatch)
    assert LONG_TAKEN[schedule](t), (schedule, t.n_early, t.n_heavy_mw, t.n_retry, t.n_requeue, t.seed_scan, t.anc_pool_asked)
    assert got == exp_hits
    assert sam == exp_sam
