"""The anchor stage as a kernel of its own (k_anchor, DSB_ANCHOR_KERNEL): with it on and off, every read gets the same record
(hits, status, fast flag, anchor count) and the same hit table -- on the golden sets through the seed-list path, on a batch
of fresh 50-kbp reads large enough to take that path by itself, and with each fallback to the walk inside k_classify forced."""
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(demo):
    import desamba_amd as D
    idx = D.Index(demo["index"])
    ctx = D.Ctx(idx, 0)
    yield D, idx, ctx
    ctx.close(); idx.close()


def _records(D, ctx, recs):
    ctx.reset_history(); ctx.reload_env()
    res = ctx.classify(D.make_reads(recs))
    out = []
    for i in range(len(recs)):
        rr = res.reads[i]
        out.append((rr.status, rr.fast, rr.n_anc, [res.hits[rr.first + k].key() for k in range(rr.n)]))
    return out, ctx.sam(res)


def _both(D, ctx, recs, monkeypatch, **env):
    """records and SAM with k_anchor on and off (the other switches as given)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got = {}
    for on in ("1", "0"):
        monkeypatch.setenv("DSB_ANCHOR_KERNEL", on)
        got[on] = _records(D, ctx, recs)
    for k in list(env) + ["DSB_ANCHOR_KERNEL"]:
        monkeypatch.delenv(k)
    ctx.reload_env()
    return got["1"], got["0"]


@pytest.mark.parametrize("name", ["ont20k", "pb", "ont5k_e25", "heavy", "manyanchors"])
def test_golden_sets_same_with_and_without_anchor_kernel(gpu, name, monkeypatch):
    D, idx, ctx = gpu
    fq = os.path.join(GOLDEN, "synth", name + ".fq")
    if not os.path.exists(fq):
        pytest.fail("missing golden set " + fq)
    recs = D.read_fastq(fq)
    (a, sam_a), (b, sam_b) = _both(D, ctx, recs, monkeypatch, DSB_SEED_SCAN="1")
    assert a == b
    assert sam_a == sam_b
    assert sam_a == open(os.path.join(GOLDEN, "synth", name + ".ubfree.sam"), "rb").read()


@pytest.fixture(scope="module")
def fresh(demo, tmp_path_factory):
    import desamba_amd as D
    fq = tmp_path_factory.mktemp("anc") / "fresh.fq"
    subprocess.check_call([os.path.join(ROOT, "tools", "readsim"), demo["index"], str(fq), "2304", "50000", "0.15", "4242", "ont"])
    return D.read_fastq(str(fq))


def test_fresh_batch_same_with_and_without_anchor_kernel(gpu, fresh, monkeypatch):
    D, idx, ctx = gpu
    (a, sam_a), (b, sam_b) = _both(D, ctx, fresh, monkeypatch)
    assert a == b
    assert sam_a == sam_b
    assert sum(1 for r in a if r[3]) == len(fresh)


@pytest.mark.parametrize("knob,value", [("DSB_ANC_POOL_RT", "20000"), ("DSB_ANC_CAP_RT", "256"), ("DSB_STEP_LIMIT_RT", "3000")])
def test_fallbacks_same_with_and_without_anchor_kernel(gpu, fresh, knob, value, monkeypatch):
    """a pool too small for the batch, an anchor cap the reads outgrow and a loop budget they run out of: such reads take
    the walk inside k_classify (and, beyond the cap or budget, the second run) -- same records either way"""
    D, idx, ctx = gpu
    recs = fresh[:1024]
    (a, sam_a), (b, sam_b) = _both(D, ctx, recs, monkeypatch, DSB_SEED_SCAN="1", **{knob: value})
    assert a == b
    assert sam_a == sam_b


def test_second_index_same_with_and_without_anchor_kernel(strain, monkeypatch):
    import desamba_amd as D
    idx = D.Index(strain["index"])
    ctx = D.Ctx(idx, 0)
    try:
        recs = D.read_fastq(strain["fastq"])
        (a, sam_a), (b, sam_b) = _both(D, ctx, recs, monkeypatch, DSB_SEED_SCAN="1")
        assert a == b
        assert sam_a == sam_b
    finally:
        ctx.close(); idx.close()
