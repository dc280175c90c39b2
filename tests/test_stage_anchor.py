"""a-4 .. a-8, the anchor stage (src/cly.c:629-939, 1286-1611) on its own: the FM search, map_seed with get_new_ed, the island walks and the strand
rule, called form by form (tests/stage/dsb_stage_forms.h: stage_anchor, stage_anchor_lane) on a read's byte strands, its seed lists and a
loaded index, and compared with the oracle's ora_anchor_stage, which runs the static functions ora_classify runs.

Forms: (a) bwt_MEM_search_t on the searches of one walk in its order, fast and slow parameters, the visited-row set carried over; (b)
fast_island wave-uniform straight into the main array (the redo form of the commit); (c) fast_classify on one strand, and on the whole read
with the strand swap and the both-direction rule restated around it; (d) fast_classify_lane, one read per lane; (e) slow_classify.  Compared,
exactly: every field of every anchor in order, n_anc, the status bits, the skip flag of (b), the overflow flag of (d), for (a) the number of
MEMs and sp, match_len, sa_sp, sa_sp_l of each; the anchor regions carry a fill pattern and guards.  Also: main arrays too small for the
commit (the serial commit drops whole islands, DSB_ST_ANC_OVF), loop budgets that run out in mid-walk (DSB_ST_TIMEOUT: (b) and (e) keep
exactly the anchors of the searches and seeds that were finished; for (c) the walks run side by side, so only the status is checked),
and every case again with the set generation started in mid-range.

Two indexes: the demo index and a seeded synthetic reference of 0.5 Mbp built on the host by the product's builder stages
(stage_anchor_lib.make_reference), each opened with the 13-mer table compressed and raw and with both rank layouts.  The classes come from
the oracle's traces, never from the code under test; each has >= 50 reads in the full set and >= 5 in the 64-lane subset."""
import collections
import os
import time

import pytest

import stage_anchor_lib as A

SEED = 4108
MID_GEN = 0x7FF00                                        # far from the 20-bit wrap: a read bumps the generation a few thousand times at most
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = [(False, False), (True, False), (False, True), (True, True)]      # (13-mer table raw, rank lines with superblocks)


@pytest.fixture(scope="module")
def sets(built, demo):
    """the synthetic index (cached under data/), the reads of both indexes and the oracle's answers: once per module"""
    times = {}
    refs, info = A.make_reference(SEED)
    d = os.path.join(ROOT, "data", "stage_anchor")
    times["index build"] = A.build_index(refs, d)
    t = time.time()
    ora = A.AnchorOracle(os.path.join(d, "index"))
    reads = A.synthetic_reads(SEED + 1, refs, info) + A.targeted_synthetic(SEED + 2, ora, refs)
    syn = A.AnchorSet(os.path.join(d, "index"), reads)
    fa = os.path.join(demo["dir"], "viral-gs.fa")
    dem = A.AnchorSet(demo["index"], A.demo_reads(demo["fastq"], 1300) + A.demo_error_reads(SEED + 3, fa, 900))
    times["reads and oracle"] = time.time() - t
    print("anchor stage: %d + %d reads; %s" % (len(syn.reads), len(dem.reads), ", ".join("%s %.1f s" % kv for kv in times.items())))
    return {"synthetic": syn, "demo": dem}


def class_counts(sets, pick=None):
    cnt = collections.Counter()
    for name, s in sets.items():
        for i in (range(len(s.reads)) if pick is None else pick[name]):
            cnt.update(s.fcls[i] | s.scls[i])
    return cnt


def test_the_oracle_reaches_the_classes(sets):
    cnt = class_counts(sets)
    print({c: cnt[c] for c in A.CLASSES + A.SLOW_CLASSES})
    for c in A.CLASSES + A.SLOW_CLASSES:
        if c in A.UNREACHABLE:
            assert cnt[c] == 0, (c, "reached after all: take it off the list", cnt[c])
        else:
            assert cnt[c] >= 50, (c, cnt[c])
    syn = sets["synthetic"]
    kinds = collections.Counter(k for k, _ in syn.reads)
    assert kinds["tops64"] >= 2 and kinds["tops65"] >= 2 and kinds["tops129"] >= 2 and kinds["long"] >= 6
    assert max(len(s) for _, s in syn.reads) >= 14000
    # what the forms add to the reads: a lane scratch that is already full, caps too small for the commit, budgets that run out
    cs = A.build_cases(syn, range(len(syn.reads)))
    assert len(cs["small_cap"].rows) >= 50 and len(cs["budget_island"].rows) >= 50 and len(cs["budget_slow"].rows) >= 50 and len(cs["budget_fast"].rows) >= 50
    assert sum(1 for r in cs["lane"].rows if r["meta"]) >= 50 and sum(1 for r in cs["lane"].rows if not r["meta"]) >= 50        # fast_classify_lane gives up / does not
    # fast_classify's own "the lane's scratch is already full" (start >= DSB_LANE_ANC_CAP): predictable for one lane only, see lane_full_one_lane
    full = sum(c in s.fcls[i] for s in sets.values() for i in range(len(s.reads)) for c in A.CASES_1LANE)
    print("reads in which an island finds its lane's scratch exactly full on the 1-lane leg:", full)
    assert full >= 1


def run_leg(which, sets, pick=None, variants=VARIANTS, gens=(0, MID_GEN), whole_only_above=None, islands_per_strand=6):
    """every form over the reads picked, on every index form asked for; the first index form with every starting generation, the others with the first.
    whole_only_above: reads longer than this run the whole-read form alone (the 64-lane emulation: a long read is there for the commit's chunks)"""
    ran = collections.Counter()
    for name, s in sets.items():
        idx = list(range(len(s.reads))) if pick is None else pick[name]
        for v, (raw, rank64) in enumerate(variants):
            leg = A.AnchorLeg(which, s.index_dir, raw=raw, rank64=rank64)
            assert leg.compressed == (not raw) and leg.superblocks == rank64, (leg.compressed, leg.superblocks)
            try:
                leg.findings()
                for g in (gens if v == 0 else gens[:1]):
                    cases = A.build_cases(s, idx, sp_gen=g, whole_only_above=whole_only_above, lane_steps=leg.lane_steps, islands_per_strand=islands_per_strand)
                    ran.update(A.check_cases(leg, cases))
                f = leg.findings()
                assert not f, f
            finally:
                leg.close()
    return dict(ran)


def test_one_lane_emulation(sets):
    t = time.time()
    ran = run_leg("emu1", sets)
    print("1-lane emulation: %.1f s, %r" % (time.time() - t, ran))


def subset64(sets, per_class=5):
    """per class the shortest reads that are in it"""
    pick = {}
    for name, s in sets.items():
        idx = set()
        for c in A.CLASSES + A.SLOW_CLASSES:
            have = sorted((i for i in range(len(s.reads)) if c in (s.fcls[i] | s.scls[i])), key=lambda i: (len(s.reads[i][1]), i))
            idx.update(have[:per_class])
        pick[name] = sorted(idx)
    return pick


# the index as the product opens it with generation 0 in both lane orders; the raw 13-mer table with rank superblocks and the generation in mid-range in one
@pytest.mark.parametrize("order,variant,gen", [("fwd", 0, 0), ("rev", 0, 0), ("fwd", 3, MID_GEN)], ids=["fwd", "rev", "fwd-raw-rank64-midgen"])
def test_64_lane_emulation(sets, order, variant, gen, monkeypatch):
    if order == "rev":
        monkeypatch.setenv("DSB_EMU_ORDER", "rev")
    pick = subset64(sets)
    cnt = class_counts(sets, pick)
    for c in A.CLASSES + A.SLOW_CLASSES:
        assert c in A.UNREACHABLE or cnt[c] >= 5, (c, cnt[c])
    t = time.time()
    ran = run_leg("emu64", sets, pick, variants=VARIANTS[variant:variant + 1], gens=(gen,), whole_only_above=3000, islands_per_strand=2)     # (forms (a) and (b) are wave-uniform: two islands per strand here)
    # what the forms add to the reads, in the subset too
    assert ran["small_cap"] >= 5 and ran["budget_island"] >= 5 and ran["budget_slow"] >= 5 and ran["budget_fast"] >= 5, ran
    for name, s in sets.items():
        rows = A.build_cases(s, pick[name])["lane"].rows
        assert name != "synthetic" or (sum(1 for r in rows if r["meta"]) >= 5 and sum(1 for r in rows if not r["meta"]) >= 5)
    print("64-lane emulation (%s, index form %d, generation %#x): %d reads, %.1f s, %r" % (order, variant, gen, sum(len(v) for v in pick.values()), time.time() - t, ran))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1, 2, 3], ids=["compressed-rank32", "raw-rank32", "compressed-rank64", "raw-rank64"])
@pytest.mark.parametrize("which", ["synthetic", "demo"])
def test_device(sets, which, variant):
    """one index in one of its forms per test (what the walks read of it is uploaded: the raw 13-mer table is 512 MiB), every form of the stage over the full
    set; the form the product opens by default runs with both starting generations, the others with generation 0"""
    t = time.time()
    ran = run_leg("device", {which: sets[which]}, variants=VARIANTS[variant:variant + 1], gens=(0, MID_GEN) if variant == 0 else (0,))
    print("device, %s index, form %d: %.1f s, %r" % (which, variant, time.time() - t, ran))
