"""a-12, the sparse DP's predecessor scan (src/cly.c:2495-2517, 2612-2638, 2759-2783) on its own: every restatement of the reference's
newest-first scan the device code has (dsb_classify_dev.h), each called directly on bare node lists (tests/stage/dsb_stage_forms.h) and
compared, node by node and exactly, with the oracle's loops (oracle/classify.c: ora_sdp_dp_stage calls the functions ora_classify runs):
  (a) pred    sdp_best_pred<0|1|2> node by node; modes 1 and 2 keep the LDS ring of the newest 16 nodes, mode 0 runs without it
  (b) batch   sdp_best_pred_b<1|2> on one wavefront (sdp_batch_old<MODE, true>), through node_get / NodeBlock, batches of 8
  (c) block   sdp_block_scores<1|2> with its deep pass sdp_batch_old<MODE, false>; blocks of the extension's own min(64, rest) and forced
              sequences of 1, 2, 7, 8, 9, 63 and 64 nodes, the scores written back between the blocks
  (d) mw      sdp_batch_old_mw<1|2> on 2, 4 and 8 wavefronts with batches of 1 .. 8 nodes, on the device only (the emulation has one
              wavefront), called whatever DSB_MW_MIN_PREDS says; the in-batch part and the combination are sdp_best_pred_b's own
Three legs: the 1-lane emulation (one node per block there: a lane is a node), the 64-lane emulation with its race detector, the GPU.

Lists: 1 .. 2100 nodes at every boundary of the ring (16), the batch (8), the chunk (64, 4 x 64) and the first deep pass, three
tandem-repeat lists of about 5000 nodes with hundreds of nodes at one t_pos, short lists whose coordinates wrap (q = -1 .. -8, a seed
of len 1 - 9 or -9 at q = 0), and lists harvested from the oracle's own extensions (ora_ext_stage: whole lists and lists given up at a merge).  Left lists are right lists
turned round.  What a list exercises is worked out from a numpy restatement of the scan (checked against the oracle's scores on every
node), never from the device: a list is in a class if one of its nodes is.  Every class has >= 50 lists in the full set and >= 5 in the
64-lane subset.

Heavy hand-over: with heavy_limit below a list's predecessor count forms (b) and (c) return early with DSB_ST_HEAVY, nodes and guards
untouched (form (a) does not look at the limit: its callers do)."""
import random
import time

import numpy as np
import pytest

import stage_lib as S
import stage_ext_lib as E

SEED = 2612
ST_HEAVY = 32


@pytest.fixture(scope="module")
def dpset(built):
    ora = S.Oracle()
    t = time.time()
    ext = E.build_ext_set(SEED + 7, ora)
    s = E.build_dp_set(SEED, ext)
    ora.close()
    print("sparse DP: %d lists, %d nodes generated and classified in %.1f s" % (len(s.lists), sum(len(x) for x in s.lists), time.time() - t))
    return s


def counts(s):
    return {c: sum(c in cl for cl in s.classes) for c in E.CLASSES}


def test_coverage_of_the_full_set(dpset):
    cnt = counts(dpset)
    print(cnt)
    for c in E.CLASSES:
        assert cnt[c] >= 50, (c, cnt[c])
    sizes = {m: {len(N) for N, mm in zip(dpset.lists, dpset.modes) if mm == m} for m in (0, 1, 2)}
    for m in (0, 1, 2):
        assert set(E.SIZES) <= sizes[m], (m, sorted(set(E.SIZES) - sizes[m]))
    tandem = [i for i, cl in enumerate(dpset.classes) if E.TANDEM in cl and len(dpset.lists[i]) >= 4900]
    assert len(tandem) >= 3 and {dpset.modes[i] for i in tandem} == {1, 2}
    assert sum(src == "harvested" for src in dpset.src) >= 20
    for i, sc in dpset.harvest_scores.items():                # the oracle's extension gave these nodes the scores the bare DP entry gives them
        assert np.array_equal(dpset.expect[i][1:len(sc)], sc[1:]), i
    assert max(len(N) for N in dpset.lists) <= 5100


def forced_sizes(s, idx, pool, seed):
    rng = random.Random(seed)
    return [[rng.choice(pool) for _ in range(rng.randint(3, 14))] for _ in idx]


def check(leg, s, form, idx=None, sizes=None, waves=0):
    idx = list(range(len(s.lists))) if idx is None else list(idx)
    cs, nodes = leg.run(s, form, idx, sizes, waves)
    ran = 0
    for k, i in enumerate(idx):
        c = cs[k]
        assert bool(c["defined"]) == (s.modes[i] != 0 or form == "pred"), (form, i)
        if not c["defined"]:
            continue
        ran += 1
        n, o = len(s.lists[i]), int(c["node_off"])
        assert int(c["status"]) == 0 and int(c["scored"]) == n, (form, waves, i, s.src[i], int(c["status"]), int(c["scored"]), n)
        assert np.array_equal(nodes[o:o + n, :3], s.lists[i][:, :3]) and (nodes[o + n:o + n + leg.GUARD] == E.PATTERN).all(), (form, waves, i, s.src[i])
        got = nodes[o:o + n, 3].astype(np.int32)
        bad = np.nonzero(got != s.expect[i])[0]
        assert len(bad) == 0, "%s (waves %d, sizes %r): list %d (%s, mode %d, %d nodes): %d scores differ from the oracle's, first at node %d: %d for %d" % (
            form, waves, None if sizes is None else sizes[k], i, s.src[i], s.modes[i], n, len(bad), bad[0], got[bad[0]], s.expect[i][bad[0]])
    return ran


def check_heavy(leg, s, idx):
    """heavy_limit below the predecessor count: a block or batch charges at least one wavefront's width of predecessors per node
    (sdp_block_scores: m * DSB_WAVE; sdp_batch_old: DSB_WAVE per group and node), so >= 300 nodes are beyond 16 widths"""
    limit = 16 * leg.lanes
    idx = [i for i in idx if s.modes[i] != 0 and len(s.lists[i]) >= 300]
    for form in ("batch", "block"):
        cs, nodes = leg.run(s, form, idx, heavy=[limit] * len(idx))
        for k, i in enumerate(idx):
            c = cs[k]; n, o = len(s.lists[i]), int(c["node_off"])
            assert int(c["status"]) & ST_HEAVY and int(c["scored"]) < n and int(c["dp_preds"]) > limit, (form, i, c.tolist())
            assert np.array_equal(nodes[o:o + n, :3], s.lists[i][:, :3]) and (nodes[o + n:o + n + leg.GUARD] == E.PATTERN).all(), (form, i)
            assert (nodes[o + int(c["scored"]):o + n, 3] == E.PATTERN).all(), (form, i)
    return len(idx)


def check_all(leg, s, idx=None):
    idx = list(range(len(s.lists))) if idx is None else list(idx)
    ran = {"pred": check(leg, s, "pred", idx), "batch": check(leg, s, "batch", idx), "block": check(leg, s, "block", idx)}
    ran["block forced"] = check(leg, s, "block", idx, forced_sizes(s, idx, [1, 2, 7, 8, 9, 63, 64], SEED + 1))
    ran["heavy"] = check_heavy(leg, s, idx)
    return ran


# ---- leg 1: the 1-lane emulation, the full set ---------------------------------------------------------------------------------------
def test_one_lane_emulation(dpset):
    leg = E.emu1()
    assert leg.ST_HEAVY == ST_HEAVY and leg.DPB == 8 and leg.RING == 16
    t = time.time()
    ran = check_all(leg, dpset)
    print("1-lane emulation: %.1f s, lists per form %r" % (time.time() - t, ran))
    assert ran["pred"] == len(dpset.lists) and ran["batch"] == ran["block"] == sum(m != 0 for m in dpset.modes) and ran["heavy"] >= 50


# ---- leg 2: 64 lanes with the race detector: the shortest lists of every class -------------------------------------------------------
def subset64(s, per_class=5):
    idx = set()
    for c in E.CLASSES:
        idx.update(sorted((i for i, cl in enumerate(s.classes) if c in cl), key=lambda i: (len(s.lists[i]), i))[:per_class])
    for m in (0, 1, 2):                                      # and the lists around the ring, the batch and the first chunk in every mode
        idx.update(i for i, N in enumerate(s.lists) if s.modes[i] == m and len(N) in (1, 2, 8, 9, 16, 17, 64, 65, 66) and s.src[i].split()[0] in ("walk", "gap"))
    return sorted(idx)


@pytest.mark.parametrize("order", ["fwd", "rev"])
def test_64_lane_emulation(dpset, order, monkeypatch):
    if order == "rev":
        monkeypatch.setenv("DSB_EMU_ORDER", "rev")
    leg = E.emu64()
    assert leg.lanes == 64
    idx = subset64(dpset)
    sub = dpset.subset(idx)
    cnt = counts(sub)
    for c in E.CLASSES:
        assert cnt[c] >= 5, (c, cnt[c])
    t = time.time()
    leg.findings()
    ran = check_all(leg, sub)
    f = leg.findings()
    assert not f, f
    print("64-lane emulation (%s): %d lists, %d nodes, %.1f s, %r" % (order, len(idx), sum(len(x) for x in sub.lists), time.time() - t, ran))


# ---- leg 3: the device -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device(dpset):
    leg = E.device()
    assert leg.lanes == 64 and leg.ST_HEAVY == ST_HEAVY
    t = time.time()
    ran = check_all(leg, dpset)
    print("device, forms (a) .. (c): %.1f s, lists per form %r" % (time.time() - t, ran))


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [2, 4, 8])
def test_device_several_wavefronts(dpset, waves):
    """(d): every extension list, batches of 8 and forced batches of 1 .. 8 nodes.  With W waves a round covers W x 256 predecessors: the
    lists of 257 .. 5000 nodes put the cut of a node into every wave's chunk, into a later round, and nowhere."""
    leg = E.device()
    idx = [i for i, m in enumerate(dpset.modes) if m != 0]
    t = time.time()
    a = check(leg, dpset, "mw", idx, None, waves)
    b = check(leg, dpset, "mw", idx, forced_sizes(dpset, idx, [1, 2, 3, 4, 5, 6, 7, 8], SEED + waves), waves)
    assert a == b == len(idx)
    print("device, sdp_batch_old_mw on %d wavefronts: %.1f s, %d lists twice" % (waves, time.time() - t, len(idx)))
