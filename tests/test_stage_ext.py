"""a-12, the right and left extensions (src/cly.c:2532-2819) on their own: one sdp_right_M2 or sdp_left_M2 per case, block-wise (through
ext_block and sdp_block_scores) and node by node (sdp_right_M2_mw / sdp_left_M2_mw with w.mw == nullptr), called directly
(tests/stage/dsb_stage_forms.h: stage_ext) and compared with the oracle's ora_ext_stage, which runs the functions ora_classify runs.
A case is a read, a strand, a synthetic 2-bit text of two references (the chains lie on the first, seq_offset 0, or on the second), a
chain list with its anchors, the chain to extend and its score; w.hit and w.sc are set up with the product's sc_hash_idx.  Compared,
exactly: the returned score, every chain afterwards (all fields), w.status == 0, the number of nodes of the final list, their
coordinates and the scores of the nodes the reference's loop scored (the block-wise form scores whole blocks: what lies behind the
reference's stop is not compared; node 0's len of a left list is never read and not compared), and the guards behind the node region.

The classes come from the oracle's reason code, its merge count and its node lists, never from the device; each has >= 50 cases in the
full set and >= 5 in the 64-lane subset.  Two quirks of the reference shape the cases: a right extension searches the read from
max(min(q_ed + 1000, L) - 2000, q_st - 8) on, compared as unsigned numbers, so it finds nothing when q_st < 8 or when the read has
fewer than 2000 bases up to there; and a reference end (next_step < 12) is reached only from the last_search window, whose width
is not cut to the bases left, or by a chain that ends at the end itself.

Heavy hand-over: with heavy_limit 1 the block-wise and the node-by-node form return with DSB_ST_HEAVY on every case whose first window
has ten nodes or more, guards intact; scores are not compared."""
import time

import numpy as np
import pytest

import stage_lib as S
import stage_ext_lib as E

SEED = 2619
ST_HEAVY = 32


@pytest.fixture(scope="module")
def extset(built):
    ora = S.Oracle()
    t = time.time()
    s = E.build_ext_set(SEED, ora)
    ora.close()
    s.cls = [s.classes(i) for i in range(len(s.rows))]
    print("extensions: %d cases generated in %.1f s" % (len(s.rows), time.time() - t))
    return s


def counts(s, idx=None):
    idx = range(len(s.rows)) if idx is None else idx
    return {c: sum(c in s.cls[i] for i in idx) for c in E.EXT_CLASSES}


def test_coverage_of_the_full_set(extset):
    cnt = counts(extset)
    print(cnt)
    for c in E.EXT_CLASSES:
        assert cnt[c] >= 50, (c, cnt[c])
    assert max(len(q) for q in extset.pool.seqs) <= 20000
    on = [int(extset.chain_arr[m["c0"]]["ref_ID"]) for m in extset.rows]
    assert min(on.count(0), on.count(1)) >= 200               # seq_offset 0 and seq_offset > 0


def check(leg, s, mw, idx=None):
    idx = list(range(len(s.rows))) if idx is None else list(idx)
    cs, ch, nodes = leg.run(s, mw, idx)
    o = 0
    for k, i in enumerate(idx):
        e, c, m = s.exp[i], cs[k], s.rows[i]
        got = ch[o:o + m["n_chains"]]; o += m["n_chains"]
        what = (("node by node" if mw else "block-wise"), i, m["kind"], "left" if m["left"] else "right", "reason %d, %d merges" % (e["reason"], e["merges"]))
        assert int(c["defined"]) == 1 and int(c["status"]) == 0, what + (int(c["status"]),)
        assert int(c["score"]) == e["score"], what + (int(c["score"]), e["score"])
        assert got.tobytes() == e["chains"].tobytes(), what + (got.tolist(), e["chains"].tolist())
        last, scored = e["segs"][-1]
        b, cap = int(c["node_off"]), int(c["sms_cap"])
        assert int(c["n_sms"]) == len(last), what + (int(c["n_sms"]), len(last))
        cols = nodes[b:b + len(last), :3].copy(); exp = last[:, :3].copy()
        if m["left"]:
            cols[0, 2] = exp[0, 2] = 0
        assert np.array_equal(cols, exp) and np.array_equal(nodes[b:b + scored, 3], last[:scored, 3]), what
        assert (nodes[b + cap:b + cap + E.EXT_GUARD] == E.PATTERN).all(), what
    return len(idx)


def check_heavy(leg, s, idx):
    # (sdp_block_scores charges m * DSB_WAVE for a block of m nodes, sdp_batch_old DSB_WAVE per node and group: ten nodes are beyond a limit of 1 on any leg)
    idx = [i for i in idx if len(s.exp[i]["win"]) and int(s.exp[i]["win"][0]) > 10]
    for mw in (0, 1):
        cs, ch, nodes = leg.run(s, mw, idx, heavy=1)
        for k, i in enumerate(idx):
            c = cs[k]; b, cap = int(c["node_off"]), int(c["sms_cap"])
            assert int(c["status"]) & ST_HEAVY, (mw, i, int(c["status"]))
            assert (nodes[b + cap:b + cap + E.EXT_GUARD] == E.PATTERN).all(), (mw, i)
    return len(idx)


def check_all(leg, s, idx=None):
    idx = list(range(len(s.rows))) if idx is None else list(idx)
    return {"block-wise": check(leg, s, 0, idx), "node by node": check(leg, s, 1, idx), "heavy": check_heavy(leg, s, idx)}


def test_one_lane_emulation(extset):
    t = time.time()
    ran = check_all(E.ext_emu1(), extset)
    print("1-lane emulation: %.1f s, %r" % (time.time() - t, ran))
    assert ran["heavy"] >= 50


def subset64(s, per_class=5):
    cost = lambda i: (sum(len(N) for N, _ in s.exp[i]["segs"]), i)
    idx = set()
    for c in E.EXT_CLASSES:
        idx.update(sorted((i for i in range(len(s.rows)) if c in s.cls[i]), key=cost)[:per_class])
    return sorted(idx)


@pytest.mark.parametrize("order", ["fwd", "rev"])
def test_64_lane_emulation(extset, order, monkeypatch):
    if order == "rev":
        monkeypatch.setenv("DSB_EMU_ORDER", "rev")
    leg = E.ext_emu64()
    idx = subset64(extset)
    cnt = counts(extset, idx)
    for c in E.EXT_CLASSES:
        assert cnt[c] >= 5, (c, cnt[c])
    t = time.time()
    leg.findings()
    ran = check_all(leg, extset, idx)
    f = leg.findings()
    assert not f, f
    print("64-lane emulation (%s): %d cases, %.1f s, %r" % (order, len(idx), time.time() - t, ran))


@pytest.mark.gpu
def test_device(extset):
    t = time.time()
    ran = check_all(E.ext_device(), extset)
    print("device: %.1f s, %r" % (time.time() - t, ran))
