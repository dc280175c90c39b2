"""a-12, the sparse approximate match and the gap scoring (src/cly.c:2335-2530) on their own: every form of `sdp_match` the device
code has (dsb_classify_dev.h: wtab_build + sdp_match_t, wtab_build_pk + sdp_match_t, sdp_match_inv, the dispatcher sdp_match_n,
sdp_match_lds on a staged read and window), gap_lane and sdp_middle_M2, each called directly (tests/stage/dsb_stage_forms.h) and
compared with the oracle's restatement of the reference's one loop (oracle/classify.c: ora_sdp_match_stage, ora_gap_stage).  Three
legs take the same cases: the 1-lane host emulation, the 64-lane emulation with its race detector (no finding allowed, also with the
lanes in reverse order), and the GPU through tests/stage/libdsbstage.so -- the only place where the wavefront primitives of
dsb_wave.h (DPP scans, ds_bpermute, LDS compare-and-swap, 16-byte LDS accesses, typed global loads) are compared with anything
but a whole read.

Domain, from the call sites:
  right extension (sdp_right_M2)  forward form; t_len = min(600, ...) >= 12, 50 more bases loaded behind it; window
                                  [max(q_ed - 2000, q_st - 8), q_ed] with q_ed <= L, so q_bg wraps in uint32 when q_st < 8
  left extension (sdp_left_M2)    backward form; t_str = ref + 50 (the 50 bases in front are loaded), t_len = min(600, ...) >= 12, window
                                  [q_bg, min(q_bg + 2000, q_st - 1)], q_bg >= 0.  At the start of a text only t_len bases are loaded at ref:
                                  the end of the window is unloaded (value 4, oracle U2); the buffer is filled once per extension and loaded
                                  piecewise, so the first unloaded byte may lie anywhere from t_len - 50 on
  middle (sdp_middle_M2)          forward form; 13 <= t_len < 2000, the window is the gap: [pq + pl - 8, cq - 1], nothing loaded behind t_len
  reads of 200 .. 8000 bases with non-ACGT bytes; windows <= 2001 positions wide (n_q <= DSB_WTAB_MAXQ is checked by every form)
Window content: the read's own bases with substitutions and indels at 0 .. 25 %, homopolymers and tandem repeats of period 2 .. 9,
the same 14 bases planted at many places, windows at the pads, windows with nothing in common.

Expected: the oracle's node list, in order, through every form that is defined for a case, and no status bit; sdp_match_inv gives up
exactly when the pairs (counted here from the inputs) exceed DSB_INV_PAIRS; the LDS mirror holds the first 64 nodes unless bit 31
says otherwise, which it may only when a probed position has more than DSB_SDP_KEEP nodes; a node arena smaller than the list gives
DSB_ST_SMS_OVF, untouched guard words and the oracle's nodes in front of the overflow; gap_lane declines exactly the gaps a
predicate written here declines and scores the others as the oracle does; sdp_middle_M2 gives the oracle's score with and without
packed words.  Nodes per probed position are derived from the oracle's list: a forward node of probed position i starts at
i - back_len (back_len < 4 unless i == 4), a backward node ends fwd (< 4 unless i == 4) bases behind the 9-mer of i.

The coverage conditions (>= 50 cases per class in the full set, >= 5 in the 64-lane subset) are asserted from the oracle's output and
the inputs alone.

Found by this test: sdp_middle_M2 staged the read only up to q_ed + 80, but an exact match that starts at q_pos == q_ed is bounded by
the window alone (the reference's unsigned `q_ed - q_pos - 1` wraps) and read up to q_ed + t_len + 3 -- in a tandem repeat that runs
from a gap into the anchor behind it the staged form compared window bytes for read bytes."""
import time

import numpy as np
import pytest

import stage_lib as S

N_READS, PER_READ, N_CHAINS = 160, 126, 260          # ~20 000 sdp_match cases, ~5 000 gaps
SEED = 12


@pytest.fixture(scope="module")
def ora(built):
    o = S.Oracle()
    yield o
    o.close()


@pytest.fixture(scope="module")
def sets(ora):
    k = S.emu1().k
    t = time.time()
    sd = S.build_sdp_set(k, ora, SEED, N_READS, PER_READ)
    gp = S.build_gap_set(k, ora, SEED + 1, N_CHAINS)
    print("stage a-12: %d sdp_match cases, %d gaps, %d chains generated in %.1f s" % (len(sd.cases), len(gp.gaps), len(gp.chain_cases), time.time() - t))
    return sd, gp


# ---- coverage ------------------------------------------------------------------------------------------------------------------
def sdp_classes(s):
    """class name -> indices of the cases in it; direction-wise where the direction applies"""
    k = s.k
    cls = {}

    def put(name, i, c):
        cls.setdefault(name + (":fwd" if c["fwd"] else ":bwd"), []).append(i)
    for i, (c, m, e) in enumerate(zip(s.cases, s.meta, s.expect)):
        runs = m["n_q"] > 0 and 4 < m["tk"] <= 0x7FFFFFFF
        if len(e) == 0 and runs:
            put("no node", i, c)
        if m["maxnodes"] >= 4:
            put("position with >= 4 nodes", i, c)
        if m["maxocc"] > k.SDP_CAND:
            put("9-mer at > 64 positions", i, c)
        if m["pairs"] > k.INV_PAIRS:
            put("pairs > 256", i, c)
        if 0 < m["n_q"] < k.INV_MINQ and m["tk"] > 4:
            put("n_q < 96", i, c)
        if m["tk"] <= 4:
            put("t_kmer_num <= 4", i, c)
        if c["q_ed"] > c["L"] - 9:
            put("q_ed > L - 9", i, c)
        if m["tk"] > 4 * k.INV_MAXPOS:
            cls.setdefault("t_kmer_num > 1200", []).append(i)          # (middle gaps only: forward)
        if m["padbits"] and m["n_q"] > 0:
            cls.setdefault("9-mer with pad bits", []).append(i)         # (left extension only: backward)
        if c["q_bg"] >= 1 << 31:
            cls.setdefault("wrapped q_bg", []).append(i)                # (right extension only: forward)
        if c["kind"] == S.MIDDLE and m["n_q"] > 0:
            cls.setdefault("staged" if m["stage"][1] else "not staged", []).append(i)
        if m["ovf"]:
            cls.setdefault("node arena overflow", []).append(i)
    return cls


SDP_CLASSES = [n + d for n in ("no node", "position with >= 4 nodes", "9-mer at > 64 positions", "pairs > 256", "n_q < 96", "t_kmer_num <= 4", "q_ed > L - 9") for d in (":fwd", ":bwd")] + \
              ["t_kmer_num > 1200", "9-mer with pad bits", "wrapped q_bg", "staged", "not staged", "node arena overflow"]


def gap_classes(g):
    cls = {}
    for i, m in enumerate(g.gap_meta):
        for w in m["why"]:
            cls.setdefault("none:" + w, []).append(i)
        if not m["why"]:
            cls.setdefault("scored:" + ("0" if m["nodes"] == 0 else "12" if m["nodes"] == g.k.GL_NODES else "1-11"), []).append(i)
    return cls


GAP_CLASSES = ["none:maxt", "none:read_end", "none:text_end", "none:words", "none:nodes", "scored:0", "scored:1-11", "scored:12"]


def test_coverage_of_the_full_set(sets):
    sd, gp = sets
    cls = sdp_classes(sd)
    print({n: len(cls.get(n, [])) for n in SDP_CLASSES})
    for n in SDP_CLASSES:
        assert len(cls.get(n, [])) >= 50, (n, len(cls.get(n, [])))
    gc = gap_classes(gp)
    print({n: len(gc.get(n, [])) for n in GAP_CLASSES})
    for n in GAP_CLASSES:
        assert len(gc.get(n, [])) >= 50, (n, len(gc.get(n, [])))
    na = gp.chain_cases["n_anc"]
    assert na.min() == 1 and na.max() == 400
    assert 15000 <= len(sd.cases) and 4000 <= len(gp.gaps)
    L = sd.cases["L"]
    assert L.min() >= 200 and L.max() <= 8000 and sd.cases["t_len"].max() < 2000
    assert all(m["n_q"] <= 2001 for m in sd.meta)


# ---- the checks, for any leg ---------------------------------------------------------------------------------------------------
def check_sdp(leg, s):
    k = s.k
    ovf = np.array([m["ovf"] for m in s.meta])
    n_exp = np.array([len(e) for e in s.expect])
    pairs = np.array([m["pairs"] for m in s.meta])
    many = np.array([m["maxnodes"] > k.SDP_KEEP for m in s.meta])
    ran = {}
    for form in S.FORMS:
        cs, nodes, mirror = leg.sdp(form, s)
        d = cs["defined"] != 0
        ran[form] = int(d.sum())
        rv = cs["rv"].astype(np.int64)
        gave_up = np.zeros(len(cs), bool)
        if form == "inv":
            # defined: there is something to look up, the window is wide and the probed positions are few (sdp_match_p's test)
            n_q = np.array([m["n_q"] for m in s.meta]); tk = np.array([m["tk"] for m in s.meta])
            assert np.array_equal(d, (n_q >= k.INV_MINQ) & (tk > 4) & (tk <= 4 * k.INV_MAXPOS) & (n_q <= k.WTAB_MAXQ))
            gave_up = d & (rv == S.INV_NONE)
            assert np.array_equal(gave_up, d & (pairs > k.INV_PAIRS)), "sdp_match_inv gives up iff pairs > DSB_INV_PAIRS"
        elif form in ("lds", "lds_pk"):
            assert np.array_equal(d, np.array([m["stage"][form == "lds_pk"] for m in s.meta]))
        elif form in ("n", "n_pk"):
            assert d.all()
        ok = d & ~ovf & ~gave_up
        # status and count
        assert not cs["status"][ok].any(), (form, np.nonzero(cs["status"] * ok)[0][:5])
        assert np.array_equal(rv[ok] & 0x7FFFFFFF, n_exp[ok]), (form, np.nonzero(ok & ((rv & 0x7FFFFFFF) != n_exp))[0][:5])
        # every node region at once: the oracle's nodes (the score word is not sdp_match's), the pattern everywhere else
        exp = np.where(ok[s.case_of][:, None], s.full, S.PATTERN)
        cmp_rows = ~ovf[s.case_of]
        bad = np.unique(s.case_of[cmp_rows & (nodes != exp).any(axis=1)])
        assert len(bad) == 0, "%s: node lists differ from the oracle's in %d cases, first %r" % (form, len(bad), [(int(b), s.cases[b].tolist()) for b in bad[:3]])
        # a node arena smaller than the list
        for i in np.nonzero(ovf & d & ~gave_up)[0]:
            c = cs[i]; o = int(c["node_off"]); cap = int(c["sms_cap"]); n = int(c["rv"]) & 0x7FFFFFFF
            assert int(c["status"]) == S.ST_SMS_OVF, (form, i, int(c["status"]))
            assert n <= cap and np.array_equal(nodes[o:o + n, :3], s.expect[i][:n]), (form, i)
            assert (nodes[o + cap:o + cap + S.GUARD] == S.PATTERN).all(), (form, i)
        if form in ("lds", "lds_pk"):
            bit = (rv >> 31) != 0
            assert not (bit & ~many)[ok].any(), "bit 31 only if a probed position has more than DSB_SDP_KEEP nodes"
            for i in np.nonzero(ok & ~bit)[0]:
                n = min(64, int(n_exp[i]))
                assert np.array_equal(mirror[i, :n, :3], s.expect[i][:n]), (form, i)
    return ran


def check_gaps(leg, g, chains=True):
    cs, G = leg.gap_lane(g)
    assert not cs["status"].any()
    none_exp = np.array([bool(m["why"]) for m in g.gap_meta])
    gain_exp = np.array([m["gain"] for m in g.gap_meta])
    got = G["gain"].astype(np.int64)
    assert np.array_equal(got == S.GL_NONE, none_exp), "gap_lane declines iff the predicate says so: %r" % (np.nonzero((got == S.GL_NONE) != none_exp)[0][:5],)
    assert np.array_equal(got[~none_exp], gain_exp[~none_exp]), np.nonzero(~none_exp & (got != gain_exp))[0][:5]
    if chains:
        for use_pk in (True, False):
            cs = leg.middle(g, use_pk)
            assert not cs["status"].any(), (use_pk, np.nonzero(cs["status"])[0][:5])
            assert np.array_equal(cs["score"], np.array(g.chain_score, np.int32)), (use_pk, np.nonzero(cs["score"] != np.array(g.chain_score))[0][:5])


# ---- leg 1: the 1-lane emulation, the full set --------------------------------------------------------------------------------
def test_one_lane_emulation_sdp_match(sets):
    sd, _ = sets
    t = time.time()
    ran = check_sdp(S.emu1(), sd)
    print("1-lane emulation, sdp_match forms: %.1f s, cases per form %r" % (time.time() - t, ran))
    assert all(v >= 1000 for v in ran.values()), ran


def test_one_lane_emulation_gaps(sets):
    _, gp = sets
    t = time.time()
    check_gaps(S.emu1(), gp)
    print("1-lane emulation, gap_lane and sdp_middle_M2: %.1f s" % (time.time() - t))


# ---- leg 2: 64 lanes with the race detector, a fixed subset ----------------------------------------------------------------------
def subset64(s, per_class=6):
    cls = sdp_classes(s)
    idx = set()
    for n in SDP_CLASSES:
        # (the cheapest cases of a class: the emulation runs every lane's loads and stores through the detector)
        c = sorted(cls.get(n, []), key=lambda i: (s.meta[i]["pairs"] + len(s.expect[i]) + s.meta[i]["n_q"], i))
        idx.update(c[:per_class])
    return s.subset(sorted(idx))


def gap_subset64(k, ora):
    return S.build_gap_set(k, ora, SEED + 2, 80)


@pytest.mark.parametrize("order", ["fwd", "rev"])
def test_64_lane_emulation(sets, ora, order, monkeypatch):
    sd, _ = sets
    if order == "rev":
        monkeypatch.setenv("DSB_EMU_ORDER", "rev")
    leg = S.emu64()
    assert leg.k.lanes == 64
    sub = subset64(sd)
    cls = sdp_classes(sub)
    for n in SDP_CLASSES:
        assert len(cls.get(n, [])) >= 5, (n, len(cls.get(n, [])))
    t = time.time()
    leg.findings()
    check_sdp(leg, sub)
    f = leg.findings()
    assert not f, f
    gp = gap_subset64(leg.k, ora)
    gc = gap_classes(gp)
    for n in GAP_CLASSES:
        assert len(gc.get(n, [])) >= 5, (n, len(gc.get(n, [])))
    check_gaps(leg, gp)
    f = leg.findings()
    assert not f, f
    print("64-lane emulation (%s): %d sdp_match cases, %d gaps, %.1f s" % (order, len(sub.cases), len(gp.gaps), time.time() - t))


# ---- leg 3: the device -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_sdp_match(sets):
    sd, _ = sets
    t = time.time()
    ran = check_sdp(S.device(), sd)
    print("device, sdp_match forms: %.1f s, cases per form %r" % (time.time() - t, ran))


@pytest.mark.gpu
def test_device_gaps(sets):
    _, gp = sets
    t = time.time()
    check_gaps(S.device(), gp)
    print("device, gap_lane and sdp_middle_M2: %.1f s" % (time.time() - t))
