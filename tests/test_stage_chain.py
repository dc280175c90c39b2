"""a-10, resolve_tree (src/cly.c:72-112,201-349) on its own: every form the device code has for its three steps (dsb_classify_dev.h) --
the sort of chain_sort_M3 (rank with distinct keys, rank with the tie rule, bottom-up merge), the DP (chain_insert_M2, chain_dp_M3_wave with
its arrays in LDS or in the idle half of the anchor arena, the serial chain_dp_M3) and chain_top_select (rank from LDS keys, or
glibc_sort_chains<0> and a cut) -- forced whatever the number of anchors is (tests/stage/dsb_stage_forms.h: stage_resolve), and resolve_tree
itself, compared with the oracle's restatement of the reference's loops (oracle/classify.c: ora_resolve_stage).  Three legs take the same
cases: the 1-lane host emulation, the 64-lane emulation with its race detector (no finding allowed, also with the lanes in reverse
order), and the GPU through tests/stage/libdsbstage.so.

Domain, from the call sites (map_seed through push_anchor; fast_classify, slow_classify):
  mtch_len       a MEM of at least 19 bases, extended: below 2000 (Q_MEM has 2000 entries); uint16 in the anchor.  Generated: 20 .. 400
  score          Q_MEM[mtch_len] + Q_LV[..] + Q_LV[..], int16; an anchor is pushed only with score > 0 (and >= 20 once rescored), so every group
                 has a positive best score.  A group without one leaves max_anchor at -1 in the reference as well: undefined there, never
                 generated, and refused by the stage entries.  Generated: 1 .. 900
  index_in_read  a position of the read (reads of up to 2^20 bases); ref_offset: any uint32 offset into a reference (also near 2^32)
  ref_ID         23 bits of the reference-position record: 0 .. 2^23 - 1, so also >= 2^21 where the rank sort takes its tie rule
  direction      0 / 1;  useless: 0 / 1 (set by fast_classify / slow_classify);  duplicate: map_seed stores 0 (1 is carried through the sums all the same)
  pre            -1 as map_seed leaves it
Cases are built from colinear runs of anchors with jitter over several references and both strands, shuffled; "probe" groups put one pair
(predecessor, anchor) at a boundary of a rule and move it about the 64-anchor blocks of chain_dp_M3_wave with filler anchors that the
DP skips (they lie behind everything in the read).

Expected, for every forced form that is defined for a case (rank sorts need n <= 1024 / DSB_WTAB_SLOTS / 2 keys, the LDS arrays n <=
DSB_CHAINDP_LDS, the rank selection <= DSB_WTAB_SLOTS / 2 chains): the oracle's anchor order, every pre link, the chains before and after
the selection field by field, n_hit and no status bit -- chain_insert_M2's loop for the M2 form, chain_insert_M3's otherwise, whatever n
is.  resolve_tree itself gives what the reference gives (M2 below 50 anchors), and the forms its own tests lead to are among the forced
ones.  A chain array smaller than the chains gives DSB_ST_HIT_OVF and untouched guard entries; the wave forms also leave the oracle's
chains in front of the overflow.

The coverage conditions (>= 50 cases per class in the full set, >= 5 in the 64-lane subset) are asserted from the oracle's output and the
inputs alone (stage_chain_lib.dp_classes restates the scan in numpy to name the ties, and must agree with the oracle's links)."""
import time

import numpy as np
import pytest

import stage_chain_lib as S

SEED = 10


@pytest.fixture(scope="module")
def ora(built):
    o = S.Oracle2()
    yield o
    o.close()


@pytest.fixture(scope="module")
def full(ora):
    k = S.emu1().k
    t = time.time()
    s = S.build_res_set(k, ora, SEED)
    s.cls = classes(s)
    print("stage a-10: %d cases, %d anchors generated and classified in %.1f s" % (len(s.cases), len(s.rows), time.time() - t))
    return s


# ---- coverage ------------------------------------------------------------------------------------------------------------------
def class_names(k):
    W = ("in", "front1", "front2")
    return ["n=%d" % n for n in S.N_EXACT(k)] + ["group=%d" % g for g in S.GROUP_SIZES[:-1]] + ["group cut at 1024", "group~1500"] + \
           ["break:%s" % d for d in (1999, 2000, 2001, "strand", "ref")] + ["overlap:%s:%+d" % (a, v) for a in "qt" for v in (-1, 0, 1)] + \
           ["dist:%s:%d:%s" % (a, v, w) for a in "qt" for v in (999, 1000, 1001) for w in W] + ["too far inside the block, a link in front of it"] + \
           ["indel:%d" % v for v in (199, 200, 201, 15, 16, 17)] + ["dq>>8:%d" % v for v in (255, 256, 257)] + \
           ["tie:nearest %s" % w for w in W] + ["tie:across chunks", "tie:own score", "equal best:one block", "equal best:across blocks"] + \
           ["equal keys", "equal keys on the tie-rule path", "ref_ID >= 2^21", "negative indel sum", "chains > DSB_WTAB_SLOTS / 2", "chain array overflow"]


FEW = ["n~3000"]          # "a few up to ~3000": present, not fifty of them


def classes(s):
    """class name -> case indices, from the inputs and the oracle's output"""
    cls = {}
    for i, (r, e) in enumerate(zip(s.case_rows, s.exp)):
        n = len(r)
        c = set()
        if n >= 2900:
            c.add("n~3000")
        c.add("n=%d" % n)
        m3 = e[1]
        c |= S.dp_classes(r, m3)
        if n and (r[:, 1] >= 1 << 21).any():
            c.add("ref_ID >= 2^21")
            if "equal keys" in c and 50 <= n <= s.k.RANKSORT_MAX:          # (what resolve_tree itself sorts with the tie rule)
                c.add("equal keys on the tie-rule path")
        if (m3["raw"]["indel"].astype(np.int32) < 0).any():
            c.add("negative indel sum")
        if len(m3["raw"]) > s.k.WTAB_SLOTS // 2:
            c.add("chains > DSB_WTAB_SLOTS / 2")
        if s.ovf[i]:
            c.add("chain array overflow")
        if s.kind[i] == "group=1500" and "group cut at 1024" in c:
            c.add("group~1500")
        for name in c:
            cls.setdefault(name, []).append(i)
    return cls


def test_coverage_of_the_full_set(full):
    names = class_names(full.k)
    print({n: len(full.cls.get(n, [])) for n in names + FEW})
    for n in names:
        assert len(full.cls.get(n, [])) >= 50, (n, len(full.cls.get(n, [])))
    for n in FEW:
        assert len(full.cls.get(n, [])) >= 3, n
    R = full.rows
    assert R[:, 4].min() >= 1 and R[:, 4].max() <= 32767 and R[:, 3].max() < 2000 and R[:, 1].max() < 1 << 23 and R[:, 5].max() <= 1


# ---- the checks, for any leg ---------------------------------------------------------------------------------------------------
def check(leg, s, combos=S.COMBOS, serial_idx=None):
    """every combination of forms over the set; serial_idx: the cases the serial forms run on (all where None).  -> cases that ran, per combination"""
    k = s.k
    ran = {}
    defined_forms = [set() for _ in s.cases]
    nat = [None] * len(s.cases)
    for combo in combos:
        idx = serial_idx if (serial_idx is not None and combo in S.SERIAL_COMBOS) else None
        cs, order, pre, hits, raw = leg.resolve(s, combo, idx)
        ran[combo] = int((cs["defined"] != 0).sum())
        for i, c in enumerate(cs):
            if not c["defined"]:
                continue
            n, a0, cap, ho, ro = int(c["n_anc"]), int(c["a0"]), int(c["hit_cap"]), int(c["hit_off"]), int(c["raw_off"])
            natural = combo == (0, 0, 0)
            e = s.exp[i][(0 if n < 50 else 1) if natural else (0 if combo[1] == S.DP_M2 else 1)]
            tag = (combo, i, s.kind[i], n)
            assert hits[ho + cap:ho + cap + k.GUARD].tobytes() == bytes([S.PATTERN_BYTE]) * (S.CH.itemsize * k.GUARD), ("guard entries", tag)
            if len(e["raw"]) > cap:
                # (the serial forms put every chain that does not fit into the last place, as push_hit does: only the status is defined)
                assert int(c["status"]) == S.ST_HIT_OVF, ("status", tag, int(c["status"]))
                if combo[1] in S.WAVE_DP:
                    assert np.array_equal(order[a0:a0 + n], e["order"]) and np.array_equal(pre[a0:a0 + n], e["pre"]), ("anchors of an overflowing case", tag)
                    assert int(c["n_raw"]) == cap and raw[ro:ro + cap].tobytes() == e["raw"][:cap].tobytes(), ("chains in front of the overflow", tag)
                continue
            assert np.array_equal(order[a0:a0 + n], e["order"]), ("anchor order", tag)
            assert np.array_equal(pre[a0:a0 + n], e["pre"]), ("pre links", tag, np.nonzero(pre[a0:a0 + n] != e["pre"])[0][:5])
            assert int(c["status"]) == 0, ("status", tag, int(c["status"]))
            if not natural:
                assert int(c["n_raw"]) == len(e["raw"]), ("chains before the selection", tag, int(c["n_raw"]), len(e["raw"]))
                got = raw[ro:ro + len(e["raw"])]
                assert got.tobytes() == e["raw"].tobytes(), ("chain records", tag, [(j, got[j], e["raw"][j]) for j in np.nonzero(got != e["raw"])[0][:2]])
                defined_forms[i].add(combo)
                want_sel = 0 if len(e["raw"]) <= 1 else S.SEL_GLIBC if len(e["raw"]) > k.WTAB_SLOTS // 2 else S.SEL_RANK
                assert int(c["nat_sel"]) == want_sel, ("the selection form the entry reports", tag, int(c["nat_sel"]), want_sel)
            else:
                # (the selection form follows from the number of chains the DP leaves, which resolve_tree does not report: the oracle's count)
                nat[i] = (int(c["nat_sort"]), int(c["nat_dp"]), 0 if len(e["raw"]) <= 1 else S.SEL_GLIBC if len(e["raw"]) > k.WTAB_SLOTS // 2 else S.SEL_RANK)
            assert int(c["n_hit"]) == len(e["fin"]), ("n_hit", tag, int(c["n_hit"]), len(e["fin"]))
            got = hits[ho:ho + len(e["fin"])]
            assert got.tobytes() == e["fin"].tobytes(), ("chains after the selection", tag, [(j, got[j], e["fin"][j]) for j in np.nonzero(got != e["fin"])[0][:2]])
    # the forms resolve_tree's own tests lead to are among the forced ones (where all combinations ran)
    if (0, 0, 0) in combos and len(combos) == len(S.COMBOS):
        for i, f in enumerate(nat):
            if f is None or s.ovf[i] or (serial_idx is not None and i not in set(serial_idx)):
                continue
            ok = any((d == S.DP_M2 or so == f[0]) and d == f[1] and (f[2] == 0 or se == f[2]) for so, d, se in defined_forms[i])
            assert ok, ("the dispatcher's forms are not among the forced ones", i, s.kind[i], f, sorted(defined_forms[i]))
    return ran


# ---- leg 1: the 1-lane emulation, the full set --------------------------------------------------------------------------------
def test_one_lane_emulation(full):
    t = time.time()
    ran = check(S.emu1(), full)
    print("1-lane emulation, a-10: %.1f s, cases per combination %r" % (time.time() - t, ran))
    assert all(v >= 500 for v in ran.values()), ran


# ---- leg 2: 64 lanes with the race detector, the cheapest cases of every class ----------------------------------------------------------
def subset64(s, per_class=5):
    idx = set()
    for n in class_names(s.k) + FEW:
        c = sorted(s.cls.get(n, []), key=lambda i: (len(s.case_rows[i]), i))
        idx.update(c[:1 if n in FEW else per_class])
    return sorted(idx)


@pytest.mark.parametrize("order", ["fwd", "rev"])
def test_64_lane_emulation(full, order, monkeypatch):
    if order == "rev":
        monkeypatch.setenv("DSB_EMU_ORDER", "rev")
    leg = S.emu64()
    assert leg.k.lanes == 64
    idx = subset64(full)
    sub = full.subset(idx)
    sub.cls = {}
    for n, members in full.cls.items():
        sub.cls[n] = [j for j, i in enumerate(idx) if i in set(members)]
    for n in class_names(full.k):
        assert len(sub.cls.get(n, [])) >= 5, (n, len(sub.cls.get(n, [])))
    t = time.time()
    leg.findings()
    # (the serial forms are lane 0 alone, every step of it through the detector: on the cases of up to 600 anchors and one larger)
    small = [j for j, r in enumerate(sub.case_rows) if len(r) <= 600]
    big = [j for j, r in enumerate(sub.case_rows) if len(r) > 600]
    check(leg, sub, serial_idx=np.array(small + big[:1], np.int64))
    f = leg.findings()
    assert not f, f
    print("64-lane emulation (%s), a-10: %d cases, %d anchors, %.1f s" % (order, len(sub.cases), len(sub.rows), time.time() - t))


# ---- leg 3: the device -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device(full):
    t = time.time()
    # the serial forms on lane 0 are the expensive ones: every case of up to 1100 anchors, and three of the larger
    n = full.cases["n_anc"]
    serial = np.concatenate([np.nonzero(n <= 1100)[0], np.nonzero(n > 1100)[0][:3]])
    ran = check(S.device(), full, serial_idx=serial)
    print("device, a-10: %.1f s, cases per combination %r" % (time.time() - t, ran))
