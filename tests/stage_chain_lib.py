"""Stages a-10 (resolve_tree), a-13 behind get_score_M2, a-14 (detect_primary) and a-17 (glibc_sort_chains) on their own: ctypes bindings of
the three legs, the oracle entries and the case generators of tests/test_stage_chain.py and tests/test_stage_finish.py.  TEST ONLY; pure
Python + numpy, seeded and deterministic.  The inputs are arrays of anchors (8 u32 a row: index_in_read, ref_ID, ref_offset, mtch_len,
score, direction, useless, duplicate) or of chains (the 48-byte chain_item of dsb_device.h / oracle/oracle.h); tests/stage/dsb_stage_forms.h
describes the flat arrays."""
import ctypes as C
import random

import numpy as np

import oracle_lib
from stage_lib import EMU1, EMU64, STAGE_SO, _ptr

ST_HIT_OVF = 2
SORT_DISTINCT, SORT_TIE, SORT_MERGE = 1, 2, 3
DP_M2, DP_LDS, DP_GLOBAL, DP_SERIAL = 1, 2, 3, 4
SEL_RANK, SEL_GLIBC = 1, 2
WAVE_DP = (DP_LDS, DP_GLOBAL)
# the forced forms every case goes through where they are defined ((0, 0, 0): resolve_tree itself)
COMBOS = [(0, 0, 0), (0, DP_M2, SEL_RANK), (0, DP_M2, SEL_GLIBC)] + [(s, d, SEL_RANK) for s in (SORT_DISTINCT, SORT_TIE, SORT_MERGE) for d in WAVE_DP] + \
         [(SORT_MERGE, DP_SERIAL, SEL_RANK), (SORT_MERGE, DP_SERIAL, SEL_GLIBC), (SORT_MERGE, DP_GLOBAL, SEL_GLIBC)]
SERIAL_COMBOS = [c for c in COMBOS if c[1] in (DP_M2, DP_SERIAL) or c[2] == SEL_GLIBC]

RES = np.dtype([(n, "<u4") for n in ("a0", "n_anc", "hit_cap", "sort", "dp", "sel", "pad0", "pad1")] + [("hit_off", "<u8"), ("raw_off", "<u8")] +
               [(n, "<u4") for n in ("n_raw", "n_hit", "status", "defined", "nat_sort", "nat_dp", "nat_sel", "pad2")])
FIN = np.dtype([(n, "<u4") for n in ("c0", "n", "read_len", "which")] + [(n, "<i4") for n in ("max_read_l", "min_length", "min_score", "min_score_LV3")] +
               [(n, "<u4") for n in ("n_cut", "n_hit", "status")] + [("max_read_l_out", "<i4")])
CH = np.dtype([("ref_ID", "<u4"), ("q_t_dis", "<i4"), ("sum_score", "<u4"), ("anchor_number", "<u4"), ("direction", "u1"), ("with_top_anchor", "u1"), ("primary", "u1"),
               ("pri_index", "u1"), ("t_st", "<u4"), ("t_ed", "<u4"), ("q_st", "<u4"), ("q_ed", "<u4"), ("indel", "<u4"), ("chain_id", "<u4"), ("cur", "<i4")])
PATTERN_BYTE = 0xCD


class Consts2:
    def __init__(self, v):
        (self.sz_res, self.sz_fin, self.sz_chain, self.WTAB_SLOTS, self.RANKSORT_MAX, self.CHAINDP_LDS, self.MAX_ANC, self.MAX_HIT, self.GUARD, self.lanes) = [int(x) for x in v]


def pattern_chains(n):
    return np.frombuffer(bytes([PATTERN_BYTE]) * (CH.itemsize * n), dtype=CH).copy()


class Leg2:
    def __init__(self, path, prefix):
        self.lib = C.CDLL(path)
        out = (C.c_uint32 * 10)()
        getattr(self.lib, "emu_stage_sizes2" if prefix == "emu_stage" else "stage_dev_sizes2")(out)
        self.k = Consts2(out)
        assert (self.k.sz_res, self.k.sz_fin, self.k.sz_chain) == (RES.itemsize, FIN.itemsize, CH.itemsize)
        sz, vp = C.c_size_t, C.c_void_p
        self._res = getattr(self.lib, prefix + "_resolve"); self._res.argtypes = [vp, C.c_uint32, vp, sz, vp, vp, vp, sz, vp, sz]
        self._fin = getattr(self.lib, prefix + "_finish"); self._fin.argtypes = [vp, C.c_uint32, vp, vp, sz]

    def resolve(self, s, combo, idx=None):
        """the cases idx (all) of a ResSet through one combination of forms -> (cases, order, pre, hits, raw); cases not in idx stay undefined"""
        cs = s.cases.copy(); cs["sort"], cs["dp"], cs["sel"] = combo
        run = cs if idx is None else cs[idx].copy()
        order = np.full(len(s.rows), 0xFFFFFFFF, np.uint32); pre = np.full(len(s.rows), -7, np.int32)
        hits = pattern_chains(s.n_hits); raw = pattern_chains(max(1, s.n_raw))
        rc = self._res(_ptr(run), len(run), _ptr(s.rows), len(s.rows), _ptr(order), _ptr(pre), _ptr(hits), len(hits), _ptr(raw), s.n_raw)
        assert rc == 0, "stage library call failed at line %d" % rc
        if idx is None:
            cs = run
        else:
            cs["defined"] = 0; cs[idx] = run
        return cs, order, pre, hits, raw

    def finish(self, cases, chains):
        cs = cases.copy(); ch = chains.copy(); tail = pattern_chains(max(1, len(ch)))
        if len(ch) == 0:
            ch = pattern_chains(1)
        rc = self._fin(_ptr(cs), len(cs), _ptr(ch), _ptr(tail), len(chains))
        assert rc == 0, "stage library call failed at line %d" % rc
        return cs, ch[:len(chains)], tail[:len(chains)]

    def findings(self):
        if not hasattr(self.lib, "dsb_emu_findings"):
            return []
        self.lib.dsb_emu_findings.argtypes = [C.c_char_p, C.c_size_t]
        buf = C.create_string_buffer(1 << 16)
        self.lib.dsb_emu_findings(buf, len(buf))
        return [l for l in buf.value.decode().split("\n") if l]


def emu1():
    return Leg2(EMU1, "emu_stage")


def emu64():
    return Leg2(EMU64, "emu_stage")


def device():
    return Leg2(STAGE_SO, "stage_dev")


class Oracle2:
    def __init__(self):
        L = oracle_lib.lib()
        vp = C.c_void_p
        L.ora_resolve_stage.argtypes = [vp, vp, C.c_uint32, C.c_int, vp, vp, vp, C.c_uint32, vp, vp, C.c_uint32]
        L.ora_finish_stage.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp, C.c_int, C.c_int, C.c_int, vp, vp]
        L.ora_sort_stage.argtypes = [vp, vp, C.c_uint32, C.c_int]
        self.L = L
        self.ctx = L.ora_ctx_new()

    def close(self):
        self.L.ora_ctx_free(self.ctx)

    def resolve(self, rows, m3):
        """-> dict(order, pre, raw, fin): the anchors' places and links, the chains before and after the selection"""
        n = len(rows)
        order = np.zeros(max(1, n), np.uint32); pre = np.zeros(max(1, n), np.int32)
        raw = np.zeros(max(1, n), CH); fin = np.zeros(max(1, n), CH); n_raw = C.c_uint32()
        r = np.ascontiguousarray(rows, np.uint32)
        n_fin = self.L.ora_resolve_stage(self.ctx, _ptr(r), n, 1 if m3 else 0, _ptr(order), _ptr(pre), _ptr(raw), len(raw), C.byref(n_raw), _ptr(fin), len(fin))
        return {"order": order[:n], "pre": pre[:n], "raw": raw[:n_raw.value].copy(), "fin": fin[:n_fin].copy()}

    def finish(self, chains, read_len, max_read_l, min_length, min_score, min_score_lv3):
        ch = chains.copy() if len(chains) else np.zeros(1, CH); tail = np.zeros(max(1, len(chains)), CH)
        mrl = C.c_int(max_read_l); n_cut = C.c_uint32()
        n_hit = self.L.ora_finish_stage(self.ctx, _ptr(ch), len(chains), read_len, C.byref(mrl), min_length, min_score, min_score_lv3, _ptr(tail), C.byref(n_cut))
        return {"n_hit": n_hit, "n_cut": n_cut.value, "max_read_l": mrl.value, "tail": tail[:n_cut.value].copy(), "chains": ch[:n_cut.value].copy()}

    def sort(self, chains, which):
        ch = chains.copy() if len(chains) else np.zeros(1, CH)
        self.L.ora_sort_stage(self.ctx, _ptr(ch), len(chains), which)
        return ch[:len(chains)]


# ---- a-10: anchors ------------------------------------------------------------------------------------------------------------
def A(q, ref, t, ml, score, strand, useless=0, dup=0):
    return (q & 0xFFFFFFFF, ref, t & 0xFFFFFFFF, ml, score, strand, useless, dup)


def colinear_run(rng, ref, strand, q0, t0, n, tight=False):
    """n anchors along one diagonal with jitter: gaps of -5 .. 300 bases (tight: 0 .. 12), now and then an indel of up to 250 or a long step"""
    out = []
    q, t = q0, t0
    for _ in range(n):
        ml = rng.randint(20, 30) if tight else rng.choice([20, 21, 25, 33, 60, 120, 400])
        out.append(A(q, ref, t, ml, rng.randint(1, 40) if rng.random() < 0.3 else rng.randint(20, 2 * ml + 40), strand, int(rng.random() < 0.4), int(rng.random() < 0.03)))
        step = ml + (rng.randint(0, 12) if tight else rng.choice([-5, -3, 0, 1, 7, 40, 150, 300]))
        ind = rng.choice([0, 0, 0, 1, -1, 8, -17, 33, -150, 199, -200, 201, 250]) if rng.random() < 0.35 else 0
        if rng.random() < 0.04 and not tight:
            step += rng.choice([600, 980, 1100, 1995, 2000, 2600])
        q += max(1, step + (ind if ind > 0 else 0)); t += max(1, step - (ind if ind < 0 else 0))
    return out


def fillers(rng, ref, strand, t_lo, t_hi, n, q_big):
    """n anchors with offsets in [t_lo, t_hi] (ascending) and read positions descending from q_big: each overlaps every later one in the read,
    and lies behind every probe anchor, so the DP skips them as predecessors of anything"""
    ts = sorted(rng.randint(t_lo, t_hi) for _ in range(n))
    return [A(q_big + 40 * (n - k), ref, ts[k], 20, rng.randint(1, 5), strand, 1, 0) for k in range(n)]


def probe_group(rng, ref, strand, t_base, kind, val):
    """one group around a pair (P, C) at a boundary of the DP's rules, with fillers that move the pair about the 64-anchor blocks:
    a fillers in front of P, b between P and C (b < 64: same block possible; 64 ..: P one or two chunks in front), c behind"""
    a, b, c = rng.randint(0, 130), rng.choice([0, 1, 3, 20, 62, 63, 64, 65, 70, 100, 127, 128, 130, 140]), rng.randint(0, 20)
    cq, ct = rng.randint(4000, 60000), t_base + 1500
    cml, pml = rng.randint(20, 60), rng.randint(20, 60)
    dq = rng.randint(pml + 5, 250); dt = dq + rng.choice([0, 0, 1, -2, 5, -9])                  # c + 3 - p on each axis
    extra = []
    if kind in ("dist_q", "dist_t"):
        d, o = val, val - rng.choice([0, 1, 20, 150])
        dq, dt = (d, o) if kind == "dist_q" else (o, d)
    elif kind in ("ovl_q", "ovl_t"):
        d = rng.randint(23, 400); pml = d + val; o = d + rng.randint(2, 40)
        dq, dt = (d, o) if kind == "ovl_q" else (o, d)
    elif kind == "indel":
        dq = rng.randint(300, 700); dt = dq - val                                                  # indel = (p_q - p_t) - (max_q - max_t) = dt - dq
    elif kind == "shift8":
        dq = val; dt = dq + rng.choice([0, 3, -3])
    P = A(cq + 3 - dq, ref, ct + 3 - dt, pml, rng.randint(30, 120), strand, int(rng.random() < 0.5))
    own = rng.randint(1, 60)
    if kind == "tie":
        # two predecessors that give C the same score, each without a predecessor of its own (they overlap in the read): the nearer one wins
        pml = 30; s = rng.randint(30, 90)
        P = A(cq + 3 - dq, ref, ct + 3 - dt, pml, s, strand)
        d2 = rng.randint(0, 12)                                                                    # P2 nearer on both axes by d2 < mtch_len
        extra = [A(cq + 3 - dq + d2, ref, ct + 3 - dt + d2, pml - min(d2, 8), s, strand)]
        if val == "own":                                                                           # ... or C's own score equals what they give: no link
            own = s + cml - (abs(dt - dq) >> 4) - (dq >> 8)
    if kind == "far_in":
        # X between P and C in the sort order, not overlapping C and more than 1000 bases in front of it in the read: the reference stops there
        # and never sees P; b2 fillers between X and C keep X in C's block where b2 < its lane
        extra = [A(cq - rng.randint(1100, 3000), ref, ct - rng.randint(0, 15), 20, rng.randint(1, 9), strand)]
        b = rng.choice([0, 2, 40, 64, 70])
    Cc = A(cq, ref, ct, cml, own, strand, int(rng.random() < 0.5))
    pt = P[2]
    q_big = cq + 5000
    g = fillers(rng, ref, strand, max(0, pt - 900), pt, a, q_big) + [P]
    if kind == "tie":
        b1 = rng.choice([0, 5, 30, 64, 70, 100])
        g += fillers(rng, ref, strand, pt, extra[0][2], b1, q_big + 6000) + extra
        g += fillers(rng, ref, strand, extra[0][2], ct, b, q_big + 12000)
    elif kind == "far_in":
        xt = extra[0][2]
        g += fillers(rng, ref, strand, pt, max(pt, xt), b, q_big + 6000) + extra + fillers(rng, ref, strand, xt, ct, rng.choice([0, 1, 5, 30]), q_big + 12000)
    else:
        g += fillers(rng, ref, strand, pt, ct, b, q_big + 6000)
    g += [Cc] + fillers(rng, ref, strand, ct, ct + 800, c, q_big + 18000)
    return g


PROBES = [(k, v) for k in ("dist_q", "dist_t") for v in (999, 1000, 1001)] + [(k, v) for k in ("ovl_q", "ovl_t") for v in (-1, 0, 1)] + \
         [("indel", s * v) for v in (199, 200, 201, 15, 16, 17, 31, 32) for s in (1, -1)] + [("shift8", v) for v in (255, 256, 257, 511, 512, 513)] + \
         [("tie", "near")] * 6 + [("tie", "own"), ("far_in", 0), ("far_in", 0)]


def equal_best_group(rng, ref, strand, t_base):
    """two anchors with the group's best score, neither reachable from the other, n fillers between them: the first one is the chain's end"""
    s = rng.randint(200, 900); q = rng.randint(4000, 50000); b = rng.choice([0, 3, 40, 63, 64, 100, 130, 150])
    a = rng.randint(0, 70)
    g = fillers(rng, ref, strand, t_base, t_base + 300, a, q + 9000) + [A(q, ref, t_base + 300, 50, s, strand)]
    g += fillers(rng, ref, strand, t_base + 300, t_base + 700, b, q + 19000) + [A(q - 2000, ref, t_base + 700, 50, s, strand)]
    return g


def break_groups(rng, strand, t_base, d):
    """two runs whose offsets differ by d (1999, 2000, 2001) where they meet; ... or equal offsets on another strand / reference"""
    ref = rng.randint(0, 5000)
    g = colinear_run(rng, ref, strand, 1000, t_base, rng.randint(1, 6), tight=True)
    last_t = max(r[2] for r in g)
    if d == "strand":                          # (strand 0 sorts first: its last offset is the other strand's first)
        g = [A(r[0], ref, r[2], r[3], r[4], 0) for r in g]
        return g + colinear_run(rng, ref, 1, 1000, last_t, rng.randint(1, 6), tight=True)
    if d == "ref":
        return g + colinear_run(rng, ref + 1, strand, 1000, last_t, rng.randint(1, 6), tight=True)
    return g + colinear_run(rng, ref, strand, 1000 + (last_t - t_base) + d, last_t + d, rng.randint(1, 6), tight=True)


def big_group(rng, ref, strand, t_base, n):
    """n anchors in one group (steps below 2000): several interleaved diagonals of tight runs"""
    out = []
    k = max(1, n // rng.choice([40, 90, 200]))
    per = [n // k + (1 if i < n % k else 0) for i in range(k)]
    for i, m in enumerate(per):
        out += colinear_run(rng, ref, strand, rng.randint(0, 3000) + 50 * i, t_base + rng.randint(0, 30), m, tight=True)
    return out


def pad_to(rng, rows, n, many_chains=False):
    """singles on references of their own (a chain each) until the case has n anchors"""
    k = 0
    while len(rows) < n:
        ref = (1 << 22) + 7 * len(rows) + k if not many_chains else 100000 + len(rows)
        rows.append(A(rng.randint(0, 90000), ref, rng.randint(0, 1 << 30), rng.randint(20, 90), rng.randint(1, 300), rng.randint(0, 1), int(rng.random() < 0.5)))
    return rows[:n]


class ResSet:
    def __init__(self, k):
        self.k = k; self.case_rows = []; self.kind = []

    def add(self, rng, rows, kind="", shuffle=True):
        rows = list(rows)
        if shuffle:
            rng.shuffle(rows)
        assert len(rows) <= self.k.MAX_ANC
        self.case_rows.append(np.array(rows, np.uint32).reshape(-1, 8)); self.kind.append(kind)

    def finish(self, ora, ovf_every=23):
        k = self.k
        self.exp = []
        rows = []; a0 = hoff = roff = 0
        cs = np.zeros(len(self.case_rows), RES)
        self.ovf = np.zeros(len(cs), bool)
        for i, r in enumerate(self.case_rows):
            e = (ora.resolve(r, False), ora.resolve(r, True))
            self.exp.append(e)
            n_raw = max(len(e[0]["raw"]), len(e[1]["raw"]))
            cap = n_raw + 4
            if ovf_every and i % ovf_every == 0 and len(e[1]["raw"]) >= 2 and len(e[0]["raw"]) >= 2:
                cap = max(1, min(len(e[0]["raw"]), len(e[1]["raw"])) // 2); self.ovf[i] = True
            assert cap <= k.MAX_HIT
            cs[i]["a0"], cs[i]["n_anc"], cs[i]["hit_cap"], cs[i]["hit_off"], cs[i]["raw_off"] = a0, len(r), cap, hoff, roff
            a0 += len(r); hoff += cap + k.GUARD; roff += cap
            rows.append(r)
        self.cases = cs
        self.rows = np.concatenate(rows) if a0 else np.zeros((1, 8), np.uint32)
        self.rows = np.ascontiguousarray(self.rows)
        self.n_hits, self.n_raw = hoff, roff
        return self

    def subset(self, idx, ora_unused=None):
        s = ResSet(self.k)
        s.case_rows = [self.case_rows[i] for i in idx]; s.kind = [self.kind[i] for i in idx]; s.exp = [self.exp[i] for i in idx]; s.ovf = self.ovf[idx].copy()
        cs = self.cases[idx].copy()
        n = cs["n_anc"].astype(np.int64); cap = cs["hit_cap"].astype(np.int64)
        cs["a0"] = np.concatenate([[0], np.cumsum(n)[:-1]]); cs["hit_off"] = np.concatenate([[0], np.cumsum(cap + self.k.GUARD)[:-1]]); cs["raw_off"] = np.concatenate([[0], np.cumsum(cap)[:-1]])
        s.cases = cs
        s.rows = np.ascontiguousarray(np.concatenate([r for r in s.case_rows] + [np.zeros((1, 8), np.uint32)]))
        s.n_hits, s.n_raw = int((cap + self.k.GUARD).sum()), int(cap.sum())
        return s


N_EXACT = lambda k: [0, 1, 49, 50, 51, k.CHAINDP_LDS, k.CHAINDP_LDS + 1, k.RANKSORT_MAX, k.RANKSORT_MAX + 1, 1024, 1025]
GROUP_SIZES = [1, 63, 64, 65, 128, 129, 1023, 1024, 1025, 1500]


def build_res_set(k, ora, seed, per_class=52):
    """Domain and classes: see the module docstring of tests/test_stage_chain.py."""
    rng = random.Random(seed)
    s = ResSet(k)
    sizes = N_EXACT(k)
    # 1. probes: one or a few probe groups on references of their own, the case padded with singles to one of the exact sizes now and then
    for rep in range(per_class):
        for kind, val in PROBES:
            rows = []
            for gi in range(rng.choice([1, 1, 2])):
                ref = rng.randint(0, 3000) + ((1 << 21) if rng.random() < 0.15 else 0)
                rows += probe_group(rng, ref, rng.randint(0, 1), rng.randint(0, 1 << 28), kind, val)
            s.add(rng, rows, "probe:%s:%s" % (kind, val))
        for _ in range(3):
            rows = []
            for gi in range(rng.choice([1, 2])):
                rows += equal_best_group(rng, rng.randint(0, 3000), rng.randint(0, 1), rng.randint(0, 1 << 28))
            s.add(rng, rows, "equal best")
        for d in (1999, 2000, 2001, "strand", "ref"):
            s.add(rng, break_groups(rng, rng.randint(0, 1), rng.randint(0, 1 << 28), d) + colinear_run(rng, 7000, 1, 50, 100, rng.randint(40, 70)), "break:%s" % d)
    # 2. the exact sizes: random runs over several references and both strands, equal sort keys among them
    for n in sizes:
        for rep in range(per_class):
            rows = []
            hi_ref = rep % 4 == 0
            while len(rows) < n:
                ref = rng.randint(0, 40) + ((1 << 21) + (1 << 22) * rng.randint(0, 1) if hi_ref else 0)
                run = colinear_run(rng, ref, rng.randint(0, 1), rng.randint(0, 5000), rng.randint(0, 1 << 20) if rng.random() < 0.8 else 0xFFF00000, rng.randint(1, 60), tight=rng.random() < 0.5)
                if rng.random() < 0.3:                     # the same anchors once more: equal keys, the sort must keep their order
                    run += [A(r[0] + rng.choice([0, 30]), r[1], r[2], r[3], rng.randint(1, 300), r[5]) for r in run[:rng.randint(1, 5)]]
                rows += run
            rng.shuffle(rows)
            s.add(rng, rows[:n], "n=%d" % n)
    # 3. the group sizes (one large group, the 1024 cut and the group that starts behind it), a few sets of ~3000 anchors
    for g in GROUP_SIZES:
        for rep in range(per_class):
            rows = big_group(rng, rng.randint(0, 100), rng.randint(0, 1), rng.randint(0, 1 << 24), g)
            rows += colinear_run(rng, 200, 0, 10, 10, rng.randint(0, 60))
            s.add(rng, pad_to(rng, rows, max(len(rows), 50)), "group=%d" % g)
    for rep in range(3):
        s.add(rng, pad_to(rng, big_group(rng, 5, 1, 1000, 1200) + big_group(rng, 9, 0, 1000, 700), k.MAX_ANC - rep * 40), "n~3000")
    # 4. more chains than the rank selection's keys have room for; they also are more than a small hit_cap holds
    for rep in range(per_class):
        s.add(rng, pad_to(rng, colinear_run(rng, 3, 1, 0, 0, 30), k.WTAB_SLOTS // 2 + 40 + rep % 7, many_chains=True), "chains>%d" % (k.WTAB_SLOTS // 2))
    return s.finish(ora)


def dp_classes(rows, e, max_group=700):
    """the classes of one case that follow from its anchors in the oracle's order and the oracle's links: a plain restatement of the DP's scan per
    group in numpy, whose links must be the oracle's (asserted), and the geometry of every (predecessor, anchor) pair"""
    cls = set()
    R = rows[e["order"]].astype(np.int64)
    n = len(R)
    if n == 0:
        return cls
    q, ref, t, ml, sc, sd = R[:, 0], R[:, 1], R[:, 2], R[:, 3], R[:, 4], R[:, 5]
    key = ref * 2 + sd
    newg = np.ones(n, bool)
    newg[1:] = (key[1:] != key[:-1]) | (((t[1:] - t[:-1]) & 0xFFFFFFFF) >= 2000)
    same = key[1:] == key[:-1]
    d = (t[1:] - t[:-1])[same]
    for v in (1999, 2000, 2001):
        if (d == v).any():
            cls.add("break:%d" % v)
    if ((t[1:] == t[:-1]) & (ref[1:] == ref[:-1]) & (sd[1:] != sd[:-1])).any():
        cls.add("break:strand")
    if ((t[1:] == t[:-1]) & (ref[1:] != ref[:-1])).any():
        cls.add("break:ref")
    if (same & (t[1:] == t[:-1])).any():
        cls.add("equal keys")
    starts = list(np.nonzero(newg)[0]) + [n]
    bounds = []
    for a, b in zip(starts[:-1], starts[1:]):
        for g in GROUP_SIZES[:-1]:
            if b - a == g:
                cls.add("group=%d" % g)
        while b - a > 1024:
            bounds.append((a, a + 1024)); a += 1024
            cls.add("group cut at 1024")
        bounds.append((a, b))
    for a, b in bounds:
        m = b - a
        if m <= 1 or m > max_group:
            continue
        Q, T, M, S = q[a:b], t[a:b], ml[a:b], sc[a:b]
        mq, mt = Q[None, :] + 3, T[None, :] + 3                                   # [i, j]: predecessor i of anchor j
        tri = np.triu(np.ones((m, m), bool), 1)
        eq, et = Q[:, None] + M[:, None] - mq, T[:, None] + M[:, None] - mt
        ovl = (eq > 0) | (et > 0)
        dq, dt = mq - Q[:, None], mt - T[:, None]
        far = ~ovl & ((dq > 1000) | (dt > 1000))
        ind = dt - dq
        ok = tri & ~ovl & ~far & (np.abs(ind) <= 200)
        blk0 = (np.arange(m) // 64 * 64)[None, :]
        ii = np.arange(m)[:, None]
        where = np.where(ii >= blk0, 0, np.where(ii >= blk0 - 64, 1, 2))           # 0 inside the block, 1 / 2: the first / a later chunk in front
        W = ("in", "front1", "front2")
        for ax, dd, od in (("q", dq, dt), ("t", dt, dq)):
            for v in (999, 1000, 1001):
                hit = tri & ~ovl & (dd == v) & (od <= 1000)
                for wv in range(3):
                    if (hit & (where == wv)).any():
                        cls.add("dist:%s:%d:%s" % (ax, v, W[wv]))
        for ax, ee, oo in (("q", eq, et), ("t", et, eq)):
            for v in (-1, 0, 1):
                if (tri & (ee == v) & (oo <= -1) & ~((dq > 1000) | (dt > 1000))).any():
                    cls.add("overlap:%s:%+d" % (ax, v))
        near = tri & ~ovl & ~far
        for v in (199, 200, 201, 15, 16, 17):
            if (near & (np.abs(ind) == v)).any():
                cls.add("indel:%d" % v)
        for v in (255, 256, 257):
            if (ok & (dq == v)).any():
                cls.add("dq>>8:%d" % v)
        # the scan, anchor by anchor: predecessors from the nearest back to the first one that is too far
        sv = np.zeros(m, np.int64); pre = np.full(m, -1, np.int64)
        for j in range(m):
            best = S[j]
            if j:
                f = np.nonzero(far[:j, j])[0]
                lo = f[-1] + 1 if len(f) else 0
                c = np.nonzero(ok[lo:j, j])[0] + lo
                if len(c):
                    ns = sv[c] + M[j] - (np.abs(ind[c, j]) >> 4) - (dq[c, j] >> 8)
                    top = ns.max()
                    if top > best:
                        w_ = c[ns == top]
                        best = top; pre[j] = w_[-1]
                        if len(w_) > 1:
                            ws = sorted(set(int(where[x, j]) for x in w_))
                            cls.add("tie:nearest %s" % W[int(where[w_[-1], j])])
                            if len(ws) > 1:
                                cls.add("tie:across chunks")
                    elif top == best:
                        cls.add("tie:own score")
                if len(f) and where[f[-1], j] == 0:
                    # ... and a predecessor in front of the block that the block DP has taken by then: admissible, not behind a too-far one of the
                    # front scan (nearest first), and better than the anchor's own score
                    fr = np.nonzero(where[:j, j] > 0)[0]
                    ff = [x for x in fr if far[x, j]]
                    cand = [x for x in fr if ok[x, j] and (not ff or x > ff[-1])]
                    if any(sv[x] + M[j] - (abs(int(ind[x, j])) >> 4) - (int(dq[x, j]) >> 8) > S[j] for x in cand):
                        cls.add("too far inside the block, a link in front of it")
            sv[j] = best
        assert np.array_equal(np.where(pre >= 0, pre + a, -1), e["pre"][a:b]), "the restated scan and the oracle disagree"
        top = np.nonzero(sv == sv.max())[0]
        if len(top) > 1:
            cls.add("equal best:" + ("one block" if top[0] // 64 == top[1] // 64 else "across blocks"))
    return cls


# ---- a-13 / a-14 / a-17: chains -----------------------------------------------------------------------------------------------------
def chain(ref=0, strand=1, t_st=0, t_ed=0, q_st=0, q_ed=0, score=100, anchors=3, indel=0, top=1, cur=0):
    c = np.zeros(1, CH)[0]
    c["ref_ID"], c["direction"], c["t_st"], c["t_ed"], c["q_st"], c["q_ed"], c["sum_score"], c["anchor_number"] = ref, strand, t_st & 0xFFFFFFFF, t_ed & 0xFFFFFFFF, q_st & 0xFFFFFFFF, q_ed & 0xFFFFFFFF, score, anchors
    c["indel"], c["with_top_anchor"], c["cur"], c["q_t_dis"] = indel & 0xFFFFFFFF, top, cur, (t_st - q_st) & 0x7FFFFFFF
    return c
