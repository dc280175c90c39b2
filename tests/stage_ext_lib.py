"""The sparse DP of stage a-12 (the predecessor scans of sdp_middle_M2 / sdp_right_M2 / sdp_left_M2) on bare node lists: ctypes bindings of
the three legs, the generator of the node lists, and a numpy restatement of the reference's newest-first scan that says which
boundaries a list exercises (tests/test_stage_dp.py).  TEST ONLY; pure Python + numpy, seeded and deterministic.

A node list is an (n, 4) uint32 array of t_pos, q_pos, len, score; node 0 carries its score (the seed of an extension, or the anchor in
front of a gap), the other scores are what a form has to produce.  The oracle (oracle/classify.c: ora_sdp_dp_stage, the very functions
ora_classify runs) gives the expected scores."""
import ctypes as C
import random

import numpy as np

import oracle_lib
import stage_lib as S

MIDDLE, RIGHT, LEFT = 0, 1, 2
FORMS = {"pred": 0, "batch": 1, "block": 2, "mw": 3}
PATTERN = S.PATTERN
M32 = 0xFFFFFFFF

DP = np.dtype([(n, "<u4") for n in ("n", "mode", "form", "waves", "s0", "n_sizes", "heavy_limit", "pad0")] + [("node_off", "<u8")] +
              [(n, "<u4") for n in ("status", "dp_preds", "scored", "defined")])


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


class DpLeg:
    def __init__(self, path, prefix):
        self.lib = C.CDLL(path)
        out = (C.c_uint32 * 8)()
        getattr(self.lib, "emu_stage_sizes_dp" if prefix == "emu_stage" else "stage_dev_sizes_dp")(out)
        self.sz, self.GUARD, self.RING, self.DPB, self.UNROLL, self.lanes, self.MAXW, self.ST_HEAVY = [int(x) for x in out]
        assert self.sz == DP.itemsize
        self._dp = getattr(self.lib, prefix + "_dp")
        self._dp.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]

    def run(self, s, form, idx=None, sizes=None, waves=0, heavy=None):
        """one form over the lists idx of a DpSet -> (cases with their out fields, the node blob afterwards)
        sizes: per list, the block / batch sizes the form takes in turn (None: the callers' own); heavy: per list, heavy_limit"""
        idx = list(range(len(s.lists))) if idx is None else list(idx)
        cs = np.zeros(len(idx), DP)
        blob, off, zs = [], 0, []
        for k, i in enumerate(idx):
            N = s.lists[i]
            reg = np.full((len(N) + self.GUARD, 4), PATTERN, np.uint32)
            reg[:len(N), :3] = N[:, :3]
            if len(N):
                reg[0, 3] = N[0, 3]
            z = [] if sizes is None else list(sizes[k])
            cs[k] = (len(N), s.modes[i], FORMS[form], waves, len(zs), len(z), 0 if heavy is None else heavy[k], 0, off, 0, 0, 0, 0)
            zs += z
            blob.append(reg); off += len(reg)
        nodes = np.concatenate(blob) if blob else np.zeros((0, 4), np.uint32)
        za = np.array(zs + [0], np.uint32)
        rc = self._dp(_ptr(cs), len(cs), _ptr(nodes), len(nodes), _ptr(za), len(za) - 1)
        assert rc == 0, "stage library call failed at line %d" % rc
        return cs, nodes

    def findings(self):
        if not hasattr(self.lib, "dsb_emu_findings"):
            return []
        self.lib.dsb_emu_findings.argtypes = [C.c_char_p, C.c_size_t]
        buf = C.create_string_buffer(1 << 16)
        self.lib.dsb_emu_findings(buf, len(buf))
        return [l for l in buf.value.decode().split("\n") if l]


def emu1():
    return DpLeg(S.EMU1, "emu_stage")


def emu64():
    return DpLeg(S.EMU64, "emu_stage")


def device():
    return DpLeg(S.STAGE_SO, "stage_dev")


def oracle_scores(mode, N):
    L = oracle_lib.lib()
    L.ora_sdp_dp_stage.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p]
    L.ora_sdp_dp_stage.restype = None
    N = np.ascontiguousarray(N, np.uint32)
    out = np.zeros(max(1, len(N)), np.int32)
    L.ora_sdp_dp_stage(mode, _ptr(N), len(N), _ptr(out))
    return out[:len(N)]


# ---- the reference's scan, restated: what a list exercises --------------------------------------------------------------------------
def _s32(x):
    return ((x & M32) ^ 0x80000000) - 0x80000000


def _judge(mode, t, q, l, pt, pq, pl, psc):
    """one node against predecessors (arrays, int64 holding uint32 values), in C's arithmetic (src/cly.c:2495-2517, 2612-2638, 2759-2783)
    -> skip, brk, ai, ns, ovl (the overlap the first test and the penalty look at), wrapped predecessor (as the kernels define it)"""
    if mode == LEFT:
        lq, lt = (q + l + 2) & M32, (t + l + 2) & M32
        skip = (pq < lq) | (pt < lt)
        brk = ~skip & (((lt + 600) & M32) < pt)
        nq, nt = (lq + 6) & M32, (lt + 6) & M32
        ov = (nq > pq) | (nt > pt)
        oq, ot = _s32(nq - pq), _s32(nt - pt)
        wrapped = (pq | pt) >= 0x80000000
    else:
        lq, lt = (q + 6) & M32, (t + 6) & M32
        pqe, pte = (pq + pl + 8) & M32, (pt + pl + 8) & M32
        skip = (pqe > lq) | (pte > lt)
        brk = ~skip & (((pt + 600) & M32) < lt) if mode == RIGHT else np.zeros(len(pt), bool)
        ov = (pqe > q) | (pte > t)
        oq, ot = _s32(pqe - q), _s32(pte - t)
        wrapped = (pqe | pte | ((pt + 600) & M32)) >= 0x80000000
    indel = _s32(pq - pt - (lq - lt))
    ai = np.abs(indel)
    ovl = np.maximum(oq, ot)
    ns = _s32(psc + l - (ai >> 3))
    ns = np.where(ov, _s32(ns - ovl), ns)
    return skip, brk, ai, ns, ovl, ov, wrapped


def node_wrapped(mode, t, q, l):
    if mode == LEFT:
        lq, lt = (q + l + 2) & M32, (t + l + 2) & M32
        v = lq | lt | ((lq + 6) & M32) | ((lt + 6) & M32) | ((lt + 600) & M32)
    else:
        lq, lt = (q + 6) & M32, (t + 6) & M32
        v = lq | lt | q | t | ((lt + 600) & M32)
    return v >= 0x80000000


def _scan(mode, N, sc, cur, hi, out=None):
    """the newest-first scan of node cur over the predecessors [0, hi) -> (best score or None if no predecessor counted, distance of the
    cut from cur or 0, distance of the best predecessor or 0); out: a dict that collects what the predecessors it reached were like"""
    t, q, l = int(N[cur, 0]), int(N[cur, 1]), int(N[cur, 2])
    best, bd, size = None, 0, 64
    while hi > 0:
        lo = max(0, hi - size)
        P = N[lo:hi][::-1].astype(np.int64)
        skip, brk, ai, ns, ovl, ov, wr = _judge(mode, t, q, l, P[:, 0], P[:, 1], P[:, 2], sc[lo:hi][::-1] & M32)
        fb = int(np.argmax(brk)) if brk.any() else len(P)
        ok = ~skip & ~brk & (ai <= 200)
        ok[fb:] = False
        if out is not None:
            r = slice(0, min(fb + 1, len(P)))
            out["ovl7"] |= bool((skip[r] & (ovl[r] == 7)).any()); out["ovl6"] |= bool((ok[r] & ov[r] & (ovl[r] == 6)).any()); out["ovl0"] |= bool((ok[r] & (ovl[r] == 0)).any())
            ns_ = ~skip[r] & ~brk[r]
            out["ai200"] |= bool((ns_ & (ai[r] == 200)).any()); out["ai201"] |= bool((ns_ & (ai[r] == 201)).any())
            out["ai7"] |= bool((ok[r] & (ai[r] % 8 == 7)).any()); out["ai8"] |= bool((ok[r] & (ai[r] >= 8) & (ai[r] % 8 == 0)).any())
            out["wpred"] |= bool(wr[r].any())
        if ok.any():
            v = np.where(ok, ns, -(1 << 40)); k = int(np.argmax(v))
            if best is None or int(v[k]) > best:
                best, bd = int(v[k]), cur - (hi - 1 - k)
                if out is not None:
                    out["best_pen"] = bool(ov[k]) and int(ovl[k]) > 0; out["best_ai"] = int(ai[k])
        if fb < len(P):
            return best, cur - (hi - 1 - fb), bd
        hi = lo; size = 256 if size == 64 else 8192         # (the chunks are this function's own: the scan's result does not depend on them)
    return best, 0, bd


CLASSES = ["no predecessor in reach", "cut inside the newest 64", "cut in a later chunk", "cut never met", "best predecessor inside the batch",
           "best predecessor inside the block", "in-batch cut discards an old-pass best", "in-block cut discards an old-pass best",
           "reach <= 8", "reach 9 .. 16", "reach 17 .. 64", "reach 65 .. 256", "reach > 256", "overlap 0", "overlap 6", "overlap 7",
           "overlap penalty applied", "|indel| 200", "|indel| 201", ">> 3 step", "indel penalty applied", "wrapped node", "wrapped predecessor"]
TANDEM = "hundreds of nodes at one t_pos"


def restate(mode, N, DPB=8, BLK=64):
    """-> (scores by the restatement, the set of classes the list is in).  reach = predecessors the scan looks at (the cut one included)"""
    n = len(N)
    sc = np.zeros(n, np.int64)
    cls = set()
    if n:
        sc[0] = int(N[0, 3])
    for cur in range(1, n):
        o = dict(ovl7=False, ovl6=False, ovl0=False, ai200=False, ai201=False, ai7=False, ai8=False, wpred=False, best_pen=False, best_ai=0)
        best, cut, bd = _scan(mode, N, sc, cur, cur, o)
        own = _s32(int(N[cur, 2]))
        score = own if best is None or best < own else best
        sc[cur] = score & M32
        reach = cut if cut else cur
        took = best is not None and best > own
        if best is None:
            cls.add("no predecessor in reach")
        if mode != MIDDLE:
            cls.add("cut never met" if not cut else "cut inside the newest 64" if cut <= 64 else "cut in a later chunk")
            for name, b0 in (("batch", 1 + DPB * ((cur - 1) // DPB)), ("block", 1 + BLK * ((cur - 1) // BLK))):
                if took and cur - bd >= b0:
                    cls.add("best predecessor inside the %s" % name)
                if cut and cur - cut >= b0 and b0 > 1:
                    ob, _, _ = _scan(mode, N, sc, cur, b0)
                    if ob is not None and ob > score:
                        cls.add("in-%s cut discards an old-pass best" % name)
        cls.add("reach <= 8" if reach <= 8 else "reach 9 .. 16" if reach <= 16 else "reach 17 .. 64" if reach <= 64 else "reach 65 .. 256" if reach <= 256 else "reach > 256")
        for k, name in (("ovl0", "overlap 0"), ("ovl6", "overlap 6"), ("ovl7", "overlap 7"), ("ai200", "|indel| 200"), ("ai201", "|indel| 201"), ("wpred", "wrapped predecessor")):
            if o[k]:
                cls.add(name)
        if o["ai7"] and o["ai8"]:
            cls.add(">> 3 step")
        if took and o["best_pen"]:
            cls.add("overlap penalty applied")
        if took and o["best_ai"] >= 8:
            cls.add("indel penalty applied")
        if bool(node_wrapped(mode, int(N[cur, 0]), int(N[cur, 1]), int(N[cur, 2]))):
            cls.add("wrapped node")
    if n > 1 and np.unique(N[1:, 0], return_counts=True)[1].max() >= 200:
        cls.add(TANDEM)
    return _s32(sc).astype(np.int32), cls


# ---- node lists ----------------------------------------------------------------------------------------------------------------------
def gen_right(rng, n, style):
    """n nodes of a right extension (or, with a plain first node, of a gap): a seed and what windows of 600 bases append, ascending in t
    but for the few bases a match is extended backwards; style weighs the stretches the list is made of"""
    t = rng.randint(2000, 1 << 20)
    q = rng.choice([0, 3, 9, 600, rng.randint(0, 15000)])
    if style == "wrap":
        q = rng.choice([M32, M32, 0, 1])                     # a chain that ends at q = -1 (wrapped), or at the very start of the read
    seed_len = (rng.choice([1 - 9, 1 - 9, -9])) & M32
    if style == "gap":
        seed_len = rng.randint(5, 50)
    out = [(t, q, seed_len)]
    dq = (q if q < (1 << 31) else q - (1 << 32)) - t + (seed_len if style == "gap" else 0) + 8
    if style != "gap":
        t -= 3
    else:
        t += seed_len + 8
    w = {"walk": dict(step=60, same=6, jump=6, ovl=10, indel=10, back=4, tandem=0), "sparse": dict(step=30, same=2, jump=30, ovl=8, indel=8, back=14, tandem=0),
         "dense": dict(step=70, same=20, jump=1, ovl=10, indel=10, back=1, tandem=0), "tandem": dict(step=10, same=5, jump=1, ovl=3, indel=3, back=1, tandem=12),
         "wrap": dict(step=60, same=6, jump=6, ovl=10, indel=10, back=4, tandem=0), "gap": dict(step=60, same=10, jump=2, ovl=12, indel=12, back=1, tandem=0)}[style]
    kinds = [k for k, v in w.items() for _ in range(v)]
    first = True
    while len(out) < n:
        kind = rng.choice(kinds)
        if first and style == "wrap":                          # nodes in front of the read's first base: the window starts at q_st - 8
            kind = "neg"
        first = False
        if kind == "neg":
            for _ in range(rng.randint(1, 6)):
                t += 4
                out.append((t, (-rng.randint(1, 8)) & M32, rng.randint(1, 12)))
            dq = rng.randint(0, 8) - t
        elif kind == "step":
            dense = style in ("dense", "tandem")
            for _ in range(rng.randint(1, 24)):
                t += rng.choice([0, 0, 1, 1, 4]) if dense else rng.choice([4, 4, 8, 12, 16, 4 * rng.randint(1, 12)])
                dq += rng.choice([0, 0, 0, 0, 1, -1, 2, -2, rng.randint(-30, 30)])
                out.append((t, max(0, t + dq), rng.choice([1, 1, 2, 3, 5, 8, 12, 20, rng.randint(1, 60)])))
        elif kind == "same":
            p, ln = rng.randint(1, 9), rng.randint(1, 30)
            for i in range(rng.randint(2, 12)):
                out.append((t, max(0, t + dq + i * p), ln))
        elif kind == "tandem":
            p, ln, reps = rng.randint(2, 9), rng.randint(1, 40), rng.randint(200, 600)
            for j in range(rng.randint(1, 3)):
                for i in range(reps):
                    out.append((t, max(0, t + dq - (reps // 2) * p + i * p), ln))
                t += 4
        elif kind == "jump":
            t += rng.choice([rng.randint(585, 615), rng.randint(585, 615), rng.randint(620, 1200), rng.randint(1200, 4000)])
            out.append((t, max(0, t + dq), rng.randint(1, 30)))
        elif kind == "back":                                   # a node far behind the list's end, then on from where the list was
            out.append((max(0, t - rng.randint(590, 1500)), max(0, t + dq - rng.randint(590, 1500)), rng.randint(1, 20)))
            for _ in range(rng.randint(1, 5)):
                t += rng.choice([0, 4, 8])
                out.append((t, max(0, t + dq), rng.randint(1, 30)))
        elif kind == "ovl" and len(out) > 1:                   # the next node starts ov bases inside the last one's end
            at, aq, al = out[-1]
            if aq < (1 << 31):
                ov = rng.choice([0, 1, 5, 6, 6, 7, 7, 8]); ov2 = rng.randint(0, ov)
                a, b = (ov, ov2) if rng.random() < 0.5 else (ov2, ov)
                nt, nq = at + al + 8 - a, aq + al + 8 - b
                if nq >= 0:
                    t = nt; dq = nq - nt
                    out.append((t, nq, rng.randint(1, 30)))
        elif kind == "indel" and len(out) > 1:                 # the next node lies d diagonals off the last one
            at, aq, al = out[-1]
            if aq < (1 << 31):
                d = rng.choice([7, 8, 9, 15, 16, 199, 200, 200, 201, 201, 202]) * rng.choice([1, -1])
                nt = at + al + 8 + rng.randint(0, 20)
                nq = nt + (aq - at) - d
                if nq >= aq + al + 2:
                    out.append((nt, nq, rng.randint(1, 30)))
                    t = nt
                    if abs(d) < 100:
                        dq = nq - nt
    N = np.zeros((n, 4), np.uint32)
    N[:, :3] = np.array(out[:n], np.int64).astype(np.uint32)
    N[0, 3] = 10000 + rng.randint(0, 3000) if style != "gap" else 10000 + rng.randint(0, 500)
    return N


def mirror_left(rng, N, wrap=False):
    """the list of a right extension turned round: a node's end becomes its start, so the left scan judges what the right scan judged"""
    t, q, l = N[:, 0].astype(np.int64), N[:, 1].astype(np.int64), _s32(N[:, 2].astype(np.int64))
    q = np.where(q >= (1 << 31), 0, q)
    te, qe = t + l + 8, q + l + 8
    T0 = int(te.max()) + rng.randint(12, 5000)
    Q0 = int(qe.max()) + (rng.randint(0, 3000) if not wrap else -rng.randint(1, 24))     # wrap: the last nodes start in front of the read (q < 0)
    M = N.copy()
    M[:, 0] = ((T0 - te) & M32).astype(np.uint32); M[:, 1] = ((Q0 - qe) & M32).astype(np.uint32)
    M[0, 2] = 0                                                # (a[0].len is never read by the left DP)
    return M


SIZES = [1, 2, 8, 9, 16, 17, 64, 65, 66, 128, 129, 256, 257, 300, 1025, 2100]


class DpSet:
    def __init__(self):
        self.lists, self.modes, self.src = [], [], []

    def add(self, mode, N, src):
        self.lists.append(np.ascontiguousarray(N, np.uint32)); self.modes.append(mode); self.src.append(src)

    def finish(self, DPB=8):
        self.expect, self.classes = [], []
        for mode, N in zip(self.modes, self.lists):
            e = oracle_scores(mode, N)
            r, cls = restate(mode, N, DPB)
            assert np.array_equal(r, e), "the numpy restatement of the scan and the oracle disagree"
            self.expect.append(e); self.classes.append(cls)
        return self

    def subset(self, idx):
        s = DpSet()
        for i in idx:
            s.add(self.modes[i], self.lists[i], self.src[i])
        s.expect = [self.expect[i] for i in idx]; s.classes = [self.classes[i] for i in idx]
        return s


def harvest(ext, n_lists):
    """node lists as sdp_right_M2 / sdp_left_M2 built them in the oracle (ora_ext_stage's segments, an ExtSet's cases): the longest ones and the
    ones given up at a merge, with the scores the oracle's extension gave the nodes it scored -> (mode, list, those scores)"""
    segs = []
    for m, e in zip(ext.rows, ext.exp):
        for k, (N, scored) in enumerate(e["segs"]):
            if 2 <= len(N) <= 5000:
                segs.append((k + 1 < len(e["segs"]), len(N), LEFT if m["left"] else RIGHT, N, scored))
    merged = sorted((x for x in segs if x[0]), key=lambda x: -x[1])[:n_lists // 2]
    longest = sorted((x for x in segs if not x[0]), key=lambda x: -x[1])[:n_lists - len(merged)]
    return [(mode, N.copy(), N[:scored, 3].astype(np.int32)) for _, _, mode, N, scored in merged + longest]


def build_dp_set(seed, ext=None, reps=2, extra=44, n_wrap=40, n_harvest=24, DPB=8):
    """the full set: every size of SIZES in every mode and style, `extra` more lists of 300 .. 520 nodes and n_wrap short
    ones with wrapped coordinates per extension mode, three
    tandem-repeat lists of about 5000 nodes, and lists harvested from the oracle's extensions (an ExtSet)"""
    rng = random.Random(seed)
    s = DpSet()
    styles = ["walk", "sparse", "dense", "wrap"]
    for n in SIZES:
        for r in range(reps):
            for mode in (MIDDLE, RIGHT, LEFT):
                st = "gap" if mode == MIDDLE else styles[(r + n) % len(styles)]
                N = gen_right(rng, n, st)
                s.add(mode, N if mode != LEFT else mirror_left(rng, N, st == "wrap"), "%s %d" % (st, n))
    for k in range(extra):
        for mode in (RIGHT, LEFT):
            st = ["dense", "dense", "walk", "dense", "sparse"][k % 5]
            N = gen_right(rng, rng.randint(300, 520), st)
            s.add(mode, N if mode != LEFT else mirror_left(rng, N, st == "wrap"), "%s extra" % st)
    for k in range(n_wrap):
        for mode in (RIGHT, LEFT):
            N = gen_right(rng, rng.randint(20, 120), "wrap")
            s.add(mode, N if mode != LEFT else mirror_left(rng, N, True), "wrap extra")
    for k in range(3):
        N = gen_right(rng, 5000 + rng.randint(-60, 60), "tandem")
        mode = (RIGHT, LEFT, RIGHT)[k]
        s.add(mode, N if mode != LEFT else mirror_left(rng, N), "tandem repeat")
    s.harvest_scores = {}
    if ext is not None:
        for mode, N, sc in harvest(ext, n_harvest):
            s.harvest_scores[len(s.lists)] = sc
            s.add(mode, N, "harvested")
    return s.finish(DPB)


# ---- the extensions on their own (tests/test_stage_ext.py) ---------------------------------------------------------------------------------
EXT = np.dtype([(n, "<u4") for n in ("L", "strand", "left", "mw", "c0", "n_chains", "chain_ID", "a0", "n_anc", "sms_cap", "heavy_limit", "n_ref")] + [("score_ori", "<i4"), ("pad0", "<u4")] +
               [(n, "<u8") for n in ("bin_off", "pk_off", "ref_off", "ref_bases", "node_off", "sc_off", "ri_off")] + [("score", "<i4")] + [(n, "<u4") for n in ("status", "n_sms", "defined")])
CHAIN = np.dtype([("ref_ID", "<u4"), ("q_t_dis", "<i4"), ("sum_score", "<u4"), ("anchor_number", "<u4"), ("direction", "u1"), ("with_top_anchor", "u1"), ("primary", "u1"), ("pri_index", "u1")] +
                 [(n, "<u4") for n in ("t_st", "t_ed", "q_st", "q_ed", "indel", "chain_id")] + [("cur", "<i4")])
EXT_CLASSES = ["reference end:right", "reference end:left", "last_search", "empty window", "first node more than 1000 beyond the best", "stop in mid-block",
               "one merge", "two merges", "node exactly 1000 bases beyond the best, a merge behind it", "window with more than 64 nodes", "more than 64 nodes within 600 bases", "left over the start of reference 0", "q_st < 8"]
EXT_GUARD = 4


def _pack_text(T):
    nb = (len(T) + 3) // 4
    p = np.zeros(nb * 4, np.uint8); p[:len(T)] = T
    q = p.reshape(nb, 4)
    by = (q[:, 0] << 6) | (q[:, 1] << 4) | (q[:, 2] << 2) | q[:, 3]
    return np.concatenate([by.astype(np.uint8), np.zeros(4096 + (-nb) % 8, np.uint8)])


def _subst(rng, S, every):
    """a copy of S with a substitution every `every` bases or so (no indels: the diagonal stays)"""
    S = list(S); i = rng.randint(every // 2, every)
    while i < len(S):
        S[i] = (S[i] + rng.randint(1, 3)) & 3; i += rng.randint(every // 2, every + every // 2)
    return S


def _tandem(rng, n):
    u = [rng.randrange(4) for _ in range(rng.randint(2, 7))]
    return (u * (n // len(u) + 1))[:n]


class ExtSet:
    """cases of one extension each: reads, texts of two references, chain lists with anchors, and the oracle's answers"""

    def __init__(self):
        self.pool = S.ReadPool(); self._ref, self.nref = [], 0
        self.rows, self.chains, self.anchors, self.ris, self.meta = [], [], [], [], []

    def add(self, rng, kind, left):
        rnd = lambda n: [rng.randrange(4) for _ in range(n)]
        d = 0
        r = rng.randrange(2)                                   # the reference the chains lie on: seq_offset 0, or behind reference 0
        A_len = rng.randint(60, 200)
        A = rnd(A_len)
        n_merge = {"merge1": 1, "merge2": 2}.get(kind, 0)
        # `out`: what lies beyond the chain in the direction of the extension, reference and read (nearest base first); others: further chains out there
        others = []
        if kind in ("empty",):
            f = rng.choice([0, 30, 300, 900, 2500]); To, Qo = rnd(rng.randint(0, 3000)), rnd(f)
        elif kind == "last":
            f = rng.randint(20, 590); To = rnd(f + rng.randint(0, 900)); Qo = S.mutate(rng, To[:f], rng.choice([0, 0.03, 0.1]))
        elif kind == "long":
            f = rng.randint(700, 3500); To = rnd(f + rng.randint(0, 900)); Qo = S.mutate(rng, To[:f], rng.choice([0.02, 0.06, 0.12]))
        elif kind == "offdiag":                                # matches 210 .. 400 diagonals off the chain's (the read lacks that many bases behind the chain):
            sh = rng.randint(210, 400); f = rng.randint(900, 1100); To = rnd(sh + f + 900)      # nothing descends from the seed, the best node stays where it is
            Qo = _subst(rng, To[sh:sh + f], 40)
            if rng.random() < 0.55:                            # no match between 1000 and 1200 bases out: the third window's first node is the first beyond 1000
                a = 985 - sh; Qo[a:a + 215] = rnd(215)
        elif kind == "tandem":
            f = rng.randint(500, 1500); rep = _tandem(rng, rng.randint(150, 420)); pre = rnd(rng.randint(0, 300))
            To = pre + rep + rnd(f); Qo = S.mutate(rng, pre, 0.03) + S.mutate(rng, rep, rng.choice([0, 0.01])) + S.mutate(rng, To[len(pre) + len(rep):], 0.05)
        elif kind == "refend":
            v = rng.randrange(3)
            if v == 0:                                         # the chain ends at the end of the reference
                To = rnd(rng.randint(0, 8)); Qo = rnd(rng.choice([0, 100, 900]))
            else:                                              # the last_search window ends within 12 bases of the reference end
                d = rng.randint(100, 539); To = rnd(d + 48 - 3 + rng.randint(0, 11)) if not left else rnd(d + 45 + rng.randint(0, 11) - 0)
                Qo = _subst(rng, To[:d], rng.choice([25, 60]))
        elif kind == "edge":                                   # a short match node exactly 1000 bases beyond the best (or one base off), and right behind it a
            sh = rng.randint(210, 400); bl = rng.randint(28, 60); B = rnd(bl); xl = rng.randint(12, 15)      # chain to merge: ext_block's strict stop test decides whether the loop gets there.
            d = rng.choice([0, 0, 0, -1, 1])                   # (the matches in between lie sh diagonals off the chain's: the best node stays the seed)
            o = 1001 + d + (0 if left else xl)
            T1 = rnd(o); Q1 = _subst(rng, T1[sh:], 40)
            x0 = 1000 + d - (xl if left else 0)                # the short node: xl bases from x0 on, a mismatch on either side
            Q1[x0 - sh:x0 + xl - sh] = T1[x0:x0 + xl]; Q1[x0 - 1 - sh] = (T1[x0 - 1] + 1) & 3; Q1[x0 + xl - sh] = (T1[x0 + xl] + 1) & 3
            others.append((o, bl, sh))
            T2 = rnd(300); To = T1 + B + T2; Qo = Q1 + B + [(T2[0] + 1) & 3] + T2[1:200]
        else:                                                  # merges: further chains on the same diagonal
            To, Qo = [], []
            for k in range(n_merge):
                g = rng.randint(40, 400); T1 = rnd(g); Q1 = _subst(rng, T1, rng.choice([20, 45]))
                Q1[-1] = (T1[-1] + 1) & 3; Q1[0] = (T1[0] + 1) & 3
                bl = rng.randint(28, 60); B = rnd(bl)
                others.append((len(To) + g, bl, 0))
                To += T1 + B; Qo += Q1 + B
            f = rng.randint(0, 700); T2 = rnd(f + 300); To += T2; Qo += [(T2[0] + 1) & 3] + S.mutate(rng, T2[1:f], 0.05) if f > 1 else []
        # what lies on the other side of the chain
        # (a right extension of a chain with q_st < 8 searches from the wrapped q_st - 8 on: it finds nothing, in the reference as here)
        # and so does one whose window would start before the read: min(q_ed + 1000, L) - 2000 is compared as an unsigned number)
        back_q = rng.choice([0, 7, 300, 1500, 1950, 2000, 2300, 2600, 2600, 3000]) if not left else rng.choice([0, 3, 40, 700])
        Tb = rnd(back_q + rng.randint(0, 50)); Qb = S.mutate(rng, Tb[len(Tb) - back_q:], 0.05)[:back_q] if back_q else []
        if not left:
            T = Tb + A + To; Q = Qb + A + Qo
            t_st, q_st = len(Tb), len(Qb)
        else:
            T = To[::-1] + A + Tb[::-1]; Q = Qo[::-1] + A + Qb[::-1]
            t_st, q_st = len(To), len(Qo)
        while len(Q) < 200:
            Q.append(rng.randrange(4))
        t_ed, q_ed = t_st + A_len, q_st + A_len
        other_T = rnd(rng.randint(300, 2000))
        texts = [T, other_T] if r == 0 else [other_T, T]
        ris = [(len(texts[0]), 0), (len(texts[1]), len(texts[0]))]
        blk = _pack_text(np.array(texts[0] + texts[1], np.uint8))
        ref_off = self.nref; self._ref.append(blk); self.nref += len(blk)
        strand = rng.choice([S.FORWARD, S.REVERSE])
        seq = bytes(b"ACGT"[b] for b in Q) if strand == S.FORWARD else bytes(b"ACGT"[3 - b] for b in reversed(Q))
        rd = self.pool.add(seq)
        c0, a0 = len(self.chains), len(self.anchors)
        ch = [(r, 0, rng.randint(20, 200), 1, strand, 0, 0, 0, t_st, t_ed, q_st, q_ed, 0, 0, -1)]
        na = 0
        for (o, bl, sh) in others:
            bt, bq = (t_ed + o, q_ed + o - sh) if not left else (t_st - o - bl, q_st - (o - sh) - bl)
            m1 = rng.randint(13, bl // 2)
            self.anchors.append((bq, bt, m1, -1, r)); self.anchors.append((bq + bl - 13, bt + bl - 13, 13, na, r)); na += 2
            ch.append((r, 0, rng.randint(10, 60), 2, strand, 0, 0, 0, bt, bt + bl, bq, bq + bl, 0, 0, na - 1))
        if rng.random() < 0.3:                                 # a chain that must not merge: other reference, same diagonal
            ch.append((1 - r, 0, 30, 1, strand, 0, 0, 0, t_ed + 100, t_ed + 130, q_ed + 100, q_ed + 130, 0, 0, -1))
        self.chains += ch
        self.ris += ris
        self.rows.append(dict(read=rd, strand=strand, left=int(left), c0=c0, n_chains=len(ch), a0=a0, n_anc=na, ref_off=ref_off, ref_bases=len(T) + len(other_T),
                              ri_off=len(self.ris) - 2, score_ori=rng.randint(20, 400), kind=kind,
                              edge=d if kind == "edge" else 0))

    def finish(self, ora):
        L = oracle_lib.lib()
        vp = C.c_void_p
        L.ora_ext_stage.argtypes = [vp, C.c_char_p, C.c_uint32, C.c_int, C.c_int, vp, C.c_uint64, vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, C.c_int, C.c_int, vp, vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32]
        self.bin, self.pk = self.pool.blobs()
        self.ref = np.concatenate(self._ref)
        self.chain_arr = np.array(self.chains, dtype=CHAIN)
        self.anc_arr = np.array(self.anchors + [(0, 0, 0, -1, 0)], np.int32).reshape(-1, 5)
        self.ri_arr = np.array(self.ris, np.uint64).reshape(-1, 2)
        self.exp = []
        info = np.zeros(4, np.uint32); win = np.zeros(256, np.uint32); seg = np.zeros(64, np.uint32); nodes = np.zeros((1 << 16, 4), np.uint32)
        for m in self.rows:
            ch = self.chain_arr[m["c0"]:m["c0"] + m["n_chains"]].copy()
            an = np.ascontiguousarray(self.anc_arr[m["a0"]:m["a0"] + max(1, m["n_anc"])])
            ri = np.ascontiguousarray(self.ri_arr[m["ri_off"]:m["ri_off"] + 2])
            seq = self.pool.seqs[m["read"]]
            sc = L.ora_ext_stage(ora.ctx, seq, len(seq), m["strand"], m["left"], vp(self.ref.ctypes.data + m["ref_off"]), m["ref_bases"], _ptr(ri), 2, _ptr(ch), len(ch), _ptr(an), m["n_anc"],
                                 0, m["score_ori"], _ptr(info), _ptr(win), len(win), _ptr(seg), len(seg) // 2, _ptr(nodes), len(nodes))
            n_win, n_seg = int(info[2]), int(info[3])
            assert n_win <= len(win) and n_seg <= len(seg) // 2
            segs, o = [], 0
            for k in range(n_seg):
                n, scored = int(seg[2 * k]), int(seg[2 * k + 1])
                segs.append((nodes[o:o + n].copy(), scored)); o += n
            self.exp.append(dict(score=sc, chains=ch, reason=int(info[0]), merges=int(info[1]), win=win[:n_win].copy(), segs=segs))
        return self

    def classes(self, i):
        m, e = self.rows[i], self.exp[i]
        cls = set()
        side = "left" if m["left"] else "right"
        if e["reason"] == 1:
            cls.add("reference end:" + side)
        if e["reason"] == 2:
            cls.add("last_search")
        if e["reason"] == 3:
            cls.add("empty window")
        if e["reason"] == 4:
            cls.add("first node more than 1000 beyond the best")
        last, scored = e["segs"][-1]
        if e["reason"] == 5 and scored < len(last):
            starts = [0] + [int(w) for w in e["win"]]
            b0 = max(w for w in [1] + starts if w <= scored - 1)
            if (scored - 1 - b0) % 64 != 63 and scored < len(last):
                cls.add("stop in mid-block")
        if m["kind"] == "edge" and e["merges"] == 1 and m["edge"] == 0:
            cls.add("node exactly 1000 bases beyond the best, a merge behind it")
        if e["merges"] == 1:
            cls.add("one merge")
        if e["merges"] >= 2:
            cls.add("two merges")
        w = np.concatenate([[1], e["win"]]).astype(np.int64)
        if len(w) > 1 and (np.diff(w) > 64).any():
            cls.add("window with more than 64 nodes")
        for N, sc in e["segs"]:
            t = np.sort(N[1:sc, 0].astype(np.int64))
            if len(t) > 65 and (t[65:] - t[:-65] <= 600).any():
                cls.add("more than 64 nodes within 600 bases")
        ch0 = self.chain_arr[m["c0"]]
        if m["left"] and int(ch0["ref_ID"]) == 0 and len(e["win"]) and int(ch0["t_st"]) + 3 < 50 + min(600, int(ch0["q_st"]) + 60 if int(ch0["q_st"]) < 600 else int(ch0["t_st"]) + 3):
            cls.add("left over the start of reference 0")
        if not m["left"] and int(ch0["q_st"]) < 8 and len(e["win"]):
            cls.add("q_st < 8")
        return cls


EXT_KINDS = {"empty": 40, "last": 40, "long": 40, "offdiag": 230, "tandem": 90, "refend": 360, "merge1": 90, "merge2": 90, "edge": 120}


def build_ext_set(seed, ora, scale=1.0):
    rng = random.Random(seed)
    s = ExtSet()
    for kind, n in EXT_KINDS.items():
        for k in range(max(2, int(n * scale))):
            s.add(rng, kind, left=bool(k & 1))
    return s.finish(ora)


class ExtLeg:
    def __init__(self, path, prefix):
        self.lib = C.CDLL(path)
        out = (C.c_uint32 * 4)()
        getattr(self.lib, "emu_stage_sizes_ext" if prefix == "emu_stage" else "stage_dev_sizes_ext")(out)
        assert [int(x) for x in out] == [EXT.itemsize, CHAIN.itemsize, 4, 16], list(out)
        self._ext = getattr(self.lib, prefix + "_ext")
        vp, sz = C.c_void_p, C.c_size_t
        self._ext.argtypes = [vp, C.c_uint32, vp, sz, vp, sz, vp, sz, vp, sz, vp, sz, vp, sz, vp, sz, vp, sz]
        self.findings = DpLeg.findings.__get__(self)

    def run(self, s, mw, idx=None, heavy=0):
        idx = list(range(len(s.rows))) if idx is None else list(idx)
        cs = np.zeros(len(idx), EXT)
        chains, sc_off, c_off, n_off = [], 0, 0, 0
        for k, i in enumerate(idx):
            m = s.rows[i]
            cap = max(64, max(len(N) for N, _ in s.exp[i]["segs"]) + 8)          # (the oracle's longest list and a few more; the guards lie behind)
            cs[k] = (len(s.pool.seqs[m["read"]]), m["strand"], m["left"], mw, c_off, m["n_chains"], 0, m["a0"], m["n_anc"], cap, heavy, 2, m["score_ori"], 0,
                     s.pool.bin_off[m["read"]], s.pool.pk_off[m["read"]], m["ref_off"], m["ref_bases"], n_off, sc_off, m["ri_off"], 0, 0, 0, 0)
            chains.append(s.chain_arr[m["c0"]:m["c0"] + m["n_chains"]]); c_off += m["n_chains"]; sc_off += 256 + 2 * m["n_chains"] + 8; n_off += cap + EXT_GUARD
        ch = np.concatenate(chains).copy()
        nodes = np.full((n_off, 4), PATTERN, np.uint32)
        scs = np.full(sc_off * 2, 0xCDCD, np.uint16)
        ri = np.ascontiguousarray(s.ri_arr)
        rc = self._ext(_ptr(cs), len(cs), _ptr(s.bin), s.bin.nbytes, _ptr(s.pk), len(s.pk), _ptr(s.ref), s.ref.nbytes, _ptr(ch), len(ch), _ptr(s.anc_arr), len(s.anc_arr),
                       _ptr(nodes), len(nodes), _ptr(scs), sc_off, _ptr(ri), len(ri))
        assert rc == 0, "stage library call failed at line %d" % rc
        return cs, ch, nodes


def ext_emu1():
    return ExtLeg(S.EMU1, "emu_stage")


def ext_emu64():
    return ExtLeg(S.EMU64, "emu_stage")


def ext_device():
    return ExtLeg(S.STAGE_SO, "stage_dev")
