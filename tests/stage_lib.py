"""Stage a-12 (sparse match and gap scoring) on its own: ctypes bindings of the three legs and the case generators of
tests/test_stage_sdp.py.  TEST ONLY; pure Python + numpy, seeded and deterministic.

The legs take the same flat arrays (tests/stage/dsb_stage_forms.h describes them): byte strands and packed strands of the reads,
reference windows as bytes, one node region per case; the oracle (oracle/classify.c: ora_sdp_match_stage, ora_gap_stage) gives the
expected node lists and scores from the ASCII reads."""
import ctypes as C
import os
import random

import numpy as np

import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU1 = os.path.join(ROOT, "tests", "emu", "libdsbemu.so")
EMU64 = os.path.join(ROOT, "tests", "emu", "libdsbemu64.so")
STAGE_SO = os.path.join(ROOT, "tests", "stage", "libdsbstage.so")

QPAD_L, QPAD_R, QPAD_R_VAL, TPAD_VAL = 64, 192, 5, 4            # oracle/classify.c, dsb_device.h
WIN_FRONT, WIN_TAIL = 64, 128                                    # bytes around a window in the window blob (DSB_REFWIN_FRONT; pads)
FORWARD, REVERSE = 1, 0
MIDDLE, RIGHT, LEFT = 0, 1, 2
FORMS = {"wtab": 0, "wtab_pk": 1, "inv": 2, "n": 3, "n_pk": 4, "lds": 5, "lds_pk": 6}
ST_SMS_OVF = 4
INV_NONE = 0xFFFFFFFF
GL_NONE = -2147483648
SMS_CAP = 16384                                                  # DSB_SMS_CAP: the smallest node arena a launch has
GUARD = 4                                                        # guard entries behind a case's node region
PATTERN = 0xCDCDCDCD

SDP = np.dtype([(n, "<u4") for n in ("L", "strand", "q_bg", "q_ed", "t_len", "t_st", "fwd", "sms_cap", "kind", "pad0")] +
               [(n, "<u8") for n in ("bin_off", "pk_off", "win_off", "node_off")] + [(n, "<u4") for n in ("rv", "status", "defined", "pad1")])
CHAIN = np.dtype([(n, "<u4") for n in ("L", "strand", "g0", "g1", "a0", "n_anc")] + [("c_a", "<i4"), ("use_pk", "<u4")] +
                 [(n, "<u8") for n in ("bin_off", "pk_off", "ref_off", "ref_bases")] + [("score", "<i4"), ("status", "<u4"), ("pad0", "<u4"), ("pad1", "<u4")])
GAP = np.dtype([(n, "<u4") for n in ("pq", "pt", "pl", "cq", "ct", "cl")] + [("gain", "<i4"), ("pad", "<u4")])

_LUT = np.ones(256, np.uint8)
for _c, _v in ((b"Aa", 0), (b"Gg", 2), (b"Tt", 3)):
    for _b in _c:
        _LUT[_b] = _v


class Consts:
    def __init__(self, v):
        (self.sz_sdp, self.sz_chain, self.sz_gap, self.WTAB_SLOTS, self.WTAB_MAXQ, self.INV_PAIRS, self.INV_MINQ, self.INV_MAXPOS,
         self.SDP_CAND, self.SDP_KEEP, self.GL_QW, self.GL_NODES, self.GL_MAXT, self.INV_WORDS, self.lanes, self.MAX_ANC) = [int(x) for x in v]


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


class Leg:
    """one of the three legs: the 1-lane emulation, the 64-lane emulation with the race detector, the device"""

    def __init__(self, path, prefix):
        self.lib = C.CDLL(path)
        self.prefix = prefix
        out = (C.c_uint32 * 16)()
        getattr(self.lib, "emu_stage_sizes" if prefix == "emu_stage" else "stage_dev_sizes")(out)
        self.k = Consts(out)
        assert (self.k.sz_sdp, self.k.sz_chain, self.k.sz_gap) == (SDP.itemsize, CHAIN.itemsize, GAP.itemsize)
        sz, vp = C.c_size_t, C.c_void_p
        self._sdp = getattr(self.lib, prefix + "_sdp"); self._sdp.argtypes = [C.c_int, vp, C.c_uint32, vp, sz, vp, sz, vp, sz, vp, sz, vp]
        self._gl = getattr(self.lib, prefix + "_gap_lane"); self._gl.argtypes = [vp, C.c_uint32, vp, sz, vp, sz, vp, sz, vp, sz]
        self._mid = getattr(self.lib, prefix + "_middle"); self._mid.argtypes = [vp, C.c_uint32, vp, sz, vp, sz, vp, sz, vp, sz]

    def sdp(self, form, s, cases=None):
        """run one form over the cases of an SdpSet -> (cases with rv/status/defined, node blob as (n, 4) u32, mirrors as (n, 64, 4) u32)"""
        cs = (s.cases if cases is None else cases).copy()
        nodes = np.full((s.node_entries, 4), PATTERN, np.uint32)
        mirror = np.full((len(cs), 64, 4), PATTERN, np.uint32)
        rc = self._sdp(FORMS[form], _ptr(cs), len(cs), _ptr(s.bin), s.bin.nbytes, _ptr(s.pk), len(s.pk), _ptr(s.win), s.win.nbytes, _ptr(nodes), len(nodes), _ptr(mirror))
        assert rc == 0, "stage library call failed at line %d" % rc
        return cs, nodes, mirror

    def gap_lane(self, g):
        cs = g.lane_cases.copy(); G = g.gaps.copy()
        rc = self._gl(_ptr(cs), len(cs), _ptr(g.bin), g.bin.nbytes, _ptr(g.pk), len(g.pk), _ptr(g.ref), g.ref.nbytes, _ptr(G), len(G))
        assert rc == 0, "stage library call failed at line %d" % rc
        return cs, G

    def middle(self, g, use_pk):
        cs = g.chain_cases.copy(); cs["use_pk"] = 1 if use_pk else 0
        rc = self._mid(_ptr(cs), len(cs), _ptr(g.bin), g.bin.nbytes, _ptr(g.pk), len(g.pk), _ptr(g.ref), g.ref.nbytes, _ptr(g.anchors), len(g.anchors))
        assert rc == 0, "stage library call failed at line %d" % rc
        return cs

    def findings(self):
        if not hasattr(self.lib, "dsb_emu_findings"):
            return []
        self.lib.dsb_emu_findings.argtypes = [C.c_char_p, C.c_size_t]
        buf = C.create_string_buffer(1 << 16)
        self.lib.dsb_emu_findings(buf, len(buf))
        return [l for l in buf.value.decode().split("\n") if l]


def emu1():
    return Leg(EMU1, "emu_stage")


def emu64():
    return Leg(EMU64, "emu_stage")


def device():
    return Leg(STAGE_SO, "stage_dev")


class Oracle:
    def __init__(self):
        L = oracle_lib.lib()
        L.ora_sdp_match_stage.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_int]
        L.ora_gap_stage.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p]
        self.L = L
        self.ctx = L.ora_ctx_new()
        self.buf = np.zeros((1 << 17, 3), np.uint32)

    def close(self):
        self.L.ora_ctx_free(self.ctx)

    def sdp(self, seq, strand, q_bg, q_ed, win, win_off, t_len, t_st, fwd):
        n = self.L.ora_sdp_match_stage(self.ctx, seq, len(seq), strand, q_bg, q_ed, C.c_void_p(win.ctypes.data + win_off), t_len, t_st, fwd, _ptr(self.buf), len(self.buf))
        return self.buf[:min(n, len(self.buf))].copy()          # (a list longer than the buffer is longer than any node arena: only its head is compared)

    def chain(self, seq, strand, ref, ref_bases, anchors, c_a):
        """-> (score, match nodes per gap from the last anchor backwards)"""
        gn = np.zeros(len(anchors) + 1, np.uint32); ng = C.c_uint32()
        a = np.ascontiguousarray(anchors, np.int32)
        sc = self.L.ora_gap_stage(self.ctx, seq, len(seq), strand, _ptr(ref), ref_bases, _ptr(a), len(a), c_a, _ptr(gn), C.byref(ng))
        return sc, gn[:ng.value].copy()


# ---- reads ------------------------------------------------------------------------------------------------------------------
def strands(seq):
    F = _LUT[np.frombuffer(seq, np.uint8)]
    return F, (3 - F)[::-1].copy()


def pack(S):
    """32 bases per word, first base in the top bits, (L + 31) / 32 + 1 words (k_encode_pack)"""
    nw = (len(S) + 31) // 32 + 1
    p = np.zeros(nw * 32, np.uint64); p[:len(S)] = S
    sh = (62 - 2 * np.arange(32)).astype(np.uint64)
    return np.bitwise_or.reduce(p.reshape(nw, 32) << sh, axis=1)


def kmers9(S):
    """the 9-mer at every position of a byte string of bases (positions 0 .. len - 9)"""
    if len(S) < 9:
        return np.zeros(0, np.int64)
    k = np.zeros(len(S) - 8, np.int64)
    for j in range(9):
        k |= S[j:len(S) - 8 + j].astype(np.int64) << (16 - 2 * j)
    return k


class ReadPool:
    """the reads of a set: ASCII, both byte strands with their pads, both packed strands"""

    def __init__(self):
        self.seqs, self.F, self.R, self.bin_off, self.pk_off, self._bin, self._pk, self._kc = [], [], [], [], [], [], [], {}
        self.nb = self.nw = 0

    def add(self, seq):
        F, R = strands(seq)
        blk = np.concatenate([np.zeros(QPAD_L, np.uint8), F, R, np.full(QPAD_R, QPAD_R_VAL, np.uint8)])
        pk = np.concatenate([pack(F), pack(R)])
        self.seqs.append(seq); self.F.append(F); self.R.append(R); self.bin_off.append(self.nb); self.pk_off.append(self.nw)
        self._bin.append(blk); self._pk.append(pk); self.nb += len(blk); self.nw += len(pk)
        return len(self.seqs) - 1

    def strand(self, r, strand):
        return self.F[r] if strand == FORWARD else self.R[r]

    def kmers(self, r, strand):
        if (r, strand) not in self._kc:
            self._kc[(r, strand)] = kmers9(self.strand(r, strand))
        return self._kc[(r, strand)]

    def blobs(self):
        return np.concatenate(self._bin), np.concatenate(self._pk + [np.zeros(2, np.uint64)])


def random_read(rng, L):
    """200 .. 8000 bases: random sequence with homopolymer and tandem-repeat stretches and some non-ACGT bytes"""
    out = bytearray()
    while len(out) < L:
        r = rng.random()
        if r < 0.55:
            out += bytes(rng.choice(b"ACGT") for _ in range(rng.randint(30, 400)))
        elif r < 0.7:
            out += bytes([rng.choice(b"ACGT")]) * rng.randint(12, 700)
        else:
            unit = bytes(rng.choice(b"ACGT") for _ in range(rng.randint(2, 9)))
            out += unit * (rng.randint(20, 700) // len(unit) + 1)
    out = out[:L]
    for _ in range(rng.randint(0, max(1, L // 150))):
        out[rng.randrange(L)] = rng.choice(b"NnacgtRY")
    return bytes(out)


def mutate(rng, S, rate):
    """a copy of the bases S with substitutions, insertions and deletions at the given rate"""
    if rate <= 0:
        return list(S)
    out = []
    for b in S:
        r = rng.random()
        if r < rate * 0.5:
            out.append(rng.randrange(4))
        elif r < rate * 0.75:
            continue
        elif r < rate:
            out += [int(b), rng.randrange(4)]
        else:
            out.append(int(b))
    return out


# ---- sdp_match cases ----------------------------------------------------------------------------------------------------------
class SdpSet:
    """cases of sdp_match with the oracle's node lists and what the coverage conditions need (all from the inputs and the oracle)"""

    def __init__(self, k):
        self.k = k
        self.pool = ReadPool()
        self.rows, self._win, self.nwin = [], [], 0
        self.meta = []                         # per case: dict(read, tk, n_q, pairs, maxocc, padbits, stage)

    def add(self, r, strand, kind, q_bg, q_ed, body, front, tail, t_st):
        """body: the t_len window bytes; front: bytes in front of it (<= WIN_FRONT, real ones last); tail: bytes the caller has behind t_len"""
        fr = np.zeros(WIN_FRONT, np.uint8)
        if len(front):
            fr[WIN_FRONT - len(front):] = front
        tl = np.full(WIN_TAIL, TPAD_VAL, np.uint8); tl[:len(tail)] = tail
        w = np.concatenate([fr, np.asarray(body, np.uint8), tl])
        L = len(self.pool.seqs[r])
        self.rows.append((L, strand, q_bg & 0xFFFFFFFF, q_ed, len(body), t_st, 1 if kind != LEFT else 0, 0, kind, 0, self.pool.bin_off[r], self.pool.pk_off[r], self.nwin + WIN_FRONT, 0, 0, 0, 0, 0))
        self.meta.append({"read": r})
        self._win.append(w); self.nwin += len(w)

    def finish(self, ora, ovf_every=0):
        """run the oracle, size the node regions (sms_cap = the oracle's count + 8; every ovf_every-th case with nodes gets a cap below its count)"""
        k = self.k
        self.cases = np.array(self.rows, dtype=SDP)
        self.win = np.concatenate(self._win)
        self.bin, self.pk = self.pool.blobs()
        self.expect = []
        off = 0
        for i, c in enumerate(self.cases):
            m = self.meta[i]; r = m["read"]; L = int(c["L"]); strand = int(c["strand"]); fwd = int(c["fwd"]); t_len = int(c["t_len"])
            e = ora.sdp(self.pool.seqs[r], strand, int(c["q_bg"]), int(c["q_ed"]), self.win, int(c["win_off"]), t_len, int(c["t_st"]), fwd)
            self.expect.append(e)
            cap = len(e) + 8
            m["ovf"] = bool(ovf_every and len(e) >= 2 and i % ovf_every == 0) or cap > SMS_CAP
            if m["ovf"]:                       # a node arena smaller than the list: half of it, or the arena of a batch of short reads (DSB_SMS_CAP)
                cap = min(max(1, len(e) // 2), SMS_CAP)
            c["sms_cap"] = cap; c["node_off"] = off; off += cap + GUARD
            # what the predicates need, from the inputs alone
            q_bg, q_ed = int(c["q_bg"]), int(c["q_ed"])
            hi = min(q_ed, L - 9)
            n_q = hi - q_bg + 1 if (L >= 9 and q_bg <= hi) else 0
            tk = (t_len - 9 + 1) & 0xFFFFFFFF
            m["n_q"], m["tk"] = n_q, tk
            pairs = maxocc = 0; padbits = False; per_pos = {}
            if n_q > 0 and 4 < tk <= 0x7FFFFFFF:
                t = self.win[int(c["win_off"]):int(c["win_off"]) + t_len + 1].astype(np.int64)
                kt = kmers9(t[:t_len])                                   # (OR of the shifted bytes: what the rolling 9-mer holds)
                ii = np.arange(4, tk, 4)
                if fwd:
                    pk_ = kt[ii] & 0x3FFFF
                else:
                    ct = t_len - 13 - (ii - 4)
                    pk_ = kt[ct] | np.where(ii > 4, t[ct + 9] >> 2, 0)
                    padbits = bool(np.any(t[:t_len] >= 4))
                u, cnt = np.unique(self.pool.kmers(r, strand)[q_bg:hi + 1], return_counts=True)
                pos = np.searchsorted(u, pk_); pos[pos >= len(u)] = 0
                occ = np.where(u[pos] == pk_, cnt[pos], 0)
                pairs, maxocc = int(occ.sum()), int(occ.max()) if len(occ) else 0
            m["pairs"], m["maxocc"], m["padbits"] = pairs, maxocc, padbits
            # nodes per probed position, from the oracle's list (see the module docstring of test_stage_sdp.py)
            if len(e):
                rel = e[:, 0].astype(np.int64) - int(c["t_st"])
                x = rel if fwd else t_len - 8 - rel - e[:, 2].astype(np.int64)
                pi = np.maximum(4, (x + 3) // 4 * 4)
                m["maxnodes"] = int(np.unique(pi, return_counts=True)[1].max())
            else:
                m["maxnodes"] = 0
            # the staging condition of sdp_middle_M2 (dsb_classify_dev.h, "Small gap"), without and with packed words
            slots = min(max(2 * n_q, 64), k.WTAB_SLOTS)
            q_lo, q_hi = q_bg - 16, q_ed + max(80, t_len + 4)
            q_bytes = ((q_hi - q_lo + 7) & ~7) if q_hi > q_lo else 0
            t_bytes = (t_len + 64 + 7) & ~7
            m["stage"] = []
            for tb in (slots, max(slots, (k.INV_WORDS + 3) & ~3)):
                m["stage"].append(bool(fwd and int(c["kind"]) == MIDDLE and 0 < n_q <= k.WTAB_MAXQ and q_bytes and q_lo >= -QPAD_L + 8 and
                                       4 * tb + q_bytes + 8 + t_bytes + 8 + 1024 <= 4 * k.WTAB_SLOTS))
        self.node_entries = off
        # the expected node blob of a form that is defined for every case
        self.full = np.full((off, 4), PATTERN, np.uint32)
        for c, e, m in zip(self.cases, self.expect, self.meta):
            if not m["ovf"]:
                o = int(c["node_off"]); self.full[o:o + len(e), :3] = e
        self.case_of = np.repeat(np.arange(len(self.cases)), self.cases["sms_cap"].astype(np.int64) + GUARD)
        return self

    def subset(self, idx):
        """the cases idx as a set of their own (same reads and windows, node regions packed anew)"""
        s = SdpSet.__new__(SdpSet); s.k = self.k; s.pool = self.pool; s.bin, s.pk, s.win = self.bin, self.pk, self.win
        s.cases = self.cases[idx].copy(); s.expect = [self.expect[i] for i in idx]; s.meta = [self.meta[i] for i in idx]
        caps = s.cases["sms_cap"].astype(np.int64) + GUARD
        s.cases["node_off"] = np.concatenate([[0], np.cumsum(caps)[:-1]]); s.node_entries = int(caps.sum())
        s.full = np.full((s.node_entries, 4), PATTERN, np.uint32)
        for c, e, m in zip(s.cases, s.expect, s.meta):
            if not m["ovf"]:
                o = int(c["node_off"]); s.full[o:o + len(e), :3] = e
        s.case_of = np.repeat(np.arange(len(s.cases)), caps)
        return s


def _window_content(rng, S, a, n, style):
    """n bases that look like read positions a .. : the read's own bases mutated, or something that drives a branch"""
    seg = S[max(0, a):max(0, a) + n + 80]
    if style == "unrelated" or len(seg) < 9:
        return [rng.randrange(4) for _ in range(n)]
    rate = rng.choice([0.0, 0.0, 0.02, 0.05, 0.1, 0.15, 0.25])
    out = mutate(rng, seg, rate)
    while len(out) < n:
        out.append(rng.randrange(4))
    return out[:n]


def _plant(rng, seq, where, n_copies, span):
    """the same 14 bases at n_copies places of seq[where : where + span], each behind a base of its own"""
    motif = bytes(rng.choice(b"ACGT") for _ in range(14))
    s = bytearray(seq)
    for _ in range(n_copies):
        p = where + rng.randrange(max(1, span - 15))
        if p + 15 < len(s):
            s[p:p + 15] = bytes([rng.choice(b"ACGT")]) + motif
    return bytes(s), motif


def _repeat_stretch(rng, L):
    """a read that is mostly one homopolymer or tandem repeat (period 2 .. 9)"""
    unit = bytes(rng.choice(b"ACGT") for _ in range(rng.choice([1, 1, 2, 3, 4, 5, 6, 7, 8, 9])))
    if len(set(unit)) == 1:
        unit = unit[:1]
    body = unit * (L // len(unit) + 1)
    head = rng.randint(0, 40)
    return (bytes(rng.choice(b"ACGT") for _ in range(head)) + body)[:L], len(unit)


def build_sdp_set(k, ora, seed, n_reads, per_read, ovf_every=40):
    """per read: per_read cases of every kind and content.  Domain: see the module docstring of tests/test_stage_sdp.py."""
    rng = random.Random(seed)
    s = SdpSet(k)
    for ri in range(n_reads):
        style_r = rng.random()
        L = rng.choice([200, 230, 400, 1000, 2500, 5000, 8000]) if ri % 3 == 0 else rng.randint(200, 8000)
        if style_r < 0.25:
            seq, _ = _repeat_stretch(rng, L)
        else:
            seq = random_read(rng, L)
        motif = None
        if 0.25 <= style_r < 0.45:
            seq, motif = _plant(rng, seq, rng.randrange(max(1, L - 300)), rng.choice([5, 8, 40, 90]), min(L, rng.choice([300, 1500])))
        r = s.pool.add(seq)
        for ci in range(per_read):
            kind = (MIDDLE, RIGHT, LEFT)[ci % 3]
            strand = rng.choice([FORWARD, REVERSE])
            S = s.pool.strand(r, strand)
            style = rng.choice(["read", "read", "read", "unrelated", "edge"])
            if kind == RIGHT:
                # sdp_right_M2: window [max(q_ed - 2000, q_st - 8), q_ed], q_ed <= L; t_len = min(600, ...) >= 12; 50 more bases loaded behind it
                t_len = rng.choice([12, 12, 60, 148, 600, 600]) if rng.random() < 0.5 else rng.randint(12, 600)
                q_ed = L if (style == "edge" or rng.random() < 0.2) else rng.randint(0, L)
                q_st8 = rng.randint(-8, -1) if rng.random() < 0.12 else rng.randint(0, max(0, q_ed))
                if rng.random() < 0.15:
                    q_st8 = max(q_st8, q_ed - rng.randint(1, 95))
                q_bg = max(q_ed - 2000, q_st8)
                a = max(0, q_bg) + rng.randint(0, max(0, min(q_ed, L) - max(0, q_bg)))
                body = _window_content(rng, S, a, t_len + 50, style)
                if motif and rng.random() < 0.5 and t_len > 40:
                    p = 4 * rng.randint(1, (t_len - 20) // 4); body[p - 1:p + 14] = [rng.randrange(4)] + [int(x) for x in _LUT[np.frombuffer(motif, np.uint8)]]
                    body = body[:t_len + 50]
                s.add(r, strand, RIGHT, q_bg, q_ed, body[:t_len], [], body[t_len:t_len + 50], rng.randint(0, 1 << 20))
            elif kind == LEFT:
                # sdp_left_M2: t_str = ref + 50, window [q_bg, min(q_bg + 2000, q_st - 1)], q_bg >= 0; t_len = min(600, ...) >= 12
                t_len = rng.choice([12, 12, 60, 148, 600, 600]) if rng.random() < 0.5 else rng.randint(12, 600)
                q_st = L - rng.randint(0, 7) if (style == "edge" or rng.random() < 0.15) else rng.randint(1, L)
                q_bg = max(0, q_st - rng.choice([1000, 1000, rng.randint(1, 95), rng.randint(1, 2000)]))
                q_ed = min(q_bg + 2000, q_st - 1)
                a = rng.randint(q_bg, max(q_bg, min(q_ed, L - 1))) - t_len
                full = _window_content(rng, S, a - 50, t_len + 50, style)
                front, body = full[:50], full[50:]
                pr = rng.random()
                if pr < 0.12:
                    # the window fetched at the very start of the text: t_len bases loaded at ref, t_str = ref + 50 -- the rest is unloaded (4);
                    # the buffer is filled once per extension and loaded piecewise, so the first unloaded byte lies anywhere from t_len - 50 on
                    p0 = max(0, t_len - 50) if pr < 0.06 else max(0, t_len - 4 * rng.randint(2, 12))
                    body = body[:p0] + [TPAD_VAL] * (t_len - p0)
                s.add(r, strand, LEFT, q_bg, q_ed, body, front, [], rng.randint(600, 1 << 20))
            else:
                # sdp_middle_M2: the gap between two anchors, 13 <= t_len < 2000, window [pq + pl - 8, cq - 1]
                big = rng.random()
                g = rng.randint(7, 60) if big < 0.45 else rng.randint(60, 400) if big < 0.75 else rng.randint(1200, 1990) if big < 0.9 else rng.randint(400, 1200)
                t_len = min(1999, g + 6)
                q_bg = L - rng.randint(1, 60) if style == "edge" else rng.randint(5, max(5, L - 10))
                dq = int(t_len * rng.uniform(0.8, 1.2)) + rng.randint(-6, 6)
                q_ed = max(0, min(L - 1, q_bg + max(0, min(1990, dq)) - 1))
                body = _window_content(rng, S, q_bg + 5, t_len, style)
                s.add(r, strand, MIDDLE, q_bg, q_ed, body, [], [], rng.randint(0, 1 << 20))
    return s.finish(ora, ovf_every)


# ---- gaps and chains ----------------------------------------------------------------------------------------------------------
class GapSet:
    """chains of anchors over synthetic reference texts: single gaps for gap_lane (two-anchor chains), whole chains for sdp_middle_M2"""

    def __init__(self, k):
        self.k = k; self.pool = ReadPool(); self._ref, self.nref = [], 0
        self.lane_rows, self.chain_rows, self._gaps, self._anc = [], [], [], []
        self.gap_meta, self.chain_meta = [], []

    def add_text(self, T):
        """2-bit text, 4 bases per byte first base in the top bits, 4 KiB of zeros behind it"""
        nb = (len(T) + 3) // 4
        p = np.zeros(nb * 4, np.uint8); p[:len(T)] = T
        q = p.reshape(nb, 4)
        by = (q[:, 0] << 6) | (q[:, 1] << 4) | (q[:, 2] << 2) | q[:, 3]
        blk = np.concatenate([by.astype(np.uint8), np.zeros(4096 + (-nb) % 8, np.uint8)])
        off = self.nref; self._ref.append(blk); self.nref += len(blk)
        return off, nb * 4

    def add_chain(self, r, strand, ref_off, ref_bases, anchors):
        """anchors: (index_in_read, ref_offset, mtch_len) in read order; chained last to first"""
        a0 = len(self._anc)
        for i, (q, t, l) in enumerate(anchors):
            self._anc.append((q, t, l, i - 1))
        L = len(self.pool.seqs[r])
        self.chain_rows.append((L, strand, 0, 0, a0, len(anchors), len(anchors) - 1, 1, self.pool.bin_off[r], self.pool.pk_off[r], ref_off, ref_bases, 0, 0, 0, 0))
        self.chain_meta.append({"read": r, "ref_off": ref_off})
        g0 = len(self._gaps)
        for i in range(len(anchors) - 1, 0, -1):
            (pq, pt, pl), (cq, ct, cl) = anchors[i - 1], anchors[i]
            self._gaps.append((pq, pt, pl, cq, ct, cl, GL_NONE, 0))
            self.gap_meta.append({"read": r, "strand": strand, "ref_off": ref_off, "ref_bases": ref_bases})
        # the gaps of this chain, 64 per gap_lane case (one per lane)
        for b in range(g0, len(self._gaps), 64):
            self.lane_rows.append((L, strand, b, min(b + 64, len(self._gaps)), 0, 0, 0, 1, self.pool.bin_off[r], self.pool.pk_off[r], ref_off, ref_bases, 0, 0, 0, 0))

    def finish(self, ora):
        k = self.k
        self.bin, self.pk = self.pool.blobs()
        self.ref = np.concatenate(self._ref)
        self.gaps = np.array(self._gaps, dtype=GAP); self.anchors = np.array(self._anc, np.int32).reshape(-1, 4)
        self.lane_cases = np.array(self.lane_rows, dtype=CHAIN); self.chain_cases = np.array(self.chain_rows, dtype=CHAIN)
        # the oracle: the score of every chain with its per-gap node counts; the gain of every gap = the score of its two anchors as a chain minus the first anchor's own
        self.chain_score = []
        gi = 0
        for c, m in zip(self.chain_cases, self.chain_meta):
            a0, n = int(c["a0"]), int(c["n_anc"])
            A = self.anchors[a0:a0 + n]
            seq = self.pool.seqs[m["read"]]; ref = self.ref[m["ref_off"]:]
            sc, gn = ora.chain(seq, int(c["strand"]), ref, int(c["ref_bases"]), A, n - 1)
            assert len(gn) == n - 1
            self.chain_score.append(sc)
            for j in range(n - 1):
                g = self.gaps[gi]; gm = self.gap_meta[gi]
                two = np.array([[g["pq"], g["pt"], g["pl"], -1], [g["cq"], g["ct"], g["cl"], 0]], np.int32)
                s2, g2 = ora.chain(seq, int(c["strand"]), ref, int(c["ref_bases"]), two, 1)
                assert int(g2[0]) == int(gn[j])
                gm["nodes"] = int(gn[j]); gm["gain"] = s2 - (int(g["pl"]) - 9 + 1)
                # gap_lane's reasons to leave a gap to the cooperative form, from the inputs and the oracle's node count
                L = len(seq); pl = int(g["pl"])
                t_len = int(g["ct"]) - (int(g["pt"]) - 3 + pl) + 3
                q_bg, q_ed = int(g["pq"]) + pl - 8, int(g["cq"]) - 1
                hi = min(q_ed, L - 9); n_q = hi - q_bg + 1 if q_bg <= hi else 0
                ref_offset = int(g["pt"]) - 3 + pl
                why = []
                if t_len >= k.GL_MAXT:
                    why.append("maxt")
                elif t_len > 12 and n_q > 0 and t_len - 8 > 4:
                    if q_bg < 8 or q_ed + 58 >= L:
                        why.append("read_end")
                    if ref_offset + t_len + 64 >= int(c["ref_bases"]):
                        why.append("text_end")
                    if not why and ((q_ed + 58) >> 5) + 1 - ((q_bg - 8) >> 5) + 1 > k.GL_QW:
                        why.append("words")
                    if not why and gm["nodes"] > k.GL_NODES:
                        why.append("nodes")
                gm["why"] = why
                gi += 1
        return self


def _chain(rng, gs, n_anchors, kinds, small=False):
    """one read over one text: anchors are exact copies of the text, the stretches between them what `kinds` says
    (small: anchors of 13 .. 14 bases and no flanks, so that 400 of them fit a read of 8000)"""
    T, Q, anchors = [], [], []
    lead_t, lead_q = (0, 0) if small else (rng.choice([0, 0, 3, 40]), rng.choice([0, 0, 40, 200]))
    T += [rng.randrange(4) for _ in range(lead_t)]; Q += [rng.randrange(4) for _ in range(lead_q)]
    for i in range(n_anchors):
        kind = kinds[i % len(kinds)] if i else None
        flank = None
        if i:
            if kind == "poly":                 # a homopolymer gap with homopolymer flanks: every window position holds the same 9-mer
                b = rng.randrange(4); flank = [b] * 9
                gt = rng.randint(7, 40); gq = max(0, gt - rng.randint(0, 8)) if rng.random() < 0.5 else rng.randint(0, 12)
                if rng.random() < 0.7:         # GL_NODES window positions exactly: the widest gap gap_lane still scores
                    gt, gq = rng.randint(7, 20), 4
                tg, qg = [b] * gt, [b] * gq
            elif kind == "repeat":
                u = [rng.randrange(4) for _ in range(rng.randint(2, 9))]; gt = rng.randint(10, 180)
                tg = (u * 100)[:gt]; qg = mutate(rng, tg, rng.choice([0, 0.05]))
            elif kind == "long":
                gt = rng.randint(190, 600); tg = [rng.randrange(4) for _ in range(gt)]; qg = mutate(rng, tg, rng.choice([0.02, 0.1, 0.2]))
            elif kind == "huge":
                gt = rng.randint(600, 1990); tg = [rng.randrange(4) for _ in range(gt)]; qg = mutate(rng, tg, rng.choice([0.02, 0.1]))[:1990]
            elif kind == "insert":             # a short stretch of the text against a long one of the read: many query words
                gt = rng.randint(20, 150); tg = [rng.randrange(4) for _ in range(gt)]; qg = mutate(rng, tg, 0.05) + [rng.randrange(4) for _ in range(rng.randint(250, 500))]
            elif kind == "tiny":
                gt = rng.randint(0, 6); tg = [rng.randrange(4) for _ in range(gt)]; qg = [rng.randrange(4) for _ in range(rng.randint(0, 6))]
            elif kind == "short":
                gt = rng.randint(7, 10); tg = [rng.randrange(4) for _ in range(gt)]; qg = mutate(rng, tg, 0.1)[:10]
            elif kind == "unrelated":
                gt = rng.randint(7, 180); tg = [rng.randrange(4) for _ in range(gt)]; qg = [rng.randrange(4) for _ in range(max(0, gt + rng.randint(-5, 5)))]
            else:
                gt = rng.randint(7, 180); tg = [rng.randrange(4) for _ in range(gt)]; qg = mutate(rng, tg, rng.choice([0, 0.03, 0.08, 0.15, 0.25]))
            T += tg; Q += qg
        al = rng.randint(13, 14) if small else rng.randint(13, 60)
        a = [rng.randrange(4) for _ in range(al)]
        if flank:
            a[:9] = flank
            prev = anchors[-1]; pq, pt, pl = prev
            T[pt + pl - 9:pt + pl] = flank; Q[pq + pl - 9:pq + pl] = flank
        anchors.append((len(Q), len(T), al))
        T += a; Q += a
    tail_t, tail_q = (0, 0) if small else (rng.choice([0, 10, 70, 300]), rng.choice([0, 5, 60, 300]))
    T += [rng.randrange(4) for _ in range(tail_t)]; Q += [rng.randrange(4) for _ in range(tail_q)]
    while len(Q) < 200:
        Q.append(rng.randrange(4))
    seq = bytes(b"ACGT"[b] for b in Q)                 # (codes: A 0, C 1, G 2, T 3)
    strand = rng.choice([FORWARD, REVERSE])
    if strand == REVERSE:              # the chain lies on the reverse strand: the read is the reverse complement of Q
        seq = bytes(b"ACGT"[3 - b] for b in reversed(Q))
    assert 200 <= len(seq) <= 8000, len(seq)
    r = gs.pool.add(seq)
    ref_off, ref_bases = gs.add_text(np.array(T, np.uint8))
    gs.add_chain(r, strand, ref_off, ref_bases, anchors)


def build_gap_set(k, ora, seed, n_chains):
    rng = random.Random(seed)
    gs = GapSet(k)
    mixes = [["plain"], ["plain", "poly"], ["poly"], ["plain", "repeat", "tiny"], ["long"], ["insert", "plain"], ["long", "plain"], ["poly", "tiny", "unrelated"], ["huge", "plain"], ["insert"], ["poly"], ["poly", "plain"]]
    for done in range(n_chains):
        if done % 10 == 0:                     # the long chains: 100 .. 400 anchors
            n = rng.choice([100, 200, 400])
            _chain(rng, gs, n, ["tiny"] if n == 400 else ["tiny", "short"], small=True)
            continue
        n = rng.choice([1, 2, 2, 3, 5, 12, 30])
        kinds = mixes[done % len(mixes)]
        if "long" in kinds or "insert" in kinds or "huge" in kinds:       # (the read stays within 8000 bases)
            n = min(n, 3 if "huge" in kinds else 9)
        _chain(rng, gs, n, kinds)
    return gs.finish(ora)
