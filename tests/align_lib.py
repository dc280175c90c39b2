"""The definition of the base-level alignment of a record (include/desamba_amd.h) restated in numpy: the generations of
the diagonal-transition recurrence with the candidate each diagonal chose, the walk back by the moves alone, the replay from (0, 0),
the merged run-length operations, the trace-room rule, and the SAM text.  The device is held against this operation for operation;
the model asserts on every pair what the definition promises of its own path."""
import numpy as np

import identity_lib as I

OPS, NOTRACE, NOROOM, UNALIGNED = 1, 2, 4, 8
OP_I, OP_D, OP_EQ, OP_X = 1, 2, 7, 8
OP_CHAR = {OP_I: "I", OP_D: "D", OP_EQ: "=", OP_X: "X"}
TRACE_KIB = 2048
NEG = -(1 << 30)
STEP = 32
NO_ALN = (0, 0, 0, 0, 0)                                            # (n_ops, n_x, n_ins, n_del, flags) of a hit that is not counted


def band(n, m, B):
    d = m - n
    lo, hi = min(0, d) - B, max(0, d) + B
    return d, lo, hi, hi - lo + 1


def gen_bytes(n, m, B):
    """R: the trace of one generation, two bit planes of 64 diagonals per 16 bytes"""
    return 16 * ((band(n, m, B)[3] + 63) // 64)


def has_path(n, m, B, edits, trace_kib=TRACE_KIB):
    """the trace-room rule for an aligned record: a function of (n, m, band, edits, trace_kib) alone"""
    return edits * gen_bytes(n, m, B) <= trace_kib * 1024


class _Slider:
    """from cells (i, i + k): the first i' >= i with Q[i'] != T[i' + k], or where the rectangle ends; many cells at once"""

    def __init__(self, Q, T):
        self.n, self.m = len(Q), len(T)
        self.Q = np.concatenate([np.asarray(Q, dtype=np.int16), np.full(STEP + 1, -1, dtype=np.int16)])
        self.T = np.concatenate([np.asarray(T, dtype=np.int16), np.full(STEP + 1, -2, dtype=np.int16)])
        self.step = np.arange(STEP, dtype=np.int64)

    def many(self, i, k):
        i = i.copy()
        live = np.arange(len(i))
        while len(live):
            a, j = i[live], i[live] + k[live]
            eq = self.Q[a[:, None] + self.step] == self.T[j[:, None] + self.step]
            run = np.where(eq.all(axis=1), STEP, np.argmin(eq, axis=1))
            run = np.minimum(run, np.minimum(self.n - a, self.m - j))
            i[live] = a + run
            live = live[(run == STEP) & (a + run < self.n) & (j + run < self.m)]
        return i

    def one(self, i, k):
        return int(self.many(np.array([i], dtype=np.int64), np.array([k], dtype=np.int64))[0])


def generations(Q, T, B, cap):
    """the forward pass: (edits or None when the cap ends it, [(klo, moves of generation e = 1 ..)]).  moves[k - klo] is the code of
    the candidate diagonal k chose: 0 the mismatch from k (wins ties), 1 a base of T alone from k - 1 if strictly further, 2 a base of
    Q alone from k + 1 if strictly further, 3 none moved (unreached, or the value carried)"""
    n, m = len(Q), len(T)
    d, lo, hi, W = band(n, m, B)
    S = _Slider(Q, T)
    prev = np.full(W + 2, NEG, dtype=np.int64)
    prev[1 - lo] = S.one(0, 0)
    if d == 0 and prev[1 - lo] >= n:
        return 0, []
    gens = []
    e = 0
    while e < cap:
        e += 1
        klo, khi = max(lo, -e), min(hi, e)
        ks = np.arange(klo, khi + 1, dtype=np.int64)
        x = ks - lo + 1
        p, pl, pr = prev[x], prev[x - 1], prev[x + 1]
        c = p.copy()
        mv = np.full(len(ks), 3, dtype=np.uint8)
        a = (p >= 0) & (p + 1 <= n) & (p + 1 + ks <= m)
        c[a] = p[a] + 1; mv[a] = 0
        b = (pl >= 0) & (pl + ks <= m) & (pl > c)
        c[b] = pl[b]; mv[b] = 1
        g = (pr >= 0) & (pr + 1 <= n) & (pr + 1 > c)
        c[g] = pr[g] + 1; mv[g] = 2
        r = c >= 0
        c[r] = S.many(c[r], ks[r])
        cur = np.full(W + 2, NEG, dtype=np.int64)
        cur[x] = c
        gens.append((klo, mv))
        prev = cur
        if klo <= d <= khi and cur[d - lo + 1] >= n:
            return e, gens
    return None, gens


def merge(ops):
    out = []
    for op, ln in ops:
        if ln == 0:
            continue
        if out and out[-1][0] == op:
            out[-1] = (op, out[-1][1] + ln)
        else:
            out.append((op, ln))
    return out


def path(Q, T, B, edits, gens):
    """the walk back from generation `edits` on diagonal d to generation 0 on diagonal 0 by the moves alone, then the replay from
    (0, 0); returns the merged operations [(op, len)].  Asserts what the definition promises."""
    n, m = len(Q), len(T)
    d = m - n
    moves = [0] * (edits + 1)
    k = d
    for e in range(edits, 0, -1):
        klo, mv = gens[e - 1]
        assert 0 <= k - klo < len(mv)
        moves[e] = int(mv[k - klo])
        assert moves[e] != 3, "a wasted generation on the path"
        k += (moves[e] == 2) - (moves[e] == 1)
    assert k == 0
    S = _Slider(Q, T)
    ops = []
    i = k = 0
    for e in range(1, edits + 1):
        i2 = S.one(i, k)
        ops.append((OP_EQ, i2 - i)); i = i2
        if moves[e] == 0:
            assert i < n and i + k < m
            ops.append((OP_X, 1)); i += 1
        elif moves[e] == 1:
            assert i + k < m
            ops.append((OP_D, 1)); k += 1
        else:
            assert i < n
            ops.append((OP_I, 1)); i += 1; k -= 1
    i2 = S.one(i, k)
    ops.append((OP_EQ, i2 - i)); i = i2
    assert (i, i + k) == (n, m), "the replay does not end on (n, m)"
    ops = merge(ops)
    nx, ni, nd = replay_check(Q, T, ops)
    assert nx + ni + nd == edits and len(ops) <= 2 * edits + 1
    return ops


def replay_check(Q, T, ops):
    """the operations consume exactly Q and T, = columns are equal and X columns unequal (by code); returns (n_x, n_ins, n_del)"""
    Q = np.asarray(Q); T = np.asarray(T)
    i = j = 0
    cnt = {OP_X: 0, OP_I: 0, OP_D: 0, OP_EQ: 0}
    last = None
    for op, ln in ops:
        assert ln > 0 and op in cnt and op != last, (op, ln)
        last = op
        if op in (OP_EQ, OP_X):
            assert i + ln <= len(Q) and j + ln <= len(T)
            same = Q[i:i + ln] == T[j:j + ln]
            assert same.all() if op == OP_EQ else not same.any(), (op, i, j, ln)
            i += ln; j += ln
        elif op == OP_I:
            i += ln
        else:
            j += ln
        cnt[op] += ln
    assert (i, j) == (len(Q), len(T)), (i, j, len(Q), len(T))
    return cnt[OP_X], cnt[OP_I], cnt[OP_D]


def align(Q, T, B=I.BAND, permille=I.PERMILLE, trace_kib=TRACE_KIB):
    """(identity record, (n_ops, n_x, n_ins, n_del, flags), operations) of one pair; the operations are there with OPS alone"""
    n, m = len(Q), len(T)
    rec, cap = I.classify_pair(n, m, permille)
    if rec is not None:
        return rec, (0, 0, 0, 0, UNALIGNED), []
    edits, gens = generations(Q, T, B, cap)
    if edits is None:
        return (cap + 1, n, m, I.OVER), (0, 0, 0, 0, UNALIGNED), []
    rec = (edits, n, m, I.EXACT if edits <= B else 0)
    ops = path(Q, T, B, edits, gens)                                  # (the assertions hold whatever the room is)
    if not has_path(n, m, B, edits, trace_kib):
        return rec, (0, 0, 0, 0, NOTRACE), []
    nx, ni, nd = replay_check(Q, T, ops)
    return rec, (len(ops), nx, ni, nd, OPS), ops


def unpack(words):
    return [(int(w) & 15, int(w) >> 4) for w in words]


def record_ops(aln, ops, h):
    """the operations of record h of a batch's (records, ops) as [(op, len)]"""
    a = aln[h]
    return unpack(ops[int(a["ops_off"]):int(a["ops_off"]) + int(a["n_ops"])])


def as_tuple(a):
    return (int(a["n_ops"]), int(a["n_x"]), int(a["n_ins"]), int(a["n_del"]), int(a["flags"]))


def batch(idx, recs, res, B=I.BAND, permille=I.PERMILLE, trace_kib=TRACE_KIB):
    """per hit of a batch's result: (identity record, alignment tuple, operations); NO_ALN for a hit that is not counted"""
    out = [(I.ZERO, NO_ALN, [])] * res.n_hits
    for i, (name, seq, qual) in enumerate(recs):
        rr = res.reads[i]
        for k in range(rr.n):
            h = res.hits[rr.first + k]
            if I.counted(h, k):
                Q, T = I.hit_pair(idx, seq, h)
                out[rr.first + k] = align(Q, T, B, permille, trace_kib)
    return out


# ---------------------------------------------------------------- the SAM text

COMP = bytes.maketrans(b"ACGT", b"TGCA")


def strand_seq(seq, forward):
    s = bytes(c if c in b"ACGT" else ord("N") for c in seq.upper())
    return s if forward else s.translate(COMP)[::-1]


def cigar(ops):
    return "".join("%d%s" % (ln, OP_CHAR[op]) for op, ln in ops)


def header(idx):
    out = [b"@HD\tVN:1.6\tSO:unknown\n"]
    out += [b"@SQ\tSN:%s\tLN:%d\n" % (idx.ref_name(r).encode(), idx.ref_len(r)) for r in range(idx.n_ref)]
    return b"".join(out) + b"@PG\tID:desamba_amd\n"


def mapq_pri(hits):
    if len(hits) == 1 or ((hits[0].sum_score - hits[1].sum_score) & 0xffffffff) > 5:
        return 30
    return ((hits[0].sum_score - hits[1].sum_score) << 2) & 0xffffffff


def sam_lines(idx, recs, res, ident, alns):
    """the text of dsb_format_aligned_sam over a batch.  ident: (edits, n, m, flags) per hit; alns: (flags, operations) per hit"""
    out = []
    for i, (name, seq, qual) in enumerate(recs):
        name = name if isinstance(name, bytes) else name.encode()
        L = len(seq)
        rr = res.reads[i]
        if rr.n == 0:
            out.append(b"%s\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t%s\n" % (name, strand_seq(seq, True) or b"*", qual if qual and L else b"*"))
            continue
        hits = [res.hits[rr.first + k] for k in range(rr.n)]
        mq = mapq_pri(hits)
        for k, h in enumerate(hits):
            if not I.counted(h, k):
                continue
            known = h.ref_ID < idx.n_ref
            LN = idx.ref_len(h.ref_ID) if known else 0
            qs, qe, ts, te = I.interval(h, L, LN)
            qe = max(qe, qs)
            fw = h.direction != 0
            sup = k > 0
            flags, ops = alns[rr.first + k]
            S = strand_seq(seq, fw)
            Ql = (qual if fw else qual[::-1]) if qual else None
            if sup:
                S = S[qs:qe]
                Ql = Ql[qs:qe] if Ql else None
            if flags & OPS:
                clip = "H" if sup else "S"
                cg = ("%d%s" % (qs, clip) if qs else "") + cigar(ops) + ("%d%s" % (L - qe, clip) if L - qe else "")
                tag = b"NM:i:%d" % ident[rr.first + k][0]
            else:
                cg, tag = "*", b"xa:i:%d" % flags
            out.append(b"%s\t%d\t%s\t%d\t%d\t%s\t*\t0\t0\t%s\t%s\t%s\tAS:i:%d\n" % (
                name, (0 if fw else 16) + (0x800 if sup else 0), idx.ref_name(h.ref_ID).encode() if known else b"*", ts + 1 if known else 0,
                min(mq, 30) if sup else mq, cg.encode(), S or b"*", Ql if Ql and S else b"*", tag, h.sum_score))
    return b"".join(out)


def parse_cigar(cg):
    out, num = [], ""
    for ch in cg:
        if ch.isdigit():
            num += ch
        else:
            assert num and int(num) > 0 and ch in "SH=XID", cg
            out.append((ch, int(num))); num = ""
    assert not num, cg
    return out


def check_sam(idx, text):
    """a small SAM checker over header + lines: returns the number of lines that carry a CIGAR.  Per line: eleven fields and the
    tags, the query-consuming operations sum to len(SEQ), H on supplementary records only, the reference span from POS inside @SQ LN,
    NM == X + I + D, and = / X agree with SEQ against the reference text by code"""
    ln_of = {}
    checked = 0
    for line in text.decode().split("\n"):
        if not line:
            continue
        if line.startswith("@"):
            f = line.split("\t")
            if f[0] == "@SQ":
                ln_of[f[1][3:]] = int(f[2][3:])
            continue
        assert not line.endswith("\t"), line[:80]
        f = line.split("\t")
        assert len(f) >= 11, line[:80]
        flag, rname, pos, cg, seq, qual = int(f[1]), f[2], int(f[3]), f[5], f[9], f[10]
        assert qual == "*" or len(qual) == len(seq)
        if flag & 4:
            assert rname == "*" and pos == 0 and cg == "*" and len(f) == 11
            continue
        tags = dict((t[:2], t[5:]) for t in f[11:])
        assert "AS" in tags
        if cg == "*":
            assert "xa" in tags and "NM" not in tags and int(tags["xa"]) and not int(tags["xa"]) & OPS
            continue
        ops = parse_cigar(cg)
        assert all(op not in "SH" for op, _ in ops[1:-1])
        assert all(op != "H" for op, _ in ops) or flag & 0x800, line[:80]
        assert all(op != "S" for op, _ in ops) or not flag & 0x800, line[:80]
        assert sum(n for op, n in ops if op in "S=XI") == len(seq), line[:80]
        span = sum(n for op, n in ops if op in "=XD")
        assert rname in ln_of and 1 <= pos and pos - 1 + span <= ln_of[rname], line[:80]
        assert int(tags["NM"]) == sum(n for op, n in ops if op in "XID"), line[:80]
        r = [x for x in range(idx.n_ref) if idx.ref_name(x) == rname][0]
        T = idx.ref_bases(r, pos - 1, span)
        Q = I.encode(seq).copy()
        if flag & 16:                                                 # (a letter that is no base was aligned as the complement of C)
            Q[np.frombuffer(seq.encode(), dtype=np.uint8) == ord("N")] = 2
        i = j = 0
        for op, n in ops:
            if op in "=X":
                same = Q[i:i + n] == T[j:j + n]
                assert same.all() if op == "=" else not same.any(), (line[:60], op, i, j)
                i += n; j += n
            elif op in "SI":
                i += n
            elif op == "D":
                j += n
        checked += 1
    return checked
