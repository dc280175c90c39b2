"""The definition of the per-hit edit distance and the per-reference identity (include/desamba_amd.h) restated in
numpy: the banded unit-cost DP row by row over the cells of the band, the flags, the cap, the records of a batch, the run's
table and the two texts.  The device computes the same value by diagonal transition; this is the yardstick it is held against."""
import numpy as np

EXACT, OVER, SKEW, EMPTY = 1, 2, 4, 8
BAD = OVER | SKEW | EMPTY
MAX_SKEW = 4096
BAND, PERMILLE = 256, 300
INF = 1 << 40
ZERO = (0, 0, 0, 0)


def banded_distance(Q, T, B, limit=None):
    """the cheapest path from (0, 0) to (n, m) with unit costs for a mismatch, a base of Q alone and a base of T alone, over the cells
    (i, j) with min(0, d) - B <= j - i <= max(0, d) + B, d = m - n.  Row i is held by diagonal: entry k - lo is cell (i, i + k).
    limit: the search stops at the first row whose cheapest cell costs more (row minima never fall) and returns limit + 1."""
    Q = np.asarray(Q, dtype=np.int64); T = np.asarray(T, dtype=np.int64)
    n, m = len(Q), len(T)
    d = m - n
    lo, hi = min(0, d) - B, max(0, d) + B
    W = hi - lo + 1
    ks = np.arange(lo, hi + 1, dtype=np.int64)
    # Tp[i + x] = T[i + ks[x] - 1], the base that cell (i, i + ks[x]) compares with Q[i - 1]; outside T a value no base equals
    Tp = np.concatenate([np.full(1 - lo, -1, dtype=np.int64), T, np.full(max(0, n + hi - m) + 1, -2, dtype=np.int64)])
    row = np.where((ks >= 0) & (ks <= m), ks, INF)                   # row 0: k bases of T alone
    step = np.arange(W, dtype=np.int64)
    for i in range(1, n + 1):
        j = i + ks
        diag = row + (Tp[i:i + W] != Q[i - 1])                        # from (i - 1, j - 1)
        up = np.concatenate([row[1:], [INF]]) + 1                     # from (i - 1, j): diagonal k + 1 of the row above
        t = np.minimum(diag, up)
        t[(j < 0) | (j > m)] = INF
        cur = np.minimum.accumulate(t - step) + step                  # from (i, j - 1), any number of times
        cur[(j < 0) | (j > m)] = INF
        row = np.minimum(cur, INF)
        if limit is not None and row.min() > limit:
            return limit + 1
    return int(row[d - lo])


def banded_distances(pairs, B, limits=None):
    """banded_distance over many pairs at once (the same rows, one numpy operation per row for all pairs still running; a test
    holds it against banded_distance): pairs of non-empty (Q, T), the longest Q first internally, results in the order given"""
    R = len(pairs)
    if R == 0:
        return []
    order = sorted(range(R), key=lambda r: -len(pairs[r][0]))
    ns = np.array([len(pairs[r][0]) for r in order], dtype=np.int64); ms = np.array([len(pairs[r][1]) for r in order], dtype=np.int64)
    ds = ms - ns
    los = np.minimum(0, ds) - B; his = np.maximum(0, ds) + B
    Ws = his - los + 1
    Wmax, nmax = int(Ws.max()), int(ns[0])
    step = np.arange(Wmax, dtype=np.int64)
    ks = los[:, None] + step[None, :]
    inband = step[None, :] < Ws[:, None]
    TP = np.full((R, nmax + Wmax + 1), -2, dtype=np.int64); QP = np.full((R, nmax), -3, dtype=np.int64)
    for x, r in enumerate(order):
        Q, T = pairs[r]
        TP[x, 1 - los[x]:1 - los[x] + ms[x]] = T; QP[x, :ns[x]] = Q
    lim = None if limits is None else np.array([limits[r] for r in order], dtype=np.int64)
    row = np.where((ks >= 0) & (ks <= ms[:, None]) & inband, ks, INF)
    ans = np.full(R, -1, dtype=np.int64)
    live = R
    for i in range(1, nmax + 1):
        while live and ns[live - 1] < i:
            live -= 1
        a = slice(0, live)
        j = i + ks[a]
        out = (j < 0) | (j > ms[a, None]) | ~inband[a]
        diag = row[a] + (TP[a, i:i + Wmax] != QP[a, i - 1:i])
        up = np.concatenate([row[a, 1:], np.full((live, 1), INF, dtype=np.int64)], axis=1) + 1
        t = np.minimum(diag, up)
        t[out] = INF
        cur = np.minimum.accumulate(t - step[None, :], axis=1) + step[None, :]
        cur[out] = INF
        row[a] = np.minimum(cur, INF)
        done = np.nonzero(ns[a] == i)[0]
        ans[done] = row[done, (ds - los)[done]]
        if lim is not None:
            over = (row[a].min(axis=1) > lim[a]) & (ans[a] < 0)
            ans[:live][over] = lim[a][over] + 1
    res = [0] * R
    for x, r in enumerate(order):
        v = int(ans[x])
        res[r] = int(min(v, lim[x] + 1)) if lim is not None else v
    return res


def classify_pair(n, m, permille):
    """(record, cap): the record of a pair that is not aligned (EMPTY, SKEW) or None, and its E_cap"""
    if n == 0 or m == 0:
        return (0, n, m, EMPTY), 0
    if abs(m - n) > MAX_SKEW:
        return (0, n, m, SKEW), 0
    return None, max(n, m) * permille // 1000


def finish(dist, n, m, B, cap):
    if dist > cap:
        return (cap + 1, n, m, OVER)
    return (dist, n, m, EXACT if dist <= B else 0)


def record(Q, T, B=BAND, permille=PERMILLE):
    """(edits, n, m, flags) of one pair"""
    n, m = len(Q), len(T)
    r, cap = classify_pair(n, m, permille)
    return r if r is not None else finish(banded_distance(Q, T, B, cap), n, m, B, cap)


def records_of(pairs, B=BAND, permille=PERMILLE):
    """record() of every pair, the alignments run together (banded_distances)"""
    out = [None] * len(pairs); caps = {}
    for p, (Q, T) in enumerate(pairs):
        out[p], cap = classify_pair(len(Q), len(T), permille)
        if out[p] is None:
            caps[p] = cap
    # (pairs of similar length together: a row costs as much as the widest band times the pairs still running)
    todo = sorted(caps, key=lambda p: (abs(len(pairs[p][1]) - len(pairs[p][0])) // 64, len(pairs[p][0])))
    for lo_ in range(0, len(todo), 64):
        grp = todo[lo_:lo_ + 64]
        dist = banded_distances([pairs[p] for p in grp], B, [caps[p] for p in grp])
        for p, dv in zip(grp, dist):
            out[p] = finish(dv, len(pairs[p][0]), len(pairs[p][1]), B, caps[p])
    return out


def identity(rec):
    e, n, m, f = rec
    return 0.0 if (f & BAD) or max(n, m) == 0 else 1.0 - e / max(n, m)


CODE = np.full(256, 1, dtype=np.uint8)                             # CLY_Bit: anything that is not A / G / T is C
for ch, c in ((b"Aa", 0), (b"Gg", 2), (b"Tt", 3)):
    for b in ch:
        CODE[b] = c


REF_CODE = np.zeros(256, dtype=np.uint8)                          # the index builder's bin_Bit: anything that is not ACGTacgt is A
for ch, c in ((b"Cc", 1), (b"Gg", 2), (b"Tt", 3)):
    for b in ch:
        REF_CODE[b] = c


def encode(seq):
    """a read's codes"""
    return CODE[np.frombuffer(seq if isinstance(seq, bytes) else seq.encode(), dtype=np.uint8)]


def encode_ref(seq):
    """the codes of reference text as the index holds it"""
    return REF_CODE[np.frombuffer(seq if isinstance(seq, bytes) else seq.encode(), dtype=np.uint8)]


def interval(hit, L, LN):
    """(qs, qe, ts, te) of a hit on a read of L bases and a reference of LN"""
    return min(hit.q_st, L), min(hit.q_ed, L), min(hit.t_st, LN), min(hit.t_ed, LN)


def counted(hit, k):
    return k == 0 or hit.pri_index == 0


def hit_pair(idx, seq, hit):
    """Q and T of one hit: the bases of the strand the chain was built on, and of its reference"""
    F = encode(seq)
    LN = idx.ref_len(hit.ref_ID) if hit.ref_ID < idx.n_ref else 0
    qs, qe, ts, te = interval(hit, len(F), LN)
    S = F if hit.direction == 1 else (3 - F[::-1])
    Q = S[qs:qe] if qe > qs else S[:0]
    T = idx.ref_bases(hit.ref_ID, ts, te - ts) if te > ts else np.zeros(0, dtype=np.uint8)
    return Q, T


def records(idx, recs, res, B=BAND, permille=PERMILLE):
    """one (edits, n, m, flags) per hit of a batch's result: the counted records aligned, all-zero for every other hit"""
    out = [ZERO] * res.n_hits
    at, pairs = [], []
    for i, (name, seq, qual) in enumerate(recs):
        rr = res.reads[i]
        for k in range(rr.n):
            h = res.hits[rr.first + k]
            if counted(h, k):
                at.append(rr.first + k); pairs.append(hit_pair(idx, seq, h))
    for a, r in zip(at, records_of(pairs, B, permille)):
        out[a] = r
    return out


def table(idx, res, n_reads, recs_):
    """the per-reference sums of a batch's records: n_ref rows of (records, q_bases, t_bases, edits, exact, unaligned)"""
    tab = [[0] * 6 for _ in range(idx.n_ref)]
    for i in range(n_reads):
        rr = res.reads[i]
        for k in range(rr.n):
            h = res.hits[rr.first + k]
            if not counted(h, k) or h.ref_ID >= idx.n_ref:
                continue
            e, n, m, f = recs_[rr.first + k]
            row = tab[h.ref_ID]
            if f & BAD:
                row[5] += 1
            else:
                row[0] += 1; row[1] += n; row[2] += m; row[3] += e; row[4] += 1 if f & EXACT else 0
    return [tuple(r) for r in tab]


def add_tables(a, b):
    return [tuple(x + y for x, y in zip(r, s)) for r, s in zip(a, b)]


def as_tuples(arr):
    return [tuple(int(v) for v in r) for r in arr.tolist()]


def lines(idx, recs, res, recs_):
    """the text of dsb_format_identity over a batch"""
    out = []
    for i, (name, seq, qual) in enumerate(recs):
        name = name if isinstance(name, bytes) else name.encode()
        rr = res.reads[i]
        if rr.n == 0:
            out.append(name + b"\t*\t*\t0\t0\t0\t0\t0\t0\t0.0000\t0\n")
        for k in range(rr.n):
            h = res.hits[rr.first + k]
            if not counted(h, k):
                continue
            LN = idx.ref_len(h.ref_ID) if h.ref_ID < idx.n_ref else 0
            qs, qe, ts, te = interval(h, len(seq), LN)
            r = recs_[rr.first + k]
            rname = idx.ref_name(h.ref_ID).encode() if h.ref_ID < idx.n_ref else b"*"
            out.append(b"%s\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%.4f\t%d\n" % (name, rname, b"+" if h.direction else b"-", qs, qe, ts, te, h.sum_score, r[0], identity(r), r[3]))
    return b"".join(out)


def table_text(idx, tab):
    out = [b"#rname\trecords\tq_bases\tt_bases\tedits\tidentity\texact\tunaligned\n"]
    for r, (rec, qb, tb, ed, ex, un) in enumerate(tab):
        if rec + un == 0:
            continue
        big = max(qb, tb)
        out.append(b"%s\t%d\t%d\t%d\t%d\t%.4f\t%d\t%d\n" % (idx.ref_name(r).encode(), rec, qb, tb, ed, (1.0 - ed / big) if big else 0.0, ex, un))
    return b"".join(out)
