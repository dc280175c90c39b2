"""Checkpoint mode of the base-level alignment (include/desamba_amd.h) restated in Python: the plan of a record, which
records get a path, and the checkpointed walk itself -- a forward pass that keeps the moves of one segment of K generations and the
furthest-reaching values of every K-th generation, and a walk back that recomputes the earlier segments from their checkpoints.  The
operations a record gets are always those of tests/align_lib.py: the definition of the alignment does not change with the mode."""
import numpy as np

import align_lib as A
import identity_lib as I

FULL, CHECKPOINT = 0, 1
NEG = A.NEG


def sizes(n, m, B, permille, trace_kib):
    """(E_cap, Rb, C, Mv, room): bytes of a generation's trace, of a checkpoint, of the move area, of the place"""
    W = A.band(n, m, B)[3]
    cap = max(n, m) * permille // 1000
    return cap, 16 * ((W + 63) // 64), 16 * ((4 * (W + 2) + 15) // 16), 16 * ((cap + 15) // 16), trace_kib * 1024


def plan(n, m, B=I.BAND, permille=I.PERMILLE, trace_kib=A.TRACE_KIB):
    """(K, n_ck) or None: a function of (n, m, band, permille, trace_kib) alone"""
    cap, Rb, C, Mv, room = sizes(n, m, B, permille, trace_kib)
    a = room - Mv
    if a < 0:
        return None
    if cap * Rb <= a:
        return max(cap, 1), 0
    K = a // 2 // Rb
    if K < 1:
        return None
    n_ck = (cap - 1) // K
    if n_ck * C > a - K * Rb:
        return None
    return K, n_ck


def smallest_room(n, m, B, permille):
    """the smallest trace_kib with a plan"""
    kib = 1
    while plan(n, m, B, permille, kib) is None:
        kib += 1
    return kib


def align_ck(Q, T, B=I.BAND, permille=I.PERMILLE, trace_kib=A.TRACE_KIB):
    """align_lib.align with unlimited room, flagged NOTRACE where the record has no plan"""
    rec, aln, ops = A.align(Q, T, B, permille, 1 << 40)
    if aln[4] & A.OPS and plan(len(Q), len(T), B, permille, trace_kib) is None:
        return rec, (0, 0, 0, 0, A.NOTRACE), []
    return rec, aln, ops


def generation(S, n, m, lo, hi, e, prev, cur):
    """generation e of align_lib.generations written into cur in place, as the device does: only the diagonals [klo, khi] are stored,
    the rest of cur is whatever it held.  Returns (klo, moves)."""
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
    cur[x] = c
    return klo, mv


def walk_segment(seg, moves, e_lo, e_hi, k):
    for e in range(e_hi, e_lo, -1):
        klo, mv = seg[e - 1 - e_lo]
        assert 0 <= k - klo < len(mv)
        moves[e] = int(mv[k - klo])
        assert moves[e] != 3, "a wasted generation on the path"
        k += (moves[e] == 2) - (moves[e] == 1)
    return k


def checkpointed_ops(Q, T, B, cap, K, fill=True):
    """(edits, operations) by the checkpointed walk with segments of K generations, or (None, None) over the cap.  Memory: two
    generations of values, the moves of K generations, one generation of values per checkpoint, one move per edit.
    fill=False leaves cur as it is on a restore (what the walk must not do: see test_checkpointed_walk_needs_the_fill)."""
    n, m = len(Q), len(T)
    d, lo, hi, W = A.band(n, m, B)
    S = A._Slider(Q, T)
    first = S.one(0, 0)
    prev = np.full(W + 2, NEG, dtype=np.int64); cur = prev.copy()
    prev[1 - lo] = first
    if d == 0 and first >= n:
        return 0, A.merge([(A.OP_EQ, n)])
    seg, ckpt = [None] * K, []
    e, hit = 0, False
    while e < cap and not hit:
        e += 1
        seg[(e - 1) % K] = generation(S, n, m, lo, hi, e, prev, cur)
        hit = max(lo, -e) <= d <= min(hi, e) and cur[d - lo + 1] >= n
        if e % K == 0 and e < cap:
            ckpt.append(cur.copy())
        prev, cur = cur, prev
    if not hit:
        return None, None
    E = e
    moves = [0] * (E + 1)
    s = (E - 1) // K
    k = walk_segment(seg, moves, s * K, E, d)
    while s:
        s -= 1
        if s:
            prev[:] = ckpt[s - 1]
        else:
            prev[:] = NEG; prev[1 - lo] = first
        if fill:
            cur[:] = NEG
        for e in range(s * K + 1, (s + 1) * K + 1):
            seg[e - 1 - s * K] = generation(S, n, m, lo, hi, e, prev, cur)
            prev, cur = cur, prev
        k = walk_segment(seg, moves, s * K, (s + 1) * K, k)
    assert k == 0
    ops = []
    i = k = 0
    for e in range(1, E + 1):
        i2 = S.one(i, k)
        ops.append((A.OP_EQ, i2 - i)); i = i2
        if moves[e] == 0:
            assert i < n and i + k < m
            ops.append((A.OP_X, 1)); i += 1
        elif moves[e] == 1:
            assert i + k < m
            ops.append((A.OP_D, 1)); k += 1
        else:
            assert i < n
            ops.append((A.OP_I, 1)); i += 1; k -= 1
    i2 = S.one(i, k)
    ops.append((A.OP_EQ, i2 - i)); i = i2
    assert (i, i + k) == (n, m), "the replay does not end on (n, m)"
    return E, A.merge(ops)
