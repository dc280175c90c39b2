"""Per-hit edit distance and per-reference identity (k_ident_list, k_hit_edits, k_ident_ref, dsb_ctx_edit_pairs; classify --identity /
--identity-refs).  The numpy model of tests/identity_lib.py is the hard assertion, record for record and exact; the model
itself is held against a plain full-matrix DP written here, and the two texts against typed-out files (tests/golden/identity)."""
import os
import subprocess

import numpy as np
import pytest

import identity_lib as M
from conftest import GOLDEN, ROOT

CLI = os.path.join(ROOT, "desamba_amd", "bin", "deSAMBA")
SYNTH = os.path.join(GOLDEN, "synth")
IDENT = os.path.join(GOLDEN, "identity")
SIZES = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129]


# ---------------------------------------------------------------- an independent DP and the pairs the tests share

def plain_dp(Q, T, band=None):
    """the textbook O(nm) matrix, cell by cell; band = (lo, hi): cells with a diagonal j - i outside it do not exist"""
    n, m = len(Q), len(T)
    BIG = 10 ** 9
    D = [[BIG] * (m + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        for j in range(m + 1):
            if band is not None and not (band[0] <= j - i <= band[1]):
                continue
            if i == 0 and j == 0:
                D[i][j] = 0
                continue
            best = BIG
            if i and j:
                best = min(best, D[i - 1][j - 1] + (0 if Q[i - 1] == T[j - 1] else 1))
            if i:
                best = min(best, D[i - 1][j] + 1)
            if j:
                best = min(best, D[i][j - 1] + 1)
            D[i][j] = best
    return D[n][m]


def band_of(n, m, B):
    d = m - n
    return (min(0, d) - B, max(0, d) + B)


def rnd(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def subst(Q, at):
    T = Q.copy()
    for p in at:
        T[p] = (T[p] + 1) % 4
    return T


def noisy(rng, Q, err):
    """substitutions, deletions and insertions at rate err in all"""
    out = []
    for b in Q:
        r = rng.random()
        if r < err / 3:
            out.append((int(b) + 1 + int(rng.integers(0, 3))) % 4)
        elif r < 2 * err / 3:
            continue
        elif r < err:
            out.append(int(b)); out.append(int(rng.integers(0, 4)))
        else:
            out.append(int(b))
    return np.array(out, dtype=np.uint8)


def fit(rng, T, m):
    """T cut or filled up with random bases to m bases"""
    return np.concatenate([T[:m], rnd(rng, max(0, m - len(T)))])


def hand_cases():
    """(name, Q, T, B, permille, expected record or None where the plain DP gives it)"""
    rng = np.random.default_rng(12)
    E, O, S, Y = M.EXACT, M.OVER, M.SKEW, M.EMPTY
    Q50, Q40, Q64, Q30, Q100 = rnd(rng, 50), rnd(rng, 40), rnd(rng, 64), rnd(rng, 30), rnd(rng, 100)
    U = rnd(rng, 60)
    leaves = np.concatenate([U[:5], rnd(rng, 6), U[5:54]])           # six bases more at 5, the last six gone: n == m, the true path needs diagonal 6
    z = lambda n: np.zeros(n, dtype=np.uint8)
    return [
        ("identical", Q50, Q50.copy(), 8, 300, (0, 50, 50, E)),
        ("all mismatch", z(20), z(20) + 1, 4, 1000, (20, 20, 20, 0)),
        ("one insertion", Q40, np.concatenate([Q40[:17], [(Q40[17] + 1) % 4], Q40[17:]]).astype(np.uint8), 2, 300, (1, 40, 41, E)),
        ("B = 0, n == m: Hamming", Q64, subst(Q64, [0, 13, 31, 32, 63]), 0, 300, (5, 64, 64, 0)),
        ("B = 0, d != 0", Q30, np.concatenate([Q30, (Q30[-3:] + 1) % 4]).astype(np.uint8), 0, 300, (3, 30, 33, 0)),
        ("the best path leaves the band", U, leaves, 2, 1000, None),
        ("edits == B", Q100, subst(Q100, [10, 40, 70, 99]), 4, 300, (4, 100, 100, E)),
        ("edits == B + 1", Q100, subst(Q100, [10, 40, 70, 99]), 3, 300, (4, 100, 100, 0)),
        ("d == E_cap", Q100, subst(Q100, [10, 40, 70, 99]), 8, 40, (4, 100, 100, E)),
        ("d == E_cap + 1", Q100, subst(Q100, [10, 40, 60, 70, 99]), 8, 40, (5, 100, 100, O)),
        ("E_cap == 0, identical", Q30, Q30.copy(), 8, 1, (0, 30, 30, E)),
        ("E_cap == 0, one mismatch", Q30, subst(Q30, [29]), 8, 1, (1, 30, 30, O)),
        ("skew 4096", rnd(rng, 10), rnd(rng, 4106), 5, 1000, None),
        ("skew 4097", rnd(rng, 10), rnd(rng, 4107), 5, 1000, (0, 10, 4107, S)),
        ("skew -4097", rnd(rng, 4107), rnd(rng, 10), 5, 1000, (0, 4107, 10, S)),
        ("empty Q", z(0), rnd(rng, 5), 8, 300, (0, 0, 5, Y)),
        ("empty T", rnd(rng, 5), z(0), 8, 300, (0, 5, 0, Y)),
    ]


# ---------------------------------------------------------------- without a GPU

def test_model_against_an_independent_dp():
    rng = np.random.default_rng(7)
    pairs = []
    for k in range(60):
        n, m = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        Q = rnd(rng, n)
        pairs.append((Q, fit(rng, noisy(rng, Q, 0.3 * rng.random()), m)))
    for Q, T in pairs:
        full = plain_dp(Q, T)
        assert M.banded_distance(Q, T, max(len(Q), len(T))) == full            # the band covers the matrix
        for B in (0, 1, 3):
            got = M.banded_distance(Q, T, B)
            assert got == plain_dp(Q, T, band_of(len(Q), len(T), B)) >= full
            if got <= B:
                assert got == full                                             # what the EXACT flag promises
    # the model over many pairs at once is the model of each
    for B, pm in ((0, 300), (3, 1000), (40, 150)):
        assert M.records_of(pairs, B, pm) == [M.record(Q, T, B, pm) for Q, T in pairs]


def test_model_hand_cases():
    for name, Q, T, B, pm, want in hand_cases():
        got = M.record(Q, T, B, pm)
        if want is not None:
            assert got == want, name
        assert M.records_of([(Q, T)], B, pm) == [got], name
    c = {name: (Q, T, B, pm) for name, Q, T, B, pm, want in hand_cases()}
    Q, T, B, pm = c["the best path leaves the band"]
    got = M.record(Q, T, B, pm)
    assert got[0] == plain_dp(Q, T, band_of(60, 60, B)) > plain_dp(Q, T) and not got[3] & M.EXACT and plain_dp(Q, T) <= 12
    Q, T, B, pm = c["skew 4096"]
    got = M.record(Q, T, B, pm)
    assert got[1:] == (10, 4106, 0) and 4096 <= got[0] <= 4106
    assert M.identity((3, 100, 100, M.EXACT)) == 0.97 and M.identity((31, 100, 100, M.OVER)) == 0.0 and M.identity((0, 0, 5, M.EMPTY)) == 0.0


def golden_batch(D):
    """three reads, five hits and their identity records, typed out: tests/golden/identity/lines.txt and table.txt"""
    reads = D.make_reads([("r1 extra", b"A" * 100, None), ("r2", b"ACGT", None), ("r3", b"C" * 50, None)])
    hits = (D.DsbHit * 5)()
    #            ref   t_st   t_ed   q_st q_ed AS  indel dir primary pri_index pad
    hits[0] = D.DsbHit(0, 10, 110, 0, 100, 500, 0, 1, 1, 0, 0)
    hits[1] = D.DsbHit(2, 200, 260, 5, 70, 120, 0, 0, 3, 0, 0)            # supplementary
    hits[2] = D.DsbHit(1, 0, 90, 0, 90, 400, 0, 1, 2, 1, 0)               # secondary: no line
    hits[3] = D.DsbHit(462, 12000, 12030, 90, 101, 64, 0, 1, 3, 0, 0)     # t_ed beyond LN = 12020, q_ed beyond L = 100
    hits[4] = D.DsbHit(1000, 5, 55, 0, 50, 70, 0, 1, 1, 0, 0)             # no such reference
    rr = (D.DsbReadResult * 3)()
    rr[0].first, rr[0].n = 0, 4
    rr[1].first, rr[1].n = 0, 0
    rr[2].first, rr[2].n = 4, 1
    ident = np.zeros(5, dtype=D.HIT_IDENTITY_DTYPE)
    ident[0] = (3, 100, 100, M.EXACT); ident[1] = (20, 65, 60, 0); ident[3] = (4, 10, 20, M.OVER); ident[4] = (0, 50, 0, M.EMPTY)
    res = D.DsbResult(rr, hits, 5)
    res._keep = (rr, hits)
    return reads, res, ident


def test_format_identity(demo):
    import desamba_amd as D
    idx = D.Index(demo["index"])
    reads, res, ident = golden_batch(D)
    want = open(os.path.join(IDENT, "lines.txt"), "rb").read()
    recs = [("r1 extra", b"A" * 100, None), ("r2", b"ACGT", None), ("r3", b"C" * 50, None)]
    assert D.format_identity(idx, reads, res, ident) == want == M.lines(idx, recs, res, M.as_tuples(ident))
    L, C = D.lib(), D.C
    first = want[:want.index(b"r2")]
    args = (idx.h, C.byref(reads[0]), C.byref(res.reads[0]), res.hits, ident.ctypes.data_as(C.c_void_p))
    assert L.dsb_format_identity(*args, C.create_string_buffer(len(first)), len(first)) == -1
    assert L.dsb_format_identity(*args, C.create_string_buffer(len(first) + 1), len(first) + 1) == len(first)
    none = b"r2\t*\t*\t0\t0\t0\t0\t0\t0\t0.0000\t0\n"
    a2 = (idx.h, C.byref(reads[1]), C.byref(res.reads[1]), None, None)
    assert L.dsb_format_identity(*a2, C.create_string_buffer(len(none)), len(none)) == -1
    assert L.dsb_format_identity(*a2, C.create_string_buffer(len(none) + 1), len(none) + 1) == len(none)
    buf = C.create_string_buffer(4096)
    assert L.dsb_format_identity(None, args[1], args[2], args[3], args[4], buf, 4096) == -1
    assert L.dsb_format_identity(idx.h, None, args[2], args[3], args[4], buf, 4096) == -1
    assert L.dsb_format_identity(idx.h, args[1], None, args[3], args[4], buf, 4096) == -1
    assert L.dsb_format_identity(idx.h, args[1], args[2], None, args[4], buf, 4096) == -1
    assert L.dsb_format_identity(idx.h, args[1], args[2], args[3], None, buf, 4096) == -1
    idx.close()


def test_identity_table_format(demo):
    import desamba_amd as D
    idx = D.Index(demo["index"])
    tab = np.zeros(idx.n_ref, dtype=D.REF_IDENTITY_DTYPE)
    tab[0] = (2, 200, 210, 13, 1, 0); tab[2] = (0, 0, 0, 0, 0, 3); tab[462] = (1, 10, 20, 4, 0, 1)
    want = open(os.path.join(IDENT, "table.txt"), "rb").read()
    assert D.format_ref_identity(idx, tab) == want == M.table_text(idx, M.as_tuples(tab))
    head = want[:want.index(b"\n") + 1]
    assert D.format_ref_identity(idx, np.zeros(idx.n_ref, dtype=D.REF_IDENTITY_DTYPE)) == head
    L, C = D.lib(), D.C
    p = tab.ctypes.data_as(C.c_void_p)
    assert L.dsb_identity_format(idx.h, p, C.create_string_buffer(len(want)), len(want)) == -1
    assert L.dsb_identity_format(idx.h, p, C.create_string_buffer(len(want) + 1), len(want) + 1) == len(want)
    assert L.dsb_identity_format(None, p, C.create_string_buffer(4096), 4096) == -1
    assert L.dsb_identity_format(idx.h, None, C.create_string_buffer(4096), 4096) == -1
    with pytest.raises(ValueError):
        D.format_ref_identity(idx, tab[:5])
    idx.close()


def test_identity_null_handles_and_options(built):
    import desamba_amd as D
    L, C = D.lib(), D.C
    p = C.POINTER(D.DsbHitIdentity)()
    out = np.zeros(4, dtype=D.REF_IDENTITY_DTYPE)
    assert L.dsb_ctx_enable_identity(None, 1, 0, 0) == D.DSB_EINVAL and L.dsb_ctx_reset_identity(None) == D.DSB_EINVAL
    assert L.dsb_batch_identity(None, C.byref(p)) == D.DSB_EINVAL and L.dsb_ctx_identity(None, out.ctypes.data_as(C.c_void_p)) == D.DSB_EINVAL
    assert L.dsb_multi_enable_identity(None, 1, 0, 0) == D.DSB_EINVAL and L.dsb_multi_identity(None, C.byref(p)) == D.DSB_EINVAL
    assert L.dsb_multi_ref_identity(None, out.ctypes.data_as(C.c_void_p)) == D.DSB_EINVAL
    assert L.dsb_ctx_edit_pairs(None, None, None, None, None, None, None, 0, 256, 300, None) == D.DSB_EINVAL
    assert L.dsb_index_ref_bases(None, 0, 0, 0, None) == D.DSB_EINVAL
    for bad in (0, -0.1, 1.0001):
        with pytest.raises(ValueError):
            D.Ctx.enable_identity(None, True, 256, bad)                # (refused before the context is touched)
    assert (D.DSB_IDENT_EXACT, D.DSB_IDENT_OVER, D.DSB_IDENT_SKEW, D.DSB_IDENT_EMPTY) == (M.EXACT, M.OVER, M.SKEW, M.EMPTY)
    assert (D.DSB_IDENT_MAX_SKEW, D.DSB_IDENT_BAND_DEFAULT, D.DSB_IDENT_PERMILLE_DEFAULT) == (M.MAX_SKEW, M.BAND, M.PERMILLE)
    assert C.sizeof(D.DsbHitIdentity) == 16 == np.dtype(D.HIT_IDENTITY_DTYPE).itemsize and np.dtype(D.REF_IDENTITY_DTYPE).itemsize == 48


def fasta_records(path):
    name, seq, out = None, [], []
    for ln in open(path, "rb"):
        if ln.startswith(b">"):
            if name is not None:
                out.append((name, b"".join(seq)))
            name, seq = ln[1:].split()[0], []
        else:
            seq.append(ln.strip())
    out.append((name, b"".join(seq)))
    return out


def test_index_ref_bases(demo):
    import desamba_amd as D
    idx = D.Index(demo["index"])
    fa = fasta_records(os.path.join(demo["dir"], "viral-gs.fa"))
    assert len(fa) == idx.n_ref
    seen = set()
    for r in range(idx.n_ref):
        name, seq = fa[r]
        LN = idx.ref_len(r)
        assert name.decode() == idx.ref_name(r) and len(seq) == LN
        want = M.encode_ref(seq)                                   # (the index packs what is not ACGT as A; reads pack it as C)
        assert np.array_equal(idx.ref_bases(r, 0, LN), want), r
        seen |= set(seq.upper()) - set(b"ACGT")
        if r % 60 and r != idx.n_ref - 1:
            continue
        for st, n in ((0, 1), (1, 33), (3, 64), (LN - 70, 70), (LN - 1, 1), (LN, 0), (5, 0)):    # a window ending at LN among them
            assert np.array_equal(idx.ref_bases(r, st, n), want[st:st + n]), (r, st, n)
        for st, n in ((LN - 70, 71), (LN, 1), (LN + 1, 0), (0, LN + 1)):                          # beyond it
            with pytest.raises(D.DsbError) as e:
                idx.ref_bases(r, st, n)
            assert e.value.code == D.DSB_EINVAL
    assert seen                                                    # the demo references do hold other letters
    with pytest.raises(D.DsbError) as e:
        idx.ref_bases(idx.n_ref, 0, 1)
    assert e.value.code == D.DSB_EINVAL
    idx.close()


# ---------------------------------------------------------------- dsb_ctx_edit_pairs: the kernel's shapes

@pytest.fixture(scope="module")
def dev(demo):
    import desamba_amd as D
    idx = D.Index(demo["index"])
    ctx = D.Ctx(idx, 0)
    yield D, idx, ctx
    ctx.close(); idx.close()


def blobs(pairs, phases=None, seed=99):
    """the two code blobs of a list of pairs, random bases between them: pair p at word phase phases[p][0] of Q and byte phase
    phases[p][1] of T; without phases wherever the pairs before it end (every phase comes up)"""
    rng = np.random.default_rng(seed)
    q, t, qo, to = [], [], [], []
    nq = nt = 0
    for p, (Q, T) in enumerate(pairs):
        gq = int((phases[p][0] - nq) % 32) if phases else int(rng.integers(0, 3))
        gt = int((phases[p][1] - nt) % 4) if phases else int(rng.integers(0, 3))
        q += [rnd(rng, gq), Q]; t += [rnd(rng, gt), T]
        qo.append(nq + gq); to.append(nt + gt)
        nq += gq + len(Q); nt += gt + len(T)
    cat = lambda parts: np.concatenate(parts).astype(np.uint8) if parts else np.zeros(0, dtype=np.uint8)
    return cat(q), qo, [len(Q) for Q, T in pairs], cat(t), to, [len(T) for Q, T in pairs]


def check_pairs(ctx, pairs, B, pm, label, phases=None):
    got = M.as_tuples(ctx.edit_pairs(*blobs(pairs, phases), band=B, max_permille=pm))
    want = M.records_of(pairs, B, pm)
    assert len(got) == len(pairs)
    for p in range(len(pairs)):
        assert got[p] == want[p], (label, p, len(pairs[p][0]), len(pairs[p][1]), got[p], want[p])
    return want


@pytest.mark.gpu
def test_edit_pairs_sizes_crossed(dev):
    D, idx, ctx = dev
    rng = np.random.default_rng(1)
    pairs = []
    for n in SIZES:
        for m in SIZES:
            Q = rnd(rng, n)
            pairs.append((Q, fit(rng, noisy(rng, Q, 0.1), m)))
    for B, pm in ((256, 300), (3, 1000), (0, 1000), (8, 500)):
        want = check_pairs(ctx, pairs, B, pm, "sizes B=%d" % B)
    assert any(r[3] & M.OVER for r in want) and any(r[3] & M.EXACT for r in want)


@pytest.mark.gpu
def test_edit_pairs_all_start_phases(dev):
    D, idx, ctx = dev
    rng = np.random.default_rng(2)
    Q = rnd(rng, 70)
    T = noisy(rng, Q, 0.1)
    phases = [(qp, tp) for qp in range(32) for tp in range(4)]
    want = check_pairs(ctx, [(Q, T)] * len(phases), 16, 300, "phases", phases)
    assert len(set(want)) == 1 and want[0][0] > 0 and want[0][3] == M.EXACT


@pytest.mark.gpu
def test_edit_pairs_band_widths(dev):
    """|d| + 2B + 1 in {1, 63, 64, 65, 129}: one lane, a round not full, full, one diagonal into the second round, three rounds"""
    D, idx, ctx = dev
    rng = np.random.default_rng(3)
    for d, B in ((0, 0), (0, 31), (1, 31), (0, 32), (0, 64), (-1, 31), (3, 63)):
        pairs = []
        for k in range(6):
            Q = rnd(rng, 300)
            pairs.append((Q, fit(rng, noisy(rng, Q, 0.25), 300 + d)))
        want = check_pairs(ctx, pairs, B, 1000, "width %d" % (abs(d) + 2 * B + 1))
        assert all(not r[3] & M.BAD for r in want) and (B == 0 or any(r[0] > B for r in want))    # paths that use the whole band


@pytest.mark.gpu
def test_edit_pairs_indel_at_word_boundaries(dev):
    D, idx, ctx = dev
    rng = np.random.default_rng(4)
    pairs, phases = [], []
    for at in (31, 32, 33, 63, 64, 65):
        Q = rnd(rng, 200)
        dele = np.concatenate([Q[:at], Q[at + 1:]])
        ins = np.concatenate([Q[:at], [(Q[at] + 2) % 4], Q[at:]]).astype(np.uint8)
        pairs += [(Q, dele), (Q, ins), (dele, Q), (ins, Q)]
        phases += [(0, 0), (0, 0), (31, 3), (1, 1)]
    want = check_pairs(ctx, pairs, 8, 300, "indel", phases)
    assert all(r[0] == 1 and r[3] == M.EXACT for r in want)


@pytest.mark.gpu
def test_edit_pairs_hand_cases(dev):
    D, idx, ctx = dev
    for name, Q, T, B, pm, want in hand_cases():
        got = M.as_tuples(ctx.edit_pairs(*blobs([(Q, T)]), band=B, max_permille=pm))[0]
        assert got == M.record(Q, T, B, pm), name
        if want is not None:
            assert got == want, name
    assert len(ctx.edit_pairs([], [], [], [], [], [])) == 0
    L, C = D.lib(), D.C
    one = np.zeros(1, dtype=D.HIT_IDENTITY_DTYPE)
    q = np.zeros(4, dtype=np.uint8); o = np.zeros(1, dtype=np.uint64); n = np.full(1, 4, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for B, pm in ((1025, 300), (256, 0), (256, 1001)):
        assert L.dsb_ctx_edit_pairs(ctx.h, p(q), p(o), p(n), p(q), p(o), p(n), 1, B, pm, p(one)) == D.DSB_EINVAL
    wrap = np.full(1, 2 ** 64 - 2, dtype=np.uint64)                   # an offset whose sum with the length wraps
    assert L.dsb_ctx_edit_pairs(ctx.h, p(q), p(wrap), p(n), p(q), p(o), p(n), 1, 8, 300, p(one)) == D.DSB_EINVAL
    assert L.dsb_ctx_edit_pairs(ctx.h, p(q), p(o), p(n), p(q), p(wrap), p(n), 1, 8, 300, p(one)) == D.DSB_EINVAL
    assert L.dsb_ctx_edit_pairs(ctx.h, p(q), p(o), p(n), p(q), p(o), p(n), 1, 1024, 1000, p(one)) == 0 and tuple(one[0]) == (0, 4, 4, M.EXACT)


@pytest.mark.gpu
def test_edit_pairs_random(dev):
    """300 seeded pairs of up to 600 bases at 0 - 30 % errors, 60 for each band"""
    D, idx, ctx = dev
    rng = np.random.default_rng(5)
    for B in (0, 1, 8, 64, 256):
        pairs = []
        while len(pairs) < 60:
            Q = rnd(rng, int(rng.integers(1, 601)))
            T = noisy(rng, Q, 0.3 * rng.random())
            if len(T):
                pairs.append((Q, T))
        check_pairs(ctx, pairs, B, 300, "random B=%d" % B)


@pytest.mark.gpu
def test_edit_pairs_widest_band(dev):
    D, idx, ctx = dev
    rng = np.random.default_rng(6)
    Q = rnd(rng, 6000 - 4096)
    T = fit(rng, noisy(rng, Q, 0.05), 6000)
    want = check_pairs(ctx, [(Q, T), (T, Q)], 1024, 1000, "widest")
    assert want[0][1:3] == (1904, 6000) and want[0][0] >= 4096 and not want[0][3]


# ---------------------------------------------------------------- through classify

def decode(codes):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.asarray(codes, dtype=np.int64)].tobytes()


def check_batch(D, runner, idx, recs, res, B=M.BAND, pm=M.PERMILLE, label=""):
    """the records of a batch against the model over the batch's own hits; returns (model records, model table)"""
    want = M.records(idx, recs, res, B, pm)
    got = M.as_tuples(runner.identity(res.n_hits))
    assert len(got) == res.n_hits == len(want), label
    for h in range(res.n_hits):
        assert got[h] == want[h], (label, h, got[h], want[h])
    return want, M.table(idx, res, len(recs), want)


@pytest.mark.gpu
def test_convention_known_truth(built, tmp_path):
    """Exact 2-kbp substrings of three random references, half of them reverse-complemented, and the same reads with ONT errors: the
    strand and the coordinates of section 1 of the definition give ~1 and ~0.9; any other give two random sequences.  The errors
    come from test_abundance.mutate, the numpy restatement of tools/readsim's ont profile, not from the tool: readsim draws its own
    reads from an index and cannot put errors into given ones."""
    import desamba_amd as D
    from test_abundance import mutate, revcomp, write_fasta
    rng = np.random.default_rng(20261020)
    refs = [("tid|%d|ref%d" % (100 + r, r), rnd(rng, 20000)) for r in range(3)]
    write_fasta(str(tmp_path / "g.fa"), refs)
    D.build_index(str(tmp_path / "g.fa"), str(tmp_path / "index"))
    exact, sim = [], []
    for i in range(24):
        st = int(rng.integers(0, 18000))
        s = refs[i % 3][1][st:st + 2000]
        mu = mutate(rng, s, 0.08)
        if i % 2:
            s, mu = revcomp(s), revcomp(mu)
        exact.append(("exact_%d_%d" % (i, st), decode(s), b"5" * len(s))); sim.append(("ont_%d_%d" % (i, st), decode(mu), b"5" * len(mu)))
    recs = exact + sim
    idx = D.Index(str(tmp_path / "index"))
    ctx = D.Ctx(idx, 0)
    ctx.enable_identity()
    res = ctx.classify(D.make_reads(recs))
    ident = M.as_tuples(ctx.identity(res.n_hits))
    for i in range(len(recs)):
        rr = res.reads[i]
        assert rr.n >= 1, recs[i][0]
        h, r = res.hits[rr.first], ident[rr.first]
        print("%s: ref %d dir %d q %d..%d t %d..%d -> edits %d n %d m %d flags %d identity %.4f" % (recs[i][0], h.ref_ID, h.direction, h.q_st, h.q_ed, h.t_st, h.t_ed, *r, M.identity(r)))
        assert h.ref_ID == i % 24 % 3 and h.direction == (0 if i % 2 else 1)
        if i < 24:
            assert M.identity(r) >= 0.99 and not r[3] & M.OVER, recs[i][0]
        else:
            assert 0.80 <= M.identity(r) < 1, recs[i][0]
    check_batch(D, ctx, idx, recs, res, label="truth")
    ctx.close(); idx.close()


def demo_reads(D, demo, n=48):
    return D.read_fastq(demo["fastq"], n)


def pad_reach_read(idx):
    """the last 1500 bases of the last reference: the record ends on the last base of the reference text"""
    r = idx.n_ref - 1
    LN = idx.ref_len(r)
    return ("last_base", decode(idx.ref_bases(r, LN - 1500, 1500)), b"5" * 1500)


@pytest.mark.gpu
def test_classify_records_equal_the_model(dev, demo):
    D, idx, ctx0 = dev
    rng = np.random.default_rng(8)
    recs = demo_reads(D, demo) + [pad_reach_read(idx)] + [("junk%d" % i, decode(rnd(rng, 1200)), b"5" * 1200) for i in range(5)]   # (unclassified reads)
    ctx = D.Ctx(idx, 0)
    ctx.enable_identity()
    reads = D.make_reads(recs)
    res = ctx.classify(reads)
    want, tab = check_batch(D, ctx, idx, recs, res, label="demo")
    last = res.reads[48]
    assert last.n >= 1 and res.hits[last.first].ref_ID == idx.n_ref - 1 and res.hits[last.first].t_ed >= idx.ref_len(idx.n_ref - 1)
    assert want[last.first][0] <= 2 and want[last.first][3] == M.EXACT     # (an exact read: the interval's own offset by one is all)
    assert all(res.reads[i].n == 0 for i in range(49, 54)) and sum(1 for i in range(48) if res.reads[i].n) >= 30
    assert M.as_tuples(ctx.ref_identity()) == tab
    assert sum(r[0] for r in tab) >= 30 and sum(r[0] + r[5] for r in tab) == sum(1 for w in want if w != M.ZERO)
    assert D.format_identity(idx, reads, res, ctx.identity(res.n_hits)) == M.lines(idx, recs, res, want)
    assert D.format_ref_identity(idx, ctx.ref_identity()) == M.table_text(idx, tab)
    shares = {f: sum(1 for w in want if w[3] & f) for f in (M.EXACT, M.OVER, M.SKEW, M.EMPTY)}
    print("demo, defaults: %d records, flags %r, identities %s" % (sum(1 for w in want if w != M.ZERO), shares, " ".join("%.3f" % M.identity(w) for w in want if w != M.ZERO)[:400]))
    ctx.close()


@pytest.mark.gpu
def test_classify_records_equal_the_model_strain(strain):
    import desamba_amd as D
    idx = D.Index(strain["index"])
    recs = D.read_fastq(strain["fastq"])
    assert len(recs) == 96
    ctx = D.Ctx(idx, 0)
    ctx.enable_identity(band=64)
    res = ctx.classify(D.make_reads(recs), strict=False)
    want, tab = check_batch(D, ctx, idx, recs, res, 64, M.PERMILLE, "strain")
    assert M.as_tuples(ctx.ref_identity()) == tab and sum(r[0] for r in tab) >= 48
    ctx.close(); idx.close()


@pytest.mark.gpu
def test_identity_identical_across_batches_slots_contexts(dev, demo, monkeypatch):
    D, idx, ctx0 = dev
    recs = demo_reads(D, demo)
    hist = lambda s: max([len(x[1]) for x in recs[:s]], default=0)

    def per_read(runner, res, a, b):
        """the records of reads a .. b of the input, read by read (the hit buffer's order is the order the reads finished in)"""
        ident = M.as_tuples(runner.identity(res.n_hits))
        return [[ident[res.reads[i].first + k] for k in range(res.reads[i].n)] for i in range(b - a)]
    ctx = D.Ctx(idx, 0)
    ctx.enable_identity()
    res = ctx.classify(D.make_reads(recs))
    want, tab = check_batch(D, ctx, idx, recs, res, label="all")
    one = per_read(ctx, res, 0, len(recs))
    base = ctx.ref_identity().tobytes()
    assert ctx.ref_identity().tobytes() == base                       # fetching twice gives the same table
    for size in (1, 7):
        ctx.reset_identity()
        parts = []
        for a in range(0, len(recs), size):
            b = min(a + size, len(recs))
            ctx.set_history(hist(a))
            r = ctx.classify(D.make_reads(recs[a:b]))
            parts += per_read(ctx, r, a, b)
        assert parts == one and ctx.ref_identity().tobytes() == base, size
    # a repeated run on a fresh context
    ctx.close()
    ctx = D.Ctx(idx, 0)
    ctx.enable_identity()
    res = ctx.classify(D.make_reads(recs))
    assert per_read(ctx, res, 0, len(recs)) == one and ctx.ref_identity().tobytes() == base
    ctx.close()
    # two input slots, fetched between them
    ctx = D.Ctx(idx, 0, input_slots=2)
    ctx.enable_identity()
    parts = [D.make_reads(recs[:20]), D.make_reads(recs[20:])]
    ctx.select_slot(0); ctx.set_history(0); ctx.upload(parts[0])
    ctx.select_slot(1); ctx.set_history(hist(20)); ctx.upload(parts[1])
    ctx.select_slot(0); ctx.run(); r0 = ctx.fetch()
    first = per_read(ctx, r0, 0, 20)
    ctx.select_slot(1); ctx.run(); r1 = ctx.fetch()
    assert first + per_read(ctx, r1, 20, len(recs)) == one and ctx.ref_identity().tobytes() == base
    ctx.close()
    # two contexts on one device, several chunks on both
    monkeypatch.setenv("DSB_SHARD_CHUNK_READS", "5")
    m = D.Multi(idx, [0, 0])
    with pytest.raises(D.DsbError) as e:
        m.identity(0)
    assert e.value.code == D.DSB_EINVAL
    m.enable_identity()
    res = m.classify(D.make_reads(recs))
    assert min(m.last_calls()) > 0
    assert per_read(m, res, 0, len(recs)) == one and m.ref_identity().tobytes() == base
    assert D.format_identity(idx, D.make_reads(recs), res, m.identity(res.n_hits)) == M.lines(idx, recs, res, M.records(idx, recs, res))
    m.close()


def cli(tmp_path, files, extra=(), tag="run", env=None, index=None):
    out = tmp_path / (tag + ".out")
    e = dict(os.environ); e.update(env or {})
    p = subprocess.run([CLI, "classify"] + list(extra) + [index] + [str(f) for f in files] + ["-o", str(out)], stderr=subprocess.PIPE, env=e)
    assert p.returncode == 0, p.stderr
    return out.read_bytes()


@pytest.mark.gpu
def test_cli_identity_outputs_and_unchanged_sam(dev, demo, tmp_path):
    D, idx, ctx0 = dev
    recs = D.read_fastq(demo["fastq"], 60)
    fq = tmp_path / "head60.fq"
    with open(fq, "wb") as f:
        for n, s, q in recs:
            f.write(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n")
    e = {"DSB_CLI_BATCH_KB": "32"}                                      # several batches
    new = lambda tag: ["--identity", str(tmp_path / (tag + ".ident")), "--identity-refs", str(tmp_path / (tag + ".idrefs"))]
    golden = open(os.path.join(GOLDEN, "demo_head60.sam"), "rb").read()
    plain = cli(tmp_path, [fq], [], "plain", e, demo["index"])
    g0 = cli(tmp_path, [fq], new("g0"), "g0", e, demo["index"])
    g00 = cli(tmp_path, [fq], ["-g", "0,0"] + new("g00"), "g00", e, demo["index"])
    again = cli(tmp_path, [fq], new("again"), "again", e, demo["index"])
    assert plain == g0 == g00 == again and plain.splitlines()[:60] == golden.splitlines()    # the SAM does not know about the flags
    for ext in (".ident", ".idrefs"):
        assert (tmp_path / ("g0" + ext)).read_bytes() == (tmp_path / ("g00" + ext)).read_bytes() == (tmp_path / ("again" + ext)).read_bytes() != b"", ext
    des = cli(tmp_path, [fq], ["-f", "DES_FULL"], "des", e, demo["index"])
    des_i = cli(tmp_path, [fq], ["-f", "DES_FULL", "--identity-band", "16", "--identity-max-frac", "0.2", "-r", "0"] + new("des"), "desi", e, demo["index"])
    assert des == des_i
    # the two files are the library's texts of the library's numbers
    for tag, B, pm in (("g0", M.BAND, M.PERMILLE), ("des", 16, 200)):
        ctx = D.Ctx(idx, 0)
        ctx.enable_identity(band=B, max_frac=pm / 1000)
        reads = D.make_reads(recs)
        res = ctx.classify(reads)
        want, tab = check_batch(D, ctx, idx, recs, res, B, pm, tag)
        assert (tmp_path / (tag + ".ident")).read_bytes() == D.format_identity(idx, reads, res, ctx.identity(res.n_hits)) == M.lines(idx, recs, res, want)
        assert (tmp_path / (tag + ".idrefs")).read_bytes() == D.format_ref_identity(idx, ctx.ref_identity()) == M.table_text(idx, tab)
        ctx.close()
    assert (tmp_path / "g0.ident").read_bytes() != (tmp_path / "des.ident").read_bytes()
    # the options alone are refused
    p = subprocess.run([CLI, "classify", "--identity-band", "8", demo["index"], str(fq)], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"--identity-band" in p.stderr
    p = subprocess.run([CLI, "classify", "--identity-band", "1025", "--identity", str(tmp_path / "x"), demo["index"], str(fq)], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"--identity-band" in p.stderr


@pytest.mark.gpu
def test_identity_lifecycle(dev, demo):
    D, idx, ctx0 = dev
    L = D.lib()
    recs = demo_reads(D, demo, 24)
    ctx = D.Ctx(idx, 0)
    for call in (lambda: ctx.identity(0), ctx.ref_identity, ctx.reset_identity):     # off
        with pytest.raises(D.DsbError) as e:
            call()
        assert e.value.code == D.DSB_EINVAL
    for B, pm in ((1025, 300), (256, 1001), (5, 0)):
        assert L.dsb_ctx_enable_identity(ctx.h, 1, B, pm) == D.DSB_EINVAL
    ctx.classify(D.make_reads(recs))
    with pytest.raises(D.DsbError) as e:                                  # enabled after the batch ran: it has no records
        ctx.enable_identity(); ctx.identity(0)
    assert e.value.code == D.DSB_EINVAL
    assert L.dsb_ctx_enable_identity(ctx.h, 1, 0, 0) == 0                 # 0, 0: the defaults
    res = ctx.classify(D.make_reads(recs))
    want, tab = check_batch(D, ctx, idx, recs, res, label="defaults")
    assert M.as_tuples(ctx.ref_identity()) == tab
    res = ctx.classify(D.make_reads(recs))                               # the table adds up
    assert M.as_tuples(ctx.ref_identity()) == M.add_tables(tab, tab)
    ctx.reset_identity()
    assert not ctx.ref_identity().tobytes().strip(b"\0")
    ctx.enable_identity(band=0, max_frac=0.05)                           # on again with another band: other records, table zeroed
    assert not ctx.ref_identity().tobytes().strip(b"\0")
    res = ctx.classify(D.make_reads(recs))
    want0, tab0 = check_batch(D, ctx, idx, recs, res, 0, 50, "band 0")
    assert M.as_tuples(ctx.ref_identity()) == tab0 and want0 != want and any(w[3] & M.OVER for w in want0)
    ctx.enable_identity(False)
    for call in (lambda: ctx.identity(res.n_hits), ctx.ref_identity, ctx.reset_identity):
        with pytest.raises(D.DsbError) as e:
            call()
        assert e.value.code == D.DSB_EINVAL
    res2 = ctx.classify(D.make_reads(recs))                              # off: classify goes on as before
    assert res2.n_hits == res.n_hits
    # an empty batch
    ctx.enable_identity()
    r = ctx.classify(D.make_reads([]))
    assert r.n_hits == 0 and len(ctx.identity(0)) == 0
    ctx.close()


# one row per forced classify path (tests/test_lca.py's matrix): a launch placed too early would change these records.  The 4096
# random reads make the batch large enough for an early launch and have no hits, so the model has nothing to align for them.
@pytest.mark.gpu
@pytest.mark.parametrize("row", ["baseline", "hout_cap", "step_limit", "heavy_mw"])
def test_identity_on_every_classify_path(dev, demo, monkeypatch, row):
    D, idx, ctx0 = dev
    knobs = {"baseline": {}, "hout_cap": {"DSB_HOUT_CAP": "8"}, "step_limit": {"DSB_STEP_LIMIT_RT": "3000"},
             "heavy_mw": {"DSB_HEAVY_FIRST": "16", "DSB_HEAVY_MW": "8"}}[row]
    rng = np.random.default_rng(11)
    junk = [("junk%d" % i, decode(rnd(rng, 300)), b"5" * 300) for i in range(4096)]
    recs = D.read_fastq(os.path.join(SYNTH, "heavy.fq")) + junk[:2000] + D.read_fastq(os.path.join(SYNTH, "manyanchors.fq")) + demo_reads(D, demo, 32) + junk[2000:]
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    ctx = D.Ctx(idx, 0)
    ctx.enable_identity(band=64)
    res = ctx.classify(D.make_reads(recs))
    t = ctx.timing()
    if row == "baseline":
        assert t.n_regrow == 0 and t.n_early > 0
    elif row == "hout_cap":
        assert t.n_regrow > 0                                      # the run after a regrown hit buffer
    elif row == "step_limit":
        assert t.n_retry > 0                                       # the second run
    else:
        assert t.n_early == 16 and t.n_heavy_mw == 8               # the early launch
    want, tab = check_batch(D, ctx, idx, recs, res, 64, M.PERMILLE, row)
    assert M.as_tuples(ctx.ref_identity()) == tab and sum(r[0] + r[5] for r in tab) >= 20
    ctx.close()
