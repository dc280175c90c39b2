"""Checkpoint mode of the base-level alignment (k_hit_align_ck, k_pair_align_ck, dsb_ctx_align_pairs_mode, dsb_ctx_alignment_mode;
classify --cigar-checkpoint).  The operations of a record are always those of tests/align_lib.py with unlimited room;
tests/align_ck_lib.py restates the plan rule, which alone decides whether a record gets them, and the checkpointed walk itself."""
import os
import subprocess

import numpy as np
import pytest

import align_ck_lib as K
import align_lib as A
import identity_lib as M
from conftest import ROOT
from test_alignment import DEMO_PICK, check_batch, demo_batch, per_read
from test_identity import blobs, cli, demo_reads, noisy, rnd, subst

CLI = os.path.join(ROOT, "desamba_amd", "bin", "deSAMBA")
EDGES = [1, 29, 30, 31, 59, 60, 61, 62]                                 # around the segment edges of K = 30
# the plans the issue of this mode lists, computed there by hand from the rule
TABLE = [((200, 200, 8, 300, 1), (60, 0)), ((200, 200, 8, 310, 1), (30, 2)), ((300, 300, 8, 500, 1), (27, 5)), ((200, 200, 32, 310, 1), None),
         ((10, 4106, 1024, 1000, 2048), (674, 6)), ((50000, 50750, 256, 300, 2048), (3253, 4)), ((50000, 50750, 256, 300, 512), (795, 19)),
         ((50000, 50750, 256, 300, 256), None), ((2700, 2700, 64, 300, 12), (119, 6)), ((2700, 2800, 64, 300, 12), None)]
# the demo reads through classify: at band 64 and 16 KiB more than half of the counted records of the DEMO_PICK batch (24 of 42, worked
# out without the device from the oracle's hits) have edits x R above the room, and every aligned one has a plan; of the first 60 reads
# (the CLI test) 29 of 52, and every aligned one has a plan from 16 KiB on.  Both tests assert their share on the device's own records.
DEMO_BAND, DEMO_KIB = 64, 16


# ---------------------------------------------------------------- without a GPU

def test_plan_equals_the_model(built):
    import desamba_amd as D
    assert (D.DSB_ALN_MODE_FULL, D.DSB_ALN_MODE_CHECKPOINT) == (K.FULL, K.CHECKPOINT) == (0, 1)
    for args, want in TABLE:
        assert K.plan(*args) == want == D.aln_plan(*args), args
    ns = [1, 2, 63, 200, 999, 1000, 1001, 2700, 4096, 5000]
    seen = {"none": 0, "one pass": 0, "checkpoints": 0}
    for n in ns:
        ms = sorted(set(x for x in ns + [n - 4097, n - 4096, n - 100, n + 100, n + 4096, n + 4097] if 1 <= x))
        for m in ms:
            for B in (0, 8, 63, 64, 256, 1024):
                for pm in (1, 300, 1000):
                    for kib in (1, 2, 12, 2048):
                        want = K.plan(n, m, B, pm, kib)
                        assert D.aln_plan(n, m, B, pm, kib) == want, (n, m, B, pm, kib)
                        if want is None:
                            seen["none"] += 1
                            continue
                        cap, Rb, C, Mv, room = K.sizes(n, m, B, pm, kib)
                        k, n_ck = want
                        assert k >= 1 and Mv + k * Rb + n_ck * C <= room, (n, m, B, pm, kib, want)
                        assert n_ck == (0 if k >= cap else (cap - 1) // k)
                        seen["checkpoints" if n_ck else "one pass"] += 1
    assert min(seen.values()) > 100, seen
    L, C = D.lib(), D.C
    k, c = C.c_uint32(), C.c_uint32()
    for bad in ((1 << 28, 5, 8, 300, 1), (5, 1 << 28, 8, 300, 1), (5, 5, 1025, 300, 1), (5, 5, 8, 0, 1), (5, 5, 8, 1001, 1), (5, 5, 8, 300, 0), (5, 5, 8, 300, 65537)):
        assert L.dsb_aln_plan(*bad, C.byref(k), C.byref(c)) == D.DSB_EINVAL, bad
    assert L.dsb_aln_plan(5, 5, 8, 300, 1, None, C.byref(c)) == D.DSB_EINVAL and L.dsb_aln_plan(5, 5, 8, 300, 1, C.byref(k), None) == D.DSB_EINVAL
    assert L.dsb_ctx_alignment_mode(None, 1) == D.DSB_EINVAL and L.dsb_multi_alignment_mode(None, 1) == D.DSB_EINVAL
    n = C.c_uint64(0)
    assert L.dsb_ctx_align_pairs_mode(None, None, None, None, None, None, None, 0, 256, 300, 2048, 1, None, None, None, 0, C.byref(n)) == D.DSB_EINVAL


def random_small_pairs(count):
    rng = np.random.default_rng(20261021)
    for it in range(count):
        Q = rnd(rng, int(rng.integers(1, 121)))
        T = noisy(rng, Q, 0.5 * rng.random())
        if not len(T):
            T = np.zeros(1, dtype=np.uint8)
        yield it, Q, T, int(rng.integers(0, 65)), int(rng.integers(1, 3))


def test_checkpointed_walk_equals_the_definition():
    """300 pairs, n 1 .. 120, bands 0 .. 64, errors 0 .. 50 %: a walk that holds K generations of moves and every K-th generation's
    values gives align_lib.path's operations, for K = 1, 2, 3, 7 and the plan's own K at 1 and 2 KiB"""
    aligned = crossed = 0
    for it, Q, T, B, kib in random_small_pairs(300):
        cap = max(len(Q), len(T))
        edits, gens = A.generations(Q, T, B, cap)
        if edits is None:
            assert K.checkpointed_ops(Q, T, B, cap, 3) == (None, None)
            continue
        want = A.path(Q, T, B, edits, gens)
        own = K.plan(len(Q), len(T), B, 1000, kib)
        for k in (1, 2, 3, 7) + ((own[0],) if own else ()):
            assert K.checkpointed_ops(Q, T, B, cap, k) == (edits, want), (it, k)
            crossed += edits > k
        aligned += 1
    assert aligned > 250 and crossed > 800


def test_checkpointed_walk_needs_the_fill():
    """a restore that leaves cur as the later segment left it reads stale values beside the generation's ends: some pair must show it"""
    wrong = 0
    for it, Q, T, B, kib in random_small_pairs(40):
        cap = max(len(Q), len(T))
        edits, gens = A.generations(Q, T, B, cap)
        if edits is None or edits < 4:
            continue
        want = A.path(Q, T, B, edits, gens)
        try:
            wrong += K.checkpointed_ops(Q, T, B, cap, 2, fill=False) != (edits, want)
        except AssertionError:
            wrong += 1
    assert wrong > 0


def test_cli_cigar_checkpoint_option(built, demo, tmp_path):
    p = subprocess.run([CLI, "classify", "--cigar-checkpoint", demo["index"], demo["fastq"]], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"--cigar-checkpoint needs --cigar-sam FILE" in p.stderr
    p = subprocess.run([CLI, "classify"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    assert b"--cigar-sam FILE" in p.stderr and b"--cigar-trace-kib N" in p.stderr and b"--cigar-checkpoint" in p.stderr


# ---------------------------------------------------------------- dsb_ctx_align_pairs_mode: the kernel's shapes

@pytest.fixture(scope="module")
def dev(demo):
    import desamba_amd as D
    idx = D.Index(demo["index"])
    ctx = D.Ctx(idx, 0)
    yield D, idx, ctx
    ctx.close(); idx.close()


def check_ck(ctx, pairs, B, pm, kib, label, phases=None, want=None):
    """in checkpoint mode: records equal the model (align_lib's operations, NOTRACE by the plan alone), operations equal one for one in
    separate reserved ranges, identity records byte-identical to edit_pairs"""
    bl = blobs(pairs, phases)
    ident, aln, ops = ctx.align_pairs(*bl, band=B, max_permille=pm, trace_kib=kib, mode=K.CHECKPOINT)
    assert ident.tobytes() == ctx.edit_pairs(*bl, band=B, max_permille=pm).tobytes(), label
    want = want or [K.align_ck(Q, T, B, pm, kib) for Q, T in pairs]
    got_i = M.as_tuples(ident)
    assert len(got_i) == len(aln) == len(pairs)
    spans = []
    for p in range(len(pairs)):
        tag = (label, p, len(pairs[p][0]), len(pairs[p][1]))
        assert got_i[p] == want[p][0], tag + (got_i[p], want[p][0])
        assert A.as_tuple(aln[p]) == want[p][1], tag + (A.as_tuple(aln[p]), want[p][1])
        if want[p][1][4] & A.OPS:
            assert int(aln[p]["ops_off"]) + int(aln[p]["n_ops"]) <= len(ops), tag
            assert A.record_ops(aln, ops, p) == want[p][2], tag
            spans.append((int(aln[p]["ops_off"]), int(aln[p]["ops_off"]) + 2 * got_i[p][0] + 1))
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), label
    return want


def spaced(seed, n, edits, step):
    Q = rnd(np.random.default_rng(seed), n)
    return Q, subst(Q, [1 + step * k for k in range(edits)])


def mixed(seed, n, edits, indels):
    """`indels` bases of Q alone near the start, as many of T alone near the end, substitutions between them: the path runs on
    diagonal -indels through the middle, where the segment edges fall"""
    rng = np.random.default_rng(seed)
    Q = rnd(rng, n)
    a = min(edits // 3, indels)
    subs = edits - 2 * a
    gone = set(4 + 5 * j for j in range(a))
    more = set(n - 36 + 5 * j for j in range(a))
    step = max(2, (n - 90) // max(subs, 1))
    changed = set(45 + step * k for k in range(subs))
    T = []
    for i, b in enumerate(Q):
        if i in gone:
            continue
        T.append((int(b) + 1) % 4 if i in changed else int(b))
        if i in more:
            T.append((int(b) + 2) % 4)
    return Q, np.array(T, dtype=np.uint8)


def edge_pairs(B, pm, counts=EDGES):
    """per count of EDGES one pair of 200 x 200 bases from spaced substitutions and one from the mix, each with exactly that many
    edits by the model (the seed is searched: a construction can come out one edit cheaper than it was built)"""
    out = []
    for make in (lambda s, e: spaced(s, 200, e, 3), lambda s, e: mixed(s, 200, e, 6)):
        for e in counts:
            for seed in range(40):
                Q, T = make(1000 * e + seed, e)
                if len(T) == 200 and M.record(Q, T, B, pm)[0] == e:
                    out.append((Q, T))
                    break
            else:
                raise AssertionError("no pair with %d edits" % e)
    return out


def dense_pairs(B, pm, lo, hi):
    """200 x 200 pairs with more than lo and at most hi edits (every second base changed, and the mix on top)"""
    out = []
    for e in range(lo + 8, 100, 6):
        for Q, T in (spaced(77 + e, 200, e, 2), mixed(99 + e, 200, e, 6)):
            r = M.record(Q, T, B, pm)
            if len(T) == 200 and not r[3] & M.BAD and lo < r[0] <= hi:
                out.append((Q, T))
    return out


@pytest.mark.gpu
def test_ck_segment_edges(dev):
    """n = m = 200, band 8, 310 permille, 1 KiB: K = 30 with 2 checkpoints; pairs with exactly 1, 29, 30, 31, 59, 60, 61 and 62 edits.
    At 310 permille the cap is 62 edits, below the 64 generations that the full mode holds in 1 KiB at 16 bytes each (and in 2 KiB at
    32): no pair of that shape can show the contrast with the full mode, and at band 32 and 2 KiB the rule gives that shape one pass
    (62 x 32 = 2048 - 64).  Both are run as they are, and the contrast and the checkpoints inside a band still opening (K = 30 < 32)
    are shown at 500 permille, the same shapes with a cap of 100 edits: (200, 200, 8, 500, 1) is K = 28 with 3 checkpoints,
    (200, 200, 32, 500, 2) is K = 30 with 3."""
    D, idx, ctx = dev
    for B, kib, pm, plan in ((8, 1, 310, (30, 2)), (32, 2, 310, (62, 0)), (8, 1, 500, (28, 3)), (32, 2, 500, (30, 3))):
        assert K.plan(200, 200, B, pm, kib) == plan
        pairs = edge_pairs(B, pm)
        if pm == 500:
            pairs += dense_pairs(B, pm, 64, 100)
        want = check_ck(ctx, pairs, B, pm, kib, "edges B=%d pm=%d" % (B, pm))
        assert [w[0][0] for w in want[:16]] == EDGES * 2
        assert all(w[1][4] == A.OPS for w in want)
        assert all(w[1][2] >= 1 and w[1][3] >= 1 for w in want[8 + 3:16])                     # (the mix: both kinds of indel from 31 edits on)
        # the full mode in the same room: a path up to 64 generations and none above
        full = [A.align(Q, T, B, pm, kib) for Q, T in pairs]
        ident, aln, ops = ctx.align_pairs(*blobs(pairs), band=B, max_permille=pm, trace_kib=kib)
        assert [A.as_tuple(a) for a in aln] == [f[1] for f in full]
        assert all((f[1][4] == A.NOTRACE) == (f[0][0] * A.gen_bytes(200, 200, B) > kib * 1024) for f in full)
        if pm == 500:
            assert sum(1 for f in full if f[1][4] == A.NOTRACE) >= 6 and max(w[0][0] for w in want) > 3 * plan[0]


@pytest.mark.gpu
def test_ck_single_pass_plan(dev):
    D, idx, ctx = dev
    assert K.plan(200, 200, 8, 300, 1) == (60, 0)
    pairs = edge_pairs(8, 310)
    want = check_ck(ctx, pairs, 8, 300, 1, "one pass")
    assert [w[1][4] for w in want] == [A.OPS if e <= 60 else A.UNALIGNED for e in EDGES * 2]
    again = [K.align_ck(Q, T, 8, 310, 1) for Q, T in pairs]
    assert all(w == a for w, a, e in zip(want, again, EDGES * 2) if e <= 60)                  # the same results as with two checkpoints


@pytest.mark.gpu
def test_ck_no_plan(dev):
    D, idx, ctx = dev
    assert K.plan(200, 200, 32, 310, 1) is None
    pairs = edge_pairs(32, 310, [1, 30, 62])
    want = check_ck(ctx, pairs, 32, 310, 1, "no plan")
    assert all(w[1] == (0, 0, 0, 0, A.NOTRACE) for w in want) and [w[0][0] for w in want] == [1, 30, 62] * 2
    ident, aln, ops = ctx.align_pairs(*blobs(pairs), band=32, max_permille=310, trace_kib=1, mode=K.CHECKPOINT)
    assert len(ops) == 0
    # not nested: the full mode has a path for the record with one edit in the same room
    assert A.align(*pairs[0], 32, 310, 1)[1][4] == A.OPS


@pytest.mark.gpu
def test_ck_all_start_phases(dev):
    """the pair of test_align_pairs_all_start_phases at all 32 x 4 phases, band 16, 1000 permille, 1 KiB: K = 28 with 3 checkpoints.
    Its six edits end inside the first segment, so a second pair of the same size with more than 28 edits goes through the same
    phases: its walk restores the initial state"""
    D, idx, ctx = dev
    rng = np.random.default_rng(2)
    Q = rnd(rng, 100)
    T = np.concatenate([subst(Q[:30], [3, 17]), Q[31:60], [(Q[60] + 1) % 4], subst(Q[60:], [5, 30])]).astype(np.uint8)
    assert K.plan(100, 100, 16, 1000, 1) == (28, 3)
    phases = [(qp, tp) for qp in range(32) for tp in range(4)]
    one = K.align_ck(Q, T, 16, 1000, 1)
    assert one[0][0] == 6 and one[1][1:4] == (4, 1, 1)
    check_ck(ctx, [(Q, T)] * len(phases), 16, 1000, 1, "phases", phases, want=[one] * len(phases))
    Q2, T2 = mixed(3, 100, 40, 4)
    two = K.align_ck(Q2, T2, 16, 1000, 1)
    assert len(T2) == 100 and 28 < two[0][0] <= 56 and two[1][4] == A.OPS
    check_ck(ctx, [(Q2, T2)] * len(phases), 16, 1000, 1, "phases, two segments", phases, want=[two] * len(phases))


@pytest.mark.gpu
def test_ck_widest_band(dev):
    """(10, 4106), band 1024, 1000 permille, the default room: 97 rounds per generation, K = 674, 6 checkpoints; the full mode has no
    path there (test_align_pairs_widest_band)"""
    D, idx, ctx = dev
    rng = np.random.default_rng(9)
    Q = rnd(rng, 10)
    pair = (Q, rnd(rng, 4106))
    assert K.plan(10, 4106, 1024, 1000, A.TRACE_KIB) == (674, 6)
    want = check_ck(ctx, [pair], 1024, 1000, A.TRACE_KIB, "widest")[0]
    assert want[1][4] == A.OPS and want[0][0] >= 4096 and not A.has_path(10, 4106, 1024, want[0][0])
    ident, aln, ops = ctx.align_pairs(*blobs([pair]), band=1024, max_permille=1000)
    assert A.as_tuple(aln[0]) == (0, 0, 0, 0, A.NOTRACE)


@pytest.mark.gpu
def test_ck_long_and_skewed(dev):
    from test_abundance import mutate
    D, idx, ctx = dev
    rng = np.random.default_rng(11)
    Q = rnd(rng, 20000)
    T = mutate(rng, Q, 0.12)
    n, m = len(Q), len(T)
    plan = K.plan(n, m, 256, M.PERMILLE, 256)
    want = check_ck(ctx, [(Q, T)], 256, M.PERMILLE, 256, "20 kbp")[0]
    print("20 kbp: %d x %d, %d edits, plan %r, %d operations" % (n, m, want[0][0], plan, want[1][0]))
    assert plan is not None and plan[1] >= 3 and want[0][0] > 3 * plan[0] and abs(m - n) > 64
    assert want[1][4] == A.OPS and not A.has_path(n, m, 256, want[0][0], 256)
    ident, aln, ops = ctx.align_pairs(*blobs([(Q, T)]), band=256, max_permille=M.PERMILLE, trace_kib=256)
    assert A.as_tuple(aln[0]) == (0, 0, 0, 0, A.NOTRACE) and M.as_tuples(ident)[0] == want[0]
    # 100 random pairs, each in the smallest room that has a plan for it
    by_room = {}
    for p in range(100):
        Q = rnd(rng, int(rng.integers(200, 3001)))
        T = mutate(rng, Q, 0.04 + 0.1 * rng.random())
        kib = K.smallest_room(len(Q), len(T), M.BAND, M.PERMILLE)
        assert K.plan(len(Q), len(T), M.BAND, M.PERMILLE, kib) and (kib == 1 or K.plan(len(Q), len(T), M.BAND, M.PERMILLE, kib - 1) is None)
        by_room.setdefault(kib, []).append((Q, T))
    n_ck = 0
    for kib, pairs in sorted(by_room.items()):
        want = check_ck(ctx, pairs, M.BAND, M.PERMILLE, kib, "random, %d KiB" % kib)
        assert all(w[1][4] == A.OPS for w in want)
        n_ck += sum(1 for (Q, T), w in zip(pairs, want) if w[0][0] > K.plan(len(Q), len(T), M.BAND, M.PERMILLE, kib)[0])
    print("random: rooms %r KiB, %d of 100 walks cross a checkpoint" % (sorted(by_room), n_ck))
    assert n_ck >= 50


@pytest.mark.gpu
def test_ck_arguments(dev, demo):
    D, idx, ctx0 = dev
    Q, T = spaced(1, 50, 3, 7)
    with pytest.raises(D.DsbError) as e:
        ctx0.align_pairs(*blobs([(Q, T)]), band=8, max_permille=300, trace_kib=1, mode=2)
    assert e.value.code == D.DSB_EINVAL
    ctx = D.Ctx(idx, 0)
    L = D.lib()
    assert L.dsb_ctx_alignment_mode(ctx.h, K.CHECKPOINT) == D.DSB_EINVAL                       # identity and alignment are off
    ctx.enable_identity(band=DEMO_BAND)
    with pytest.raises(D.DsbError) as e:
        ctx.alignment_mode(K.CHECKPOINT)                                                      # before enable_alignment
    assert e.value.code == D.DSB_EINVAL
    ctx.enable_alignment(trace_kib=DEMO_KIB)
    assert L.dsb_ctx_alignment_mode(ctx.h, 2) == D.DSB_EINVAL
    ctx.alignment_mode(K.CHECKPOINT); ctx.alignment_mode(K.FULL); ctx.alignment_mode(K.CHECKPOINT)
    recs = demo_reads(D, demo, 12)
    reads = D.make_reads(recs)
    res = ctx.classify(reads)
    ck = check_batch(D, ctx, idx, recs, res, B=DEMO_BAND, label="mode on", model=False)
    ctx.enable_alignment(trace_kib=DEMO_KIB); ctx.reset_identity(); ctx.reset_history()       # enabled again: the mode is FULL
    res = ctx.classify(reads)
    full = check_batch(D, ctx, idx, recs, res, B=DEMO_BAND, trace_kib=DEMO_KIB, label="enabled again")   # (the model of the full mode)
    assert sum(1 for g in ck if g[1][4] == A.OPS) > sum(1 for g in full if g[1][4] == A.OPS) and any(g[1][4] == A.NOTRACE for g in full)
    ctx.enable_alignment(False)
    assert L.dsb_ctx_alignment_mode(ctx.h, K.CHECKPOINT) == D.DSB_EINVAL
    ctx.close()
    m = D.Multi(idx, [0, 0])
    m.enable_identity()
    with pytest.raises(D.DsbError) as e:
        m.alignment_mode(K.CHECKPOINT)
    assert e.value.code == D.DSB_EINVAL
    m.enable_alignment(trace_kib=DEMO_KIB)
    assert L.dsb_multi_alignment_mode(m.h, 2) == D.DSB_EINVAL
    m.alignment_mode(K.CHECKPOINT)
    m.close()


# ---------------------------------------------------------------- through classify

@pytest.mark.gpu
def test_ck_demo_reads_equal_the_full_mode(dev, demo, monkeypatch):
    """the DEMO_PICK batch at band 64: in 16 KiB the full mode leaves more than half of the counted records without a path, the
    checkpoint mode none of the aligned ones, and their operations are those of the full mode at the default room -- through a
    context in one batch and in batches of seven, and through two contexts in chunks of five"""
    D, idx, ctx0 = dev
    recs = demo_batch(D, idx, demo)
    n = len(recs)
    reads = D.make_reads(recs)
    hist = lambda s: max([len(x[1]) for x in recs[:s]], default=0)
    by_read = lambda r, ident: [[ident[r.reads[i].first + k] for k in range(r.reads[i].n)] for i in range(n)]
    ctx = D.Ctx(idx, 0)
    ctx.enable_identity(band=DEMO_BAND); ctx.enable_alignment()
    res = ctx.classify(reads)
    ref = per_read(res, check_batch(D, ctx, idx, recs, res, B=DEMO_BAND, label="full, default room", model=False), n)
    sam0 = ctx.sam(res); ident0 = by_read(res, M.as_tuples(ctx.identity(res.n_hits))); tab0 = ctx.ref_identity().tobytes()
    counted = [g for r in ref for g in r if g[1] != A.NO_ALN]
    aligned = [g for g in counted if not g[0][3] & M.BAD]
    assert len(counted) >= 40 and all(g[1][4] == A.OPS for g in aligned)
    # the two conditions, by the model, on the device's own records
    short = sum(1 for g in aligned if not A.has_path(g[0][1], g[0][2], DEMO_BAND, g[0][0], DEMO_KIB))
    print("demo, band %d, %d KiB: %d counted, %d aligned, %d without a path in full mode" % (DEMO_BAND, DEMO_KIB, len(counted), len(aligned), short))
    assert 2 * short >= len(counted)
    assert all(K.plan(g[0][1], g[0][2], DEMO_BAND, M.PERMILLE, DEMO_KIB) is not None for g in aligned)
    assert any(g[0][0] > K.plan(g[0][1], g[0][2], DEMO_BAND, M.PERMILLE, DEMO_KIB)[0] for g in aligned)      # (walks that cross a checkpoint)
    ctx.enable_alignment(trace_kib=DEMO_KIB); ctx.reset_identity(); ctx.reset_history()
    res = ctx.classify(reads)
    full = check_batch(D, ctx, idx, recs, res, B=DEMO_BAND, label="full, small room", model=False)
    assert sum(1 for g in full if g[1][4] == A.NOTRACE) == short
    ctx.alignment_mode(K.CHECKPOINT); ctx.reset_identity(); ctx.reset_history()
    res = ctx.classify(reads)
    assert per_read(res, check_batch(D, ctx, idx, recs, res, B=DEMO_BAND, label="checkpoint", model=False), n) == ref
    assert ctx.sam(res) == sam0 and by_read(res, M.as_tuples(ctx.identity(res.n_hits))) == ident0 and ctx.ref_identity().tobytes() == tab0
    parts = []
    for a in range(0, n, 7):
        b = min(a + 7, n)
        ctx.set_history(hist(a))
        r = ctx.classify(D.make_reads(recs[a:b]))
        parts += per_read(r, check_batch(D, ctx, idx, recs[a:b], r, B=DEMO_BAND, label="7", model=False), b - a)
    assert parts == ref
    ctx.close()
    monkeypatch.setenv("DSB_SHARD_CHUNK_READS", "5")
    m = D.Multi(idx, [0, 0])
    m.enable_identity(band=DEMO_BAND); m.enable_alignment(trace_kib=DEMO_KIB); m.alignment_mode(K.CHECKPOINT)
    res = m.classify(reads)
    assert min(m.last_calls()) > 0
    assert per_read(res, check_batch(D, m, idx, recs, res, B=DEMO_BAND, label="multi", model=False), n) == ref
    m.close()


@pytest.mark.gpu
def test_cli_cigar_checkpoint(dev, demo, tmp_path):
    D, idx, ctx0 = dev
    recs = D.read_fastq(demo["fastq"], 60)
    fq = tmp_path / "head60.fq"
    with open(fq, "wb") as f:
        for n, s, q in recs:
            f.write(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n")
    e = {"DSB_CLI_BATCH_KB": "32"}                                      # several batches
    band = ["--identity-band", str(DEMO_BAND)]
    small = ["--cigar-trace-kib", str(DEMO_KIB)]
    a = cli(tmp_path, [fq], band + ["--cigar-sam", str(tmp_path / "a.sam")] + small + ["--cigar-checkpoint"], "a", e, demo["index"])
    b = cli(tmp_path, [fq], band + ["--cigar-sam", str(tmp_path / "b.sam")], "b", e, demo["index"])
    c = cli(tmp_path, [fq], band + ["--cigar-sam", str(tmp_path / "c.sam")] + small, "c", e, demo["index"])
    ta, tb, tc = ((tmp_path / (x + ".sam")).read_bytes() for x in "abc")
    assert a == b == c and ta == tb
    # the condition: in that room the full mode leaves records without a path, and no aligned record is without a plan
    lines = lambda t: [ln for ln in t.split(b"\n") if ln and not ln.startswith(b"@")]
    notrace = sum(1 for ln in lines(tc) if b"\txa:i:%d\t" % A.NOTRACE in ln)
    assert notrace >= 10 and not any(b"\txa:i:%d\t" % A.NOTRACE in ln for ln in lines(ta)) and A.check_sam(idx, ta) >= 30
