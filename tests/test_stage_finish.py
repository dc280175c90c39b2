"""a-13 behind get_score_M2, a-14 and a-17 on their own: the cut at the head of delete_small_score_rst and its part behind get_score_M2 (sort by
position, absorb and merge, the three score filters, sort by score, cut), detect_primary, and glibc_sort_chains with each of the three
comparators (dsb_classify_dev.h), called on arrays of chains (tests/stage/dsb_stage_forms.h: stage_finish) and compared field by field
with the oracle (oracle/classify.c: ora_finish_stage, ora_sort_stage).  detect_primary, glibc_sort_chains<W> and the head cut (small_score_head_cut) are called as they are;
the tail of delete_small_score_rst is replayed statement by statement by stage_small_score_tail (DESIGN.md says why), so a change of the
tail's own text in the product is not seen here.  Three legs: the 1-lane emulation, the 64-lane emulation with the race detector (both
lane orders, no finding), the GPU.

Domain: detect_primary keeps its primaries in two lists that it caps at 750 entries (`if (n_primary_v > 750) n_primary_v = 750`, so the highest
index written is 750): primary_v, ints in score_v, which has 1024 ints in every arena (arena_layout, the emulation, the stage slice), and
primary_v_idx, bytes in the idle reference window win_mid (DSB_REFWIN = 2176 bytes; the reference has 800 of each).  751 entries fit both.
In the product at most 400 chains reach it (the head cut), and this test feeds it through that cut, so more than 400 primaries, let alone
750 supplementaries, cannot occur and are not generated.  Thresholds as the command line sets
them (min length 170, min score 64, LV3 74).  read_len 200 .. 2^20, q_st <= q_ed except for the wrapped q_st the left extension can leave
(above 4294960000, which detect_primary resets).

Classes asserted from the inputs and the oracle's output: 0, 1, 2, 199-201, 399-401 chains; sum_score 50 / 51 at index 200; the filter regimes
(max_read_l 509 / 510, read length 309 / 310, LV3 with a short and with a weak chain); absorbed and merged chains, a zeroed chain between two
merged ones; equal odd and equal even sum_score in runs of 2 .. 9, 16, 17 and 400 for comparator 2; secondaries with an overlap of exactly
half and one base less, on the opposite strand, more than 255 secondaries of one primary, sum_score + max_gap at the bound, a wrapped q_st."""
import random
import time

import numpy as np
import pytest

import stage_chain_lib as S

SEED = 13
MINLEN, MINSC, LV3 = 170, 64, 74


@pytest.fixture(scope="module")
def ora(built):
    o = S.Oracle2()
    yield o
    o.close()


def random_chains(rng, n, L, refs=6, zero=0.1):
    out = np.zeros(n, S.CH)
    t0 = [rng.randint(0, 1 << 20) for _ in range(refs)]
    for i in range(n):
        ref = rng.randrange(refs)
        ql = rng.choice([20, 100, 169, 170, 171, 400, 1500])
        q = rng.randint(0, max(0, L - ql))
        t = t0[ref] + rng.choice([0, 4, 5, 6, 300, 980, 1300, 5000]) * rng.randint(0, 3) + rng.randint(0, 40)
        sc = 0 if rng.random() < zero else rng.choice([20, 24, 25, 26, 29, 30, 50, 51, 62, 63, 64, 72, 73, 74, 75, 100, 101, 300, 301, 302, 2000])
        out[i] = S.chain(ref, rng.randint(0, 1), t, t + ql + rng.randint(-3, 3), q, q + ql, sc, rng.randint(1, 9), rng.randint(-5, 5), rng.randint(0, 1), i)
    return out


def build_cases(seed, per=52):
    """-> list of (chains, read_len, max_read_l, tag)"""
    rng = random.Random(seed)
    cases = []
    for rep in range(per):
        for n in (0, 1, 2, 199, 200, 201, 399, 400, 401):
            L = rng.choice([250, 309, 310, 509, 510, 3000, 1 << 20])
            ch = random_chains(rng, n, L, zero=0.0 if n >= 199 else 0.1)
            if n > 200:
                ch["sum_score"][:200] = 300; ch["sum_score"][200] = rng.choice([50, 51]); ch["sum_score"][201:] = rng.choice([49, 51, 60])
            cases.append((ch, L, rng.choice([0, 509, 510, 9000]), "n=%d" % n))
        # filter regimes: one strong chain and chains at the thresholds, on references of their own (nothing merges)
        for (mrl, L) in ((0, 509), (0, 510), (600, 309), (600, 310), (0, 5000)):
            ch = np.zeros(8, S.CH)
            for i, (sc, ql) in enumerate([(500, 400), (25 - (60 >> 5), 60), (26 - (60 >> 5), 60), (29 - 1, 60), (30 - 1, 60), (73 - 5, 169), (73 - 5, 170), (63 - 5, 171)]):
                ch[i] = S.chain(10 + i, rng.randint(0, 1), 1000 * i, 1000 * i + ql, 5 * i, 5 * i + ql, sc, 3, 0, 1, i)
            cases.append((ch[rng.sample(range(8), 8)], L, mrl, "regime"))
        # absorb and merge at each bound, a zeroed chain in between
        for (dt, dq, ds) in ((4, 4, 4), (5, 4, 4), (4, 5, 4), (4, 4, 5)):
            a = S.chain(3, 1, 5000, 5400, 100, 500, 300, 4, 0, 1, 0); b = S.chain(3, 1, 5000 + dt, 5300, 100 + dq, 400, 300 + ds, 4, 0, 1, 1)
            cases.append((np.array([b, a] if rng.random() < 0.5 else [a, b]), 3000, 9000, "absorb"))
        for (gt, gq) in ((-20, 0), (-19, 0), (999, 999), (1000, 999), (999, 1000), (0, -20), (0, -19), (500, 301), (500, 300), (301, 500)):
            a = S.chain(4, 0, 8000, 8400, 1000, 1400, 300, 4, 0, 1, 0); z = S.chain(4, 0, 8100, 8200, 50, 150, 0, 1, 0, 1, 1)
            b = S.chain(4, 0, 8400 + gt, 8900 + gt, 1400 + gq, 1900 + gq, 200, 4, 0, 1, 2); o = S.chain(4, 1, 8400, 8900, 1400, 1900, 200, 4, 0, 1, 3)
            cases.append((np.array([a, z, o, b])[rng.sample(range(4), 4)], 5000, 9000, "merge"))
        # detect_primary: a primary and secondaries at the bounds; many secondaries; a wrapped q_st
        L = 4000
        p = S.chain(1, 1, 0, 1000, 1000, 2000, 6400 + rng.choice([0, 64]), 9, 0, 1, 0)
        sec = [S.chain(20 + j, 1, 0, ln, 2000 - ln // 2 - d, 2000 - ln // 2 - d + ln, 900, 5, 0, 1, 1 + j) for j, (ln, d) in enumerate(((400, 0), (400, -1), (401, 0), (401, -1)))]
        opp = [S.chain(30, 0, 0, 400, L - 2000 + 100, L - 2000 + 500, 800, 5, 0, 1, 6), S.chain(31, 0, 0, 400, 1100, 1500, 700, 5, 0, 1, 7)]
        mg = p["sum_score"] >> 6
        gap = [S.chain(40 + j, 1, 0, 400, 1200, 1600, int(p["sum_score"]) - int(mg) + d, 5, 0, 1, 8 + j) for j, d in enumerate((-1, 0, 1))]
        wrap = [S.chain(50, 1, 5, 300, 4294960001 + rng.randint(0, 7000), 280, 650, 5, 0, 1, 11), S.chain(51, 1, 5, 300, 4294960000, 2600, 640, 5, 0, 1, 12)]
        cases.append((np.array([p] + sec + opp + gap + wrap), L, 9000, "primary"))
        many = [S.chain(100 + j, j & 1, 0, 300, 1100 + (j % 5), 1400 + (j % 5), 5000 - j, 5, 0, 1, j) if j & 1 == 1 else
                S.chain(100 + j, 0, 0, 300, L - 1400 - (j % 5), L - 1100 - (j % 5), 5000 - j, 5, 0, 1, j) for j in range(1, 300)]
        cases.append((np.array([p] + many), L, 9000, "many secondaries"))
    return cases


def sort_cases(seed):
    """-> list of (chains, which): for comparator 2 runs of equal odd and equal even sum_score in 2 .. 9, 16, 17 and 400 chains"""
    rng = random.Random(seed)
    out = []
    for rep in range(52):
        for n in (2, 3, 4, 5, 6, 7, 8, 9, 16, 17) + (400,):
            for parity in (0, 1):
                extra = rng.choice([0, 0, 1, 3]) if n < 400 else 0           # the run alone, or inside a list of other scores
                ch = random_chains(rng, n + extra, 3000)
                ch["sum_score"] = 100 + parity
                for j in rng.sample(range(n + extra), extra):
                    ch["sum_score"][j] = rng.choice([98, 99, 102, 103]) + 4 * j
                out.append((ch, 2))
        for which in (0, 1):
            out.append((random_chains(rng, rng.choice([0, 1, 2, 3, 17, 64, 400]), 3000, refs=3), which))
    return out


@pytest.fixture(scope="module")
def sets(ora):
    t = time.time()
    fin = build_cases(SEED)
    exp = [ora.finish(ch, L, mrl, MINLEN, MINSC, LV3) for ch, L, mrl, _ in fin]
    srt = sort_cases(SEED + 1)
    sexp = [ora.sort(ch, w) for ch, w in srt]
    print("stage a-13/a-14/a-17: %d finish cases, %d sort cases generated in %.1f s" % (len(fin), len(srt), time.time() - t))
    return fin, exp, srt, sexp


def classes(fin, exp, srt):
    cls = {}

    def put(name, i):
        cls.setdefault(name, set()).add(i)
    for i, ((ch, L, mrl, tag), e) in enumerate(zip(fin, exp)):
        put("n=%d" % len(ch), i)
        if len(ch) > 200:
            put("score at 200: %d" % int(ch["sum_score"][200]), i)
        m = max(mrl, L)
        if e["n_cut"]:
            put("regime:" + ("max_read_l %d" % m if m in (509, 510) else "read %d" % L if (m >= 510 and L in (309, 310)) else "LV3" if (m >= 510 and L >= 310) else "other"), i)
        T, P = e["tail"], e["chains"]
        nh = e["n_hit"]
        if tag in ("absorb", "merge"):
            put("%s: %d left" % (tag, nh), i)
        if tag == "merge" and nh == 2 and (T["sum_score"] == 500).any():
            put("merged over a zeroed chain", i)
        if nh > 1:
            p0 = P[0]
            for c in P[1:nh]:
                if c["primary"] != 2:
                    continue
                same = c["direction"] == p0["direction"]
                ps, pe = (int(p0["q_st"]), int(p0["q_ed"])) if same else (L - int(p0["q_ed"]), L - int(p0["q_st"]))
                ov = min(int(c["q_ed"]), pe) - max(int(c["q_st"]), ps); ln = int(c["q_ed"]) - int(c["q_st"])
                if 2 * ov == ln:
                    put("overlap exactly half", i)
                if not same:
                    put("secondary on the opposite strand", i)
                if int(c["sum_score"]) + max(int(p0["sum_score"]) >> 6, 5) == int(p0["sum_score"]):
                    put("sum_score + max_gap at the bound", i)
            for c in P[1:nh]:                  # (the first primary is asked first: a chain it overlaps by less than half is left to the later ones)
                ov = min(int(c["q_ed"]), int(p0["q_ed"])) - max(int(c["q_st"]), int(p0["q_st"])); ln = int(c["q_ed"]) - int(c["q_st"])
                if c["direction"] == p0["direction"] and ov > 0 and 2 * ov in (ln - 1, ln - 2):
                    put("overlap one base less than half", i)
            if (P["primary"][:nh] == 2).sum() > 255:
                put("more than 255 secondaries", i)
        if (ch["q_st"] > 4294960000).any() and nh and (T["q_st"][:nh] > 4294960000).any():
            put("wrapped q_st", i)
    for i, (ch, w) in enumerate(srt):
        if w == 2:
            u, cnt = np.unique(ch["sum_score"], return_counts=True)
            v = int(u[cnt.argmax()])
            put("sort 2: %s run of %d" % ("odd" if v & 1 else "even", int(cnt.max())) + ("" if len(u) == 1 else " among others"), ("s", i))
    return cls


NAMES = ["n=%d" % n for n in (0, 1, 2, 199, 200, 201, 399, 400, 401)] + ["score at 200: 50", "score at 200: 51", "regime:max_read_l 509", "regime:max_read_l 510", "regime:read 309",
         "regime:read 310", "regime:LV3", "absorb: 1 left", "absorb: 2 left", "merge: 2 left", "merge: 3 left", "merged over a zeroed chain", "overlap exactly half",
         "overlap one base less than half", "secondary on the opposite strand", "sum_score + max_gap at the bound", "more than 255 secondaries", "wrapped q_st"]
SORT_NAMES = ["sort 2: %s run of %d" % (p, n) for p in ("odd", "even") for n in (2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 400)]


def test_coverage(sets):
    fin, exp, srt, _ = sets
    cls = classes(fin, exp, srt)
    print({n: len(cls.get(n, ())) for n in NAMES + SORT_NAMES})
    for n in NAMES:
        assert len(cls.get(n, ())) >= 50, (n, len(cls.get(n, ())))
    for n in SORT_NAMES:
        assert len(cls.get(n, ())) + len(cls.get(n + " among others", ())) >= 50, n
    # the filters' verdicts at the thresholds, from the oracle's tail: a chain whose s = sum_score + (length >> 5) is one below the bound goes, at the bound stays
    for (ch, L, mrl, tag), e in zip(fin, exp):
        if tag == "regime":
            kept = set(int(r) for r in e["tail"]["ref_ID"][:e["n_hit"]])
            m = max(mrl, L)
            want = {10} | ({12, 13, 14, 15, 16, 17} if m < 510 else {14, 15, 16, 17} if L < 310 else {16})
            assert kept == want, (L, mrl, kept, want)


def check(leg, fin, exp, srt, sexp, idx=None, sidx=None):
    idx = range(len(fin)) if idx is None else idx
    sidx = range(len(srt)) if sidx is None else sidx
    cs = np.zeros(len(idx) + len(sidx), S.FIN); blobs = []; off = 0
    for j, i in enumerate(idx):
        ch, L, mrl, _ = fin[i]
        cs[j] = (off, len(ch), L, 0, mrl, MINLEN, MINSC, LV3, 0, 0, 0, 0); blobs.append(ch); off += len(ch)
    for j, i in enumerate(sidx):
        ch, w = srt[i]
        cs[len(idx) + j] = (off, len(ch), 0, w + 1, 0, MINLEN, MINSC, LV3, 0, 0, 0, 0); blobs.append(ch); off += len(ch)
    chains = np.concatenate(blobs + [np.zeros(1, S.CH)])[:off] if off else np.zeros(0, S.CH)
    out, got, tail = leg.finish(cs, np.ascontiguousarray(chains))
    assert not out["status"].any()
    for j, i in enumerate(idx):
        e = exp[i]; c = out[j]; o = int(c["c0"]); n = e["n_cut"]
        assert (int(c["n_cut"]), int(c["n_hit"]), int(c["max_read_l_out"])) == (n, e["n_hit"], e["max_read_l"]), (i, fin[i][3], c, e["n_cut"], e["n_hit"], e["max_read_l"])
        assert tail[o:o + n].tobytes() == e["tail"].tobytes(), ("chains behind the tail", i, fin[i][3])
        assert got[o:o + n].tobytes() == e["chains"].tobytes(), ("chains behind detect_primary", i, fin[i][3])
        assert got[o + n:o + len(fin[i][0])].tobytes() == fin[i][0][n:].tobytes(), ("chains behind the cut are untouched", i)
    for j, i in enumerate(sidx):
        c = out[len(idx) + j]; o = int(c["c0"]); n = len(srt[i][0])
        assert got[o:o + n].tobytes() == sexp[i].tobytes(), ("glibc_sort_chains<%d>" % srt[i][1], i, n)


def test_one_lane_emulation(sets):
    t = time.time()
    check(S.emu1(), *sets)
    print("1-lane emulation, a-13/a-14/a-17: %.1f s" % (time.time() - t))


@pytest.mark.parametrize("order", ["fwd", "rev"])
def test_64_lane_emulation(sets, order, monkeypatch):
    if order == "rev":
        monkeypatch.setenv("DSB_EMU_ORDER", "rev")
    fin, exp, srt, sexp = sets
    cls = classes(fin, exp, srt)
    idx, sidx = set(), set()
    for n in NAMES + SORT_NAMES:
        both = set(cls.get(n, ())) | (set(cls.get(n + " among others", ())) if n in SORT_NAMES else set())
        m = sorted(both, key=lambda v: (len(srt[v[1]][0]) if isinstance(v, tuple) else len(fin[v][0]), str(v)))[:5]
        assert len(m) >= 5, n
        for v in m:
            (sidx if isinstance(v, tuple) else idx).add(v[1] if isinstance(v, tuple) else v)
    sidx |= {i for i, (ch, w) in enumerate(srt) if w != 2 and i < 40}
    leg = S.emu64()
    t = time.time()
    leg.findings()
    check(leg, fin, exp, srt, sexp, sorted(idx), sorted(sidx))
    f = leg.findings()
    assert not f, f
    print("64-lane emulation (%s), a-13/a-14/a-17: %d + %d cases, %.1f s" % (order, len(idx), len(sidx), time.time() - t))


@pytest.mark.gpu
def test_device(sets):
    t = time.time()
    check(S.device(), *sets)
    print("device, a-13/a-14/a-17: %.1f s" % (time.time() - t))
