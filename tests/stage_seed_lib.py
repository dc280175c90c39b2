"""The front of the pipe on the host, for tests/test_stage_seed.py: a-1 encode / pack, a-2 the low-complexity filter and a-3 the two table
probes in plain numpy (one window per element), the class counters of the seed scan, a plain model of what k_seed_scan's look-ahead asks
for, the cases, and the ctypes binding of the emulation's stage entries.  The expected seed list of a strand is always
oracle_lib.seed_stage(hit bytes): the oracle's own scan and marking.  TEST ONLY."""
import ctypes as C
import os

import numpy as np

import oracle_lib
from emu_lib import EMU_SO, EmuSeed

U64 = np.uint64
FILLS = (0.15, 0.45, 0.7, 0.87, 0.95, 0.985)          # a hit needs both tables: about 2, 20, 49, 76, 90 and 97 % of the windows hit
# table bytes -> (mask bits, k): set_ekmer_par's sizes as dsb_ctx_use_synthetic_filter takes them
TABLES = {1 << 27: (30, 16), 1 << 28: (31, 17), 1 << 30: (33, 18), 1 << 32: (35, 19), 1 << 34: (37, 20)}
TABLE_OF_K = {16: 1 << 27, 17: 1 << 28, 18: 1 << 30, 19: 1 << 32, 20: 1 << 34}
DEVICE_FILLS = {16: FILLS, 17: (0.45, 0.95), 18: (0.45, 0.95), 19: (0.7,), 20: (0.7,)}
LOOKS = {"default": (4, 2, 4, 4), "dense": (4, 2, 4, 3), "round3": (8, 6, 8, 8), "one": (1, 0, 1, 1), "wide_stride1": (8, 6, 8, 1), "narrow_stride8": (1, 6, 1, 8)}
CPU_MASK_BITS = 22                                    # the CPU legs' tables: 2^22 bits each under the synthetic rule (the scan does not care how wide the mask is)

_CODE = np.full(256, 1, dtype=np.uint8)
for _c, _v in ((b"Aa", 0), (b"Gg", 2), (b"Tt", 3)):
    for _b in _c:
        _CODE[_b] = _v


# ---- a-1: CLY_Bit codes, the reverse strand, packed words -------------------------------------------------------------------
def codes(seq, strand=1):
    """2-bit codes of a strand (1 = forward, 0 = reverse): A/a 0, G/g 2, T/t 3, everything else 1 (src/cly.c:17-35)"""
    b = _CODE[np.frombuffer(bytes(seq), dtype=np.uint8)]
    return b if strand else (3 - b[::-1]).astype(np.uint8)


def pack(seq):
    """k_encode_pack's layout: (L + 31) // 32 + 1 words per strand, 32 bases per word, first base in the top bits, zeros behind the strand;
    the forward strand's words first"""
    L = len(seq); nw = (L + 31) // 32 + 1
    out = np.zeros(2 * nw, dtype=U64)
    for s, strand in enumerate((1, 0)):
        b = np.zeros(nw * 32, dtype=U64); b[:L] = codes(seq, strand)
        b = b.reshape(nw, 32)
        v = np.zeros(nw, dtype=U64)
        for j in range(32):
            v = (v << U64(2)) | b[:, j]
        out[s * nw:(s + 1) * nw] = v
    return out


# ---- a-2: k-mers and store_kmers' filter ------------------------------------------------------------------------------------
def kmers(b, k):
    """the k-mer of every window of a strand's codes (first base in the high bits)"""
    n = len(b) - k + 1
    v = np.zeros(max(n, 0), dtype=U64)
    for j in range(k):
        v = (v << U64(2)) | b[j:j + n].astype(U64)
    return v


def filter_ok(b, k):
    """store_kmers (src/cly.c:360-398): a window is dropped when one base fills >= int(0.8 k) of it, and the k-mer 0 never hits"""
    n = len(b) - k + 1; sbm = int(0.8 * k)
    ok = np.ones(max(n, 0), dtype=bool)
    for c in range(4):
        cs = np.concatenate(([0], np.cumsum(b == c)))
        ok &= (cs[k:k + n] - cs[:n]) < sbm
    return ok & (kmers(b, k) != 0)


# ---- a-3: the hashes and the table bits -------------------------------------------------------------------------------------
def hash64_1(key):
    key = (~key + (key << U64(21))); key = key ^ (key >> U64(24)); key = (key + (key << U64(3))) + (key << U64(8))
    key = key ^ (key >> U64(14)); key = (key + (key << U64(2))) + (key << U64(4)); key = key ^ (key >> U64(28)); key = key + (key << U64(31))
    return key


def hash64_2(key):
    key = key + ~(key << U64(32)); key = key ^ (key >> U64(22)); key = key + ~(key << U64(13)); key = key ^ (key >> U64(8))
    key = key + (key << U64(3)); key = key ^ (key >> U64(15)); key = key + ~(key << U64(27)); key = key ^ (key >> U64(31))
    return key


def synth_mix(bit, which):
    """dsb_synth_mix (dsb_gpu.hip): the 24-bit mix of (bit, table) the synthetic tables are made from"""
    z = bit * U64(0x9E3779B97F4A7C15) + U64(((which + 1) * 0xD1342543DE82EF95) & 0xFFFFFFFFFFFFFFFF)
    z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9); z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return (z ^ (z >> U64(31))) >> U64(40)


def synth_bit(bit, which, fill):
    return synth_mix(np.asarray(bit, dtype=U64), which) < U64(int(fill * 16777216.0))


def synth_table(mask_bits, which, fill):
    """a whole synthetic table as bytes (bit h = bit 7 - (h & 7) of byte h >> 3): the CPU legs' small tables"""
    bits = synth_bit(np.arange(1 << mask_bits, dtype=U64), which, fill)
    return np.packbits(bits)


def summary(table, shift):
    """k_ek_summary: bit g (bit g & 7 of byte g >> 3) = OR of the table bits [g << shift, (g + 1) << shift), shift 3 .. 8"""
    gb = 1 << (shift - 3)
    anyb = table.reshape(-1, gb).max(axis=1) != 0
    return np.packbits(anyb, bitorder="little")


class StrandK:
    """one strand at one k: the k-mer of every window and whether it passes the filter (a read shorter than 40 bases has no windows)"""
    __slots__ = ("n", "k", "L", "km", "okf")

    def __init__(self, seq, strand, k):
        b = codes(seq, strand)
        self.k = k; self.L = len(b); self.n = len(b) - k + 1 if len(b) >= 40 else 0
        self.km = kmers(b, k) if self.n else np.zeros(0, dtype=U64)
        self.okf = filter_ok(b, k) if self.n else np.zeros(0, dtype=bool)


class Strand:
    """a strand under one filter: hit = passes the low-complexity filter and both table bits are set"""
    __slots__ = ("n", "k", "L", "km", "okf", "t0", "t1", "hit")

    def __init__(self, base, bit_fn):
        self.n, self.k, self.L, self.km, self.okf = base.n, base.k, base.L, base.km, base.okf
        self.t0, self.t1 = bit_fn(self.km)
        self.hit = (self.okf & self.t0 & self.t1).astype(np.uint8)


def synth_bits(mask_bits, fill):
    mask = U64((1 << mask_bits) - 1)
    return lambda km: (synth_bit(hash64_1(km) & mask, 0, fill), synth_bit(hash64_2(km) & mask, 1, fill))


def table_bits(ek0, ek1, mask_bits):
    mask = U64((1 << mask_bits) - 1)

    def f(km):
        h1 = hash64_1(km) & mask; h2 = hash64_2(km) & mask
        return ((ek0[(h1 >> U64(3)).astype(np.int64)] >> (7 - (h1 & U64(7))).astype(np.uint8)) & 1).astype(bool), \
               ((ek1[(h2 >> U64(3)).astype(np.int64)] >> (7 - (h2 & U64(7))).astype(np.uint8)) & 1).astype(bool)
    return f


def expected(hit, strand):
    """-> ([(offset, len, top)], total_score): the oracle's scan and marking on these hit bytes"""
    return oracle_lib.seed_stage(hit, strand)


# ---- a plain model of what a lane of k_seed_scan asks for under a look setting ----------------------------------------------------
def asked(hm, look, L=None, k=None, rc=False):
    """hm: the hit bytes in scan order (the reverse strand mirrored: hm[m] = hit[n - 1 - m]).  The reference's scan probes every third
    window, two back at a hit, forward while windows hit up to 61, and goes on three behind the seed; the lane asks for the same windows
    in rounds with some look-ahead: `stride_n` stride points per round (`after_seed` in the first round behind a seed), the two behind a
    hit together with `back_fwd` in front, `fwd_n` per round along a run.  -> (times each window was asked for, facts): facts counts
    rounds, the stride rounds right behind a seed, whose size after_seed sets (counted when that many points lie in front of the strand's end), and -- with L and k -- the rounds whose lowest window sits at base >= 20 of its
    packed word, those whose third word lies behind the strand's words, and the reverse-strand windows that map to rel >= 64"""
    after_seed, back_fwd, fwd_n, stride_n = look
    n = len(hm); cnt = np.zeros(n, dtype=np.int64)
    facts = {"rounds": 0, "after_seed_rounds": 0, "third_word": 0, "third_behind": 0, "rel64": 0}
    nw = (L + 31) // 32 + 1 if L else 0

    def ask(ws):
        facts["rounds"] += 1
        for w in ws:
            cnt[w] += 1
        if L and ws:
            lo = min(ws)
            if (lo & 31) >= 20:
                facts["third_word"] += 1
            if (lo >> 5) + 2 >= nw:
                facts["third_behind"] += 1
            if rc:
                facts["rel64"] += sum(1 for w in ws if 96 - (w - (lo & ~31)) - k >= 64)
    i = 2; spec = stride_n; behind_seed = False
    while i < n:
        pts = [p for p in range(i, i + 3 * spec, 3) if p < n]
        if behind_seed and len(pts) == spec:
            facts["after_seed_rounds"] += 1
        ask(pts)
        first = next((p for p in pts if hm[p]), None)
        if first is None:
            i += 3 * spec; spec = stride_n; behind_seed = False
            continue
        i = first
        fw = [p for p in range(i + 1, i + 1 + back_fwd) if p < n]
        ask([i - 1, i - 2] + fw)
        back = (2 if hm[i - 2] else 1) if hm[i - 1] else 0
        off = i - back; ln = 1 + back; j = i + 1
        slots = back_fwd
        while True:
            run = 0
            while run < slots and j + run < n and hm[j + run]:
                run += 1
            take = min(run, 61 - ln); ln += take; j += take
            if not (take == slots and ln < 61 and j < n):
                break
            slots = fwd_n
            ask([p for p in range(j, j + fwd_n) if p < n])
        i = off + ln + 3; spec = after_seed; behind_seed = True
    return cnt, facts


def host_counters(st, strand, look):
    """what k_seed_scan's two counters must say for this strand: (windows asked for that pass the filter, of those the ones whose table-0
    bit is set), then the windows asked for and the facts of asked()"""
    if st.n == 0:
        return 0, 0, 0, {}
    rc = strand == 0
    hm = st.hit[::-1] if rc else st.hit
    cnt, facts = asked(hm, look, st.L, st.k, rc)
    if rc:
        cnt = cnt[::-1]
    return int((cnt * st.okf).sum()), int((cnt * (st.okf & st.t0)).sum()), int(cnt.sum()), facts


def probe_counter(st):
    """k_seed_probe's counter: every window that passes the filter and table 0 goes on to table 1"""
    return int((st.okf & st.t0).sum())


# ---- classes, from the hit bytes and the oracle's seeds only -------------------------------------------------------------------
CLASSES = ("back0", "back1", "back2", "gap_back", "len1", "len2_59", "len60", "len61_next_hit", "len61_next_miss", "run_across_word", "back_across_word_0",
           "back_across_word_1", "seed_at_0", "seed_to_end", "end_by_seed", "end_by_stride", "no_seed", "one_seed", "key_eq_bin_end", "key_below_bin_end",
           "bin_skipped", "mark_taken_back")
UNREACHABLE = {"run_across_two_words": "a seed holds at most 61 windows, two word boundaries lie 64 apart: the stride hit and the last window of its run span at most one"}


def classes(hit, seeds, strand):
    """the classes one strand is a member of.  Scan order: the reverse strand mirrored (window m = own window n - 1 - m), in which both
    strands are scanned upwards; the 64-window words are those of the strand's own hit bits, which seed_vector_scan reads"""
    n = len(hit); rc = strand == 0
    hm = hit[::-1] if rc else hit
    out = set()
    if not seeds:
        out.add("no_seed")
    if len(seeds) == 1:
        out.add("one_seed")
    cur = 2; index_end = 100; first_key = None
    for m, (o, l, top) in enumerate(seeds):
        off = n - o - l if rc else o
        i = cur + 3 * ((max(off - cur, 0) + 2) // 3)
        back = i - off
        assert 0 <= back <= 2 and hm[i], "the oracle's seed does not start at a stride point"
        out.add("back%d" % back)
        if back == 0 and hm[i - 2]:
            out.add("gap_back")
        out.add("len1" if l == 1 else "len60" if l == 60 else "len2_59" if l < 60 else "len61")
        if l == 61:
            out.discard("len61")
            if off + 61 < n:
                out.add("len61_next_hit" if hm[off + 61] else "len61_next_miss")
        own = (lambda w: n - 1 - w) if rc else (lambda w: w)
        if own(i) >> 6 != own(off + l - 1) >> 6:
            out.add("run_across_word")
            assert abs((own(i) >> 6) - (own(off + l - 1) >> 6)) == 1
        if back >= 1 and own(i) >> 6 != own(i - 1) >> 6:
            out.add("back_across_word_0")
        if back == 2 and own(i) >> 6 == own(i - 1) >> 6 and own(i) >> 6 != own(i - 2) >> 6:
            out.add("back_across_word_1")
        if off == 0:
            out.add("seed_at_0")
        if off + l == n:
            out.add("seed_to_end")
        key = off
        if key < index_end:
            out.add("key_below_bin_end")
            if m == 1 and first_key is not None and first_key >= 100:
                out.add("mark_taken_back")
        else:
            if key == index_end:
                out.add("key_eq_bin_end")
            if key >= index_end + 100:
                out.add("bin_skipped")
            index_end += 100
        if m == 0:
            first_key = key
        cur = off + l + 3
    out.add("end_by_seed" if seeds and cur >= n else "end_by_stride")
    return out


# ---- cases --------------------------------------------------------------------------------------------------------------------
def designed_arrays():
    """hit arrays that fill every class by construction -> [(name, u8 array)]"""
    out = []

    def add(name, a):
        out.append((name, np.asarray(a, dtype=np.uint8)))
    sizes = list(range(21, 26)) + [63, 64, 65, 127, 128, 129, 400, 701]
    for n in sizes:
        add("none_%d" % n, np.zeros(n)); add("all_%d" % n, np.ones(n)); add("alt_%d" % n, np.arange(n) % 2); add("alt1_%d" % n, (np.arange(n) + 1) % 2)
        add("hhhm_%d" % n, (np.arange(n) % 4) != 3); add("hmhhhm_%d" % n, np.tile([1, 0, 1, 1, 1, 0], n // 6 + 1)[:n])
        for w in list(range(6)) + list(range(n - 6, n)):
            a = np.zeros(n); a[w] = 1; add("one_%d_%d" % (n, w), a)
    n = 400
    for ln in range(58, 65):
        for st in list(range(2, 8)) + list(range(60, 69)) + list(range(124, 133)) + list(range(n - 64, n - 57)):
            if st + ln <= n:
                a = np.zeros(n); a[st:st + ln] = 1; add("run_%d_at_%d" % (ln, st), a)
    for left in range(4):
        for ln in (1, 2, 3, 30, 61, 62):
            for n in (128, 131, 400):
                a = np.zeros(n); a[n - left - ln:n - left] = 1; add("tail_%d_%d_%d" % (left, ln, n), a)
    for key in (99, 100, 101, 199, 200, 300, 301, 305, 450):
        for first in (None, 2, 50):
            for ln in (1, 4):
                for n in (520, 523):
                    a = np.zeros(n); a[key:key + ln] = 1
                    if first is not None:
                        a[first:first + 2] = 1
                    add("key_%d_%s_%d_%d" % (key, first, ln, n), a)
    # a bin whose first seed is its longest, one where a later seed takes the mark, and a first seed beyond window 100 followed by a seed of its bin
    for a_len, b_len in ((9, 3), (3, 9), (5, 5)):
        for base in (0, 100, 130):
            a = np.zeros(420); a[base + 5:base + 5 + a_len] = 1; a[base + 40:base + 40 + b_len] = 1; a[base + 70:base + 72] = 1
            add("bin_%d_%d_%d" % (a_len, b_len, base), a)
    # the very first seed lies beyond window 100 and gets the mark of the bin it ends; a second seed of its own bin takes the mark back
    for first in (100, 120, 160):
        for second in (first + 10, 190):
            for l1, l2 in ((1, 1), (5, 1), (1, 7), (5, 7)):
                for n in (300, 333):
                    a = np.zeros(n); a[first:first + l1] = 1; a[second:second + l2] = 1; add("takeback_%d_%d_%d_%d_%d" % (first, second, l1, l2, n), a)
    return out


def random_arrays(n_arrays=1500, seed=11):
    rng = np.random.default_rng(seed)
    probs = (0.01, 0.04, 0.2, 0.5, 0.75, 0.9, 0.97, 0.999)
    out = []
    for t in range(n_arrays):
        p = probs[t % len(probs)]
        n = 21 + t % 64 if t < 512 else int(rng.integers(21, 3001))
        out.append(("rnd_%d_p%g_n%d" % (t, p, n), (rng.random(n) < p).astype(np.uint8)))
    return out


def make_reads(seed, n_reads=600, long_reads=12):
    """reads for one k: random bases with low-complexity stretches, lower case, N, IUPAC letters and '*'; L = 39, 40, 41, every residue of
    L mod 64, most of them short (the work of a test grows with the bases), a few up to 2500"""
    rng = np.random.default_rng(seed)
    lens = [39, 40, 41] + list(range(42, 42 + 64)) + [2500, 2499, 2047, 2048, 2049] + [333] * 40        # (forty of one length: a batch that is not ragged)
    while len(lens) < n_reads:
        r = rng.random()
        lens.append(int(rng.integers(40, 200)) if r < 0.5 else int(rng.integers(200, 700)) if r < 1 - long_reads / n_reads else int(rng.integers(700, 2500)))
    out = []
    for t, L in enumerate(lens):
        s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, L)].copy()
        kind = t % 8
        if kind == 1 and L > 60:      # a homopolymer and a dinucleotide stretch
            a = int(rng.integers(0, L - 40)); s[a:a + int(rng.integers(14, 40))] = ord("ACGT"[int(rng.integers(0, 4))])
            b = int(rng.integers(0, L - 40)); m = int(rng.integers(16, 40)); s[b:b + m] = np.tile(np.frombuffer(b"CA", dtype=np.uint8), m)[:len(s[b:b + m])]
        if kind == 2:
            lo = rng.random(L) < 0.3; s[lo] |= 0x20
        if kind == 3:
            for ch in b"NRYKM*nx-":
                s[rng.random(L) < 0.01] = ch
        if kind == 4 and L > 50:      # all-A windows
            a = int(rng.integers(0, L - 30)); s[a:a + int(rng.integers(20, 30))] = ord("A")
        if kind == 5 and L > 50:      # A-rich: dropped by the filter, not the k-mer 0
            a = int(rng.integers(0, L - 30)); m = int(rng.integers(20, 30)); s[a:a + m] = np.where(rng.random(len(s[a:a + m])) < 0.9, ord("A"), s[a:a + m])
        out.append((b"r%d_%d" % (t, L), s.tobytes(), None))
    return out


# ---- the emulation's stage entries ----------------------------------------------------------------------------------------------
_emu = None


def emu():
    global _emu
    if _emu is None:
        L = C.CDLL(EMU_SO)
        P32 = C.POINTER(C.c_uint32)
        L.emu_stage_scan_read.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_int, C.c_char_p,
                                          C.POINTER(EmuSeed), C.c_int, P32, P32]
        L.emu_stage_scan_bytes.argtypes = [C.c_char_p, C.c_uint32, C.c_int, C.c_char_p, C.POINTER(EmuSeed), C.c_int, P32, P32]
        L.emu_stage_probe.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_void_p, P32]
        L.emu_stage_vector_scan.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(EmuSeed), C.c_int, P32]
        _emu = L
    return _emu


_buf = (EmuSeed * 4096)()


def _seeds(n):
    assert 0 <= n <= 4096, n
    return [(_buf[i].offset, _buf[i].len, _buf[i].top) for i in range(n)]


def emu_scan_bytes(hit, strand, look):
    """the dsb_seed_scan.h state machine alone -> (seeds, total, windows asked for)"""
    ts = C.c_uint32(); cnt = (C.c_uint32 * 5)()
    n = emu().emu_stage_scan_bytes(bytes(hit), len(hit), strand, bytes(look), _buf, 4096, C.byref(ts), cnt)
    return _seeds(n), ts.value, cnt[1]


def emu_scan_read(pk, L, k, ek0, ek1, mask_bits, strand, look, summ=None, shift=0):
    """one lane of k_seed_scan on a packed read -> (seeds, total, (windows that pass the filter, windows asked for, table-1 probes))"""
    ts = C.c_uint32(); cnt = (C.c_uint32 * 5)()
    n = emu().emu_stage_scan_read(pk.ctypes.data, L, k, int(0.8 * k), ek0.ctypes.data, ek1.ctypes.data, (1 << mask_bits) - 1, summ.ctypes.data if summ is not None else None, shift,
                                  strand, bytes(look), _buf, 4096, C.byref(ts), cnt)
    return _seeds(n), ts.value, (cnt[0], cnt[1], cnt[2])


def emu_probe(pk, L, k, ek0, ek1, mask_bits, strand, summ=None, shift=0):
    """every window of a strand through dsb_probe_window -> (hit bytes, table-1 probes)"""
    nw = (L + 31) // 32 + 1; n = L - k + 1
    out = np.zeros(n, dtype=np.uint8); t1 = C.c_uint32()
    P = pk[(0 if strand else nw):]
    emu().emu_stage_probe(P.ctypes.data, n, k, int(0.8 * k), ek0.ctypes.data, ek1.ctypes.data, (1 << mask_bits) - 1, summ.ctypes.data if summ is not None else None, shift,
                          out.ctypes.data, C.byref(t1))
    return out, t1.value


def emu_vector_scan(hit, strand):
    """seed_vector_scan on the hit words of these bytes (bits behind n zero, one zero word behind them)"""
    n = len(hit)
    words = np.zeros((n + 63) // 64 + 1, dtype=U64)
    bits = np.zeros(len(words) * 64, dtype=np.uint8); bits[:n] = np.asarray(hit) != 0
    words[:] = np.packbits(bits, bitorder="little").view(U64)
    ts = C.c_uint32()
    m = emu().emu_stage_vector_scan(words.ctypes.data, n, strand, _buf, 4096, C.byref(ts))
    return _seeds(m), ts.value
