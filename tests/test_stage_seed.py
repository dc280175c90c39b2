"""Stage tests of the front of the pipe (DESIGN.md "Stage tests for the seed lookup"): a-1 encode / pack, a-2 the low-complexity filter,
a-3 the two table probes and the three device forms of the seed scan -- seed_vector_scan over the hit words, the dsb_seed_scan.h state
machine, and one lane of k_seed_scan (the state machine with the emulation's restatement of the kernel's round) -- against the oracle's own scan and marking (ora_seed_stage) on hit bytes
that plain numpy computes (tests/stage_seed_lib.py).  The CPU legs run the device code in the 1-lane emulation; the device leg goes through
the product library on synthetic filter tables of every size, and on the demo index for the summary of table 0."""
import collections
import ctypes as C
import os
import time

import numpy as np
import pytest

import stage_seed_lib as S

# classes of the scan's wanted windows and of the filter, counted beside those of stage_seed_lib.CLASSES
WANT_CLASSES = ("third_word", "third_behind", "rel64", "filter_drop_both_bits", "all_A_kmer")
FULL_MIN, DEVICE_MIN = 50, 5


# ---- the cases and what is expected of them, computed once ------------------------------------------------------------------------
class Config:
    """the reads of one k under one filter: per read the two strands (forward, reverse), the oracle's seeds on their hit bytes, and the
    host's count of what each scan asks for"""

    def __init__(self, k, reads, bases, bit_fn):
        self.k = k; self.reads = reads
        self.st = [(S.Strand(f, bit_fn), S.Strand(r, bit_fn)) for f, r in bases]
        self.exp = [(S.expected(f.hit, 1), S.expected(r.hit, 0)) for f, r in self.st]
        self._cnt = {}

    def strands(self):
        for i, (f, r) in enumerate(self.st):
            yield i, 1, f, self.exp[i][0]
            yield i, 0, r, self.exp[i][1]

    def counters(self, look, idx=None):
        """(windows, probes_t1, asked, facts per strand) of k_seed_scan over the reads idx (all by default)"""
        if look not in self._cnt:
            self._cnt[look] = {(i, s): S.host_counters(st, s, look) for i, s, st, _ in self.strands()}
        per = self._cnt[look]
        keys = [(i, s) for i in (range(len(self.reads)) if idx is None else idx) for s in (1, 0)]
        return sum(per[q][0] for q in keys), sum(per[q][1] for q in keys), sum(per[q][2] for q in keys), [per[q][3] for q in keys]

    def probe_counter(self, idx=None):
        return sum(S.probe_counter(st) for i in (range(len(self.reads)) if idx is None else idx) for st in self.st[i])

    def classes(self):
        c = collections.Counter()
        for i, s, st, (seeds, total) in self.strands():
            if st.n == 0:
                continue
            c.update(S.classes(st.hit, seeds, s))
            if (~st.okf & st.t0 & st.t1).any():
                c["filter_drop_both_bits"] += 1
            if (st.km == 0).any():
                c["all_A_kmer"] += 1
        return c


_reads, _bases, _tables, _configs = {}, {}, {}, {}


def reads_of(k):
    if k not in _reads:
        _reads[k] = S.make_reads(k)
        _bases[k] = [(S.StrandK(seq, 1, k), S.StrandK(seq, 0, k)) for nm, seq, q in _reads[k]]
    return _reads[k], _bases[k]


def cpu_tables(fill):
    if fill not in _tables:
        _tables[fill] = (S.synth_table(S.CPU_MASK_BITS, 0, fill), S.synth_table(S.CPU_MASK_BITS, 1, fill))
    return _tables[fill]


def config(k, fill, where):
    """where: "cpu" (the 2^22-bit tables of the CPU legs) or "device" (the mask of the table size that k belongs to)"""
    key = (k, fill, where)
    if key not in _configs:
        reads, bases = reads_of(k)
        bits = S.synth_bits(S.TABLES[S.TABLE_OF_K[k]][0], fill) if where == "device" else S.table_bits(*cpu_tables(fill), S.CPU_MASK_BITS)
        _configs[key] = Config(k, reads, bases, bits)
    return _configs[key]


def want_classes(cfg, look):
    c = collections.Counter()
    for f in cfg.counters(look)[3]:
        for name in ("third_word", "third_behind", "rel64", "after_seed_rounds"):
            if f.get(name):
                c[name] += 1
    return c


@pytest.fixture(scope="module")
def arrays(built):
    arrs = S.designed_arrays() + S.random_arrays()
    return [(name, a, d, S.expected(a, d)) for name, a in arrs for d in (1, 0)]


# ---- CPU legs -----------------------------------------------------------------------------------------------------------------------
def test_synthetic_rule_in_numpy(built):
    """the numpy restatement of the synthetic tables' rule against the library's dsb_synthetic_filter_bit: 10 000 sampled bits per table
    and fill, over the whole range of the largest mask"""
    import desamba_amd as D
    L = D.lib(); rng = np.random.default_rng(5)
    for fill in S.FILLS:
        for which in (0, 1):
            bits = np.concatenate((rng.integers(0, 1 << 37, 9990, dtype=np.uint64), np.array([0, 1, 7, 8, (1 << 30) - 1, 1 << 30, (1 << 37) - 1, 1 << 36, 255, 256], dtype=np.uint64)))
            got = S.synth_bit(bits, which, fill)
            exp = np.array([L.dsb_synthetic_filter_bit(which, int(b), fill) for b in bits], dtype=bool)
            assert (got == exp).all(), (fill, which)
            assert abs(got.mean() - fill) < 0.03


def test_pack_and_summary_in_numpy(built):
    """the library's own pieces against direct statements: a packed word holds 32 bases, first base on top; a summary bit is the OR of
    its table bits"""
    seq = b"ACGTNacgtn*RYT" * 11 + b"GATTACA"
    pk = S.pack(seq); L = len(seq); nw = (L + 31) // 32 + 1
    for s, strand in enumerate((1, 0)):
        b = S.codes(seq, strand)
        for p in (0, 1, 31, 32, 33, L - 1):
            assert (int(pk[s * nw + p // 32]) >> (62 - 2 * (p % 32))) & 3 == b[p]
        assert int(pk[s * nw + nw - 1]) == 0
    t0 = S.synth_table(16, 0, 0.02)
    for shift in (3, 6, 8):
        sm = S.summary(t0, shift)
        bits = np.unpackbits(t0)
        for g in (0, 1, 5, 100, (1 << (16 - shift)) - 1):
            assert ((sm[g >> 3] >> (g & 7)) & 1) == bits[g << shift:(g + 1) << shift].max()


def test_arrays_seed_vector_scan(arrays):
    """leg (a): seed_vector_scan (the scan k_classify and k_seed_dump run over the hit words) on every array, both directions.  The
    emulation's shim has one pointer type for global memory and LDS, so there is one instantiation to run."""
    for name, a, d, exp in arrays:
        assert S.emu_vector_scan(a, d) == exp, (name, d)


@pytest.mark.parametrize("look", sorted(S.LOOKS))
def test_arrays_state_machine(arrays, look):
    """leg (b) on arrays: the dsb_seed_scan.h state machine alone under every look setting; on the designed arrays the number of windows
    it asks for is also what the plain model of the look-ahead asks for"""
    lk = S.LOOKS[look]
    for name, a, d, exp in arrays:
        sv, total, n_asked = S.emu_scan_bytes(a, d, lk)
        assert (sv, total) == exp, (name, d)
        if not name.startswith("rnd_"):
            assert n_asked == int(S.asked(a[::-1] if d == 0 else a, lk)[0].sum()), (name, d)


@pytest.mark.parametrize("k", [16, 17, 18, 19, 20])
def test_reads_cpu(built, k):
    """legs (b) and (c) on reads at the six fills: the hit bytes of every window through dsb_probe_window on the packed words equal the
    numpy bytes (the filter is forced by the reads' low-complexity stretches), and one lane of k_seed_scan -- the state machine and the
    restated round -- gives the oracle's seeds under every look setting, with the work counters the host counts"""
    t0 = time.time()
    for fill in S.FILLS:
        cfg = config(k, fill, "cpu"); ek0, ek1 = cpu_tables(fill)
        rule = S.synth_bits(S.CPU_MASK_BITS, fill)          # the tables the emulation reads are the rule's
        for st in [x for pair in cfg.st[:40] for x in pair]:
            r0, r1 = rule(st.km)
            assert (r0 == st.t0).all() and (r1 == st.t1).all()
        summ = S.summary(ek0, 6) if fill == S.FILLS[0] else None
        pks = {}
        counted = [lk for nm, lk in S.LOOKS.items() if k == 16 or nm == "default"]
        for lk in counted:
            cfg.counters(lk)
        for i, s, st, exp in cfg.strands():
            seq = cfg.reads[i][1]; L = len(seq)
            if L < 40:
                assert st.n == 0 and exp == ([], 0)
                continue
            pk = pks.setdefault(i, S.pack(seq))
            hb, went_t1 = S.emu_probe(pk, L, k, ek0, ek1, S.CPU_MASK_BITS, s)
            assert (hb == st.hit).all() and went_t1 == S.probe_counter(st), (fill, i, s)
            for nm, lk in S.LOOKS.items():
                sv, total, cnt = S.emu_scan_read(pk, L, k, ek0, ek1, S.CPU_MASK_BITS, s, lk)
                assert (sv, total) == exp, (fill, i, s, nm)
                if lk in counted:
                    w, p1, al, _ = cfg._cnt[lk][(i, s)]
                    assert cnt == (w, al, p1), (fill, i, s, nm)
            if summ is not None:      # the summary saves table reads and changes nothing else
                assert (S.emu_probe(pk, L, k, ek0, ek1, S.CPU_MASK_BITS, s, summ, 6)[0] == st.hit).all()
                sv, total, cnt2 = S.emu_scan_read(pk, L, k, ek0, ek1, S.CPU_MASK_BITS, s, S.LOOKS["default"], summ, 6)
                assert (sv, total) == exp and cnt2 == S.emu_scan_read(pk, L, k, ek0, ek1, S.CPU_MASK_BITS, s, S.LOOKS["default"])[2]
    print("test_reads_cpu k=%d: %.1f s" % (k, time.time() - t0))


def device_configs():
    return [(k, fill) for k in sorted(S.DEVICE_FILLS) for fill in S.DEVICE_FILLS[k]]


def test_classes(arrays):
    """every class holds at least 50 strands in the full set (arrays, and the reads of every k and fill) and at least 5 in the device
    subset (the reads under the tables and fills of the device leg); the classes no input can reach hold none"""
    full = collections.Counter()
    for name, a, d, (seeds, total) in arrays:
        full.update(S.classes(a, seeds, d))
    looks = collections.Counter()
    for k in (16, 17, 18, 19, 20):
        for fill in S.FILLS:
            cfg = config(k, fill, "cpu")
            full.update(cfg.classes())
            full.update(want_classes(cfg, S.LOOKS["default"]))
        for nm, lk in S.LOOKS.items():
            looks[nm] += want_classes(config(k, 0.7, "cpu"), lk)["after_seed_rounds"]
    dev = collections.Counter()
    for k, fill in device_configs():
        cfg = config(k, fill, "device")
        dev.update(cfg.classes())
        for lk in (S.LOOKS["dense"] if k == 16 else S.LOOKS["default"], S.LOOKS["round3"], S.LOOKS["one"]):
            dev.update(want_classes(cfg, lk))
    print("classes (full set / device subset):")
    for c in S.CLASSES + WANT_CLASSES:
        print("  %-24s %7d %7d" % (c, full[c], dev[c]))
    print("  rounds sized by after_seed, strands per look setting:", dict(looks))
    for c in S.CLASSES + WANT_CLASSES:
        assert full[c] >= FULL_MIN, (c, full[c])
        assert dev[c] >= DEVICE_MIN, (c, dev[c])
    for nm in S.LOOKS:
        assert looks[nm] >= FULL_MIN, (nm, looks[nm])
    for c in S.UNREACHABLE:
        assert full[c] == 0 and dev[c] == 0, c


# ---- device leg ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def syn(demo):
    """one context for the synthetic tables of every size (a new size replaces the tables), with two input slots"""
    import desamba_amd as D
    idx = D.Index(demo["index"]); ctx = D.Ctx(idx, 0, input_slots=2)
    yield D, ctx
    ctx.close(); idx.close()


def _env(monkeypatch, ctx, scan, look=None):
    monkeypatch.setenv("DSB_SEED_SCAN", str(scan))
    if look is None:
        monkeypatch.delenv("DSB_SCAN_LOOK", raising=False)
    else:
        monkeypatch.setenv("DSB_SCAN_LOOK", ",".join(str(v) for v in look))
    ctx.reload_env()


def _check_dump(ctx, cfg, idx, bits):
    """the stage dumps of the reads idx of cfg (batch order) against the numpy bytes and the oracle's seeds"""
    for j, i in enumerate(idx):
        for s in (1, 0):
            st = cfg.st[i][0 if s else 1]
            if bits:
                assert ctx.exist_bits(j, s) == st.hit.tobytes(), (cfg.k, i, s)
            assert ctx.seeds(j, s) == cfg.exp[i][0 if s else 1], (cfg.k, i, s)


def _default_look(k):
    return S.LOOKS["dense"] if S.TABLE_OF_K[k] <= (256 << 20) else S.LOOKS["default"]


def _run_scan(monkeypatch, D, ctx, cfg, idx, k, looks=(None, (8, 6, 8, 8), (1, 0, 1, 1)), upload=True):
    for look in looks:
        _env(monkeypatch, ctx, 1, look)
        if upload:
            ctx.upload(D.make_reads([cfg.reads[i] for i in idx]))
        ctx.run(); t = ctx.timing()
        assert t.seed_scan == 1 and t.classify_ms == 0
        _check_dump(ctx, cfg, idx, bits=False)
        w, p1, _, _ = cfg.counters(look if look is not None else _default_look(k), idx)
        assert (t.windows, t.probes_t1) == (w, p1), (k, look)


@pytest.mark.gpu
@pytest.mark.parametrize("k,fill", device_configs())
def test_device_fill(syn, monkeypatch, k, fill):
    """both seed lookups of the library on synthetic tables of the size that belongs to k, all reads in one ragged batch.  The probe of
    every window: the hit bits equal the numpy bytes (which also checks encode and pack), seed_vector_scan on the device (k_seed_dump)
    gives the oracle's seeds, and the table-1 counter is the host's.  k_seed_scan under the default look setting, round 3's and the
    narrowest: the oracle's seeds and total_score on both strands, and both work counters equal to the host's count of what the state
    machine asks for -- under the default setting that count is the dense one (stride 3) for tables of <= 256 MiB, which differs."""
    D, ctx = syn
    cfg = config(k, fill, "device"); idx = list(range(len(cfg.reads)))
    t0 = time.time()
    ctx.use_synthetic_filter(S.TABLE_OF_K[k], fill)
    t_fill = time.time() - t0
    _env(monkeypatch, ctx, 0)
    ctx.upload(D.make_reads(cfg.reads)); ctx.run(); t = ctx.timing()
    assert t.seed_scan == 0 and t.classify_ms == 0
    _check_dump(ctx, cfg, idx, bits=True)
    assert t.probes_t1 == cfg.probe_counter()
    if k == 16:
        assert cfg.counters(S.LOOKS["dense"])[:2] != cfg.counters(S.LOOKS["default"])[:2]
    _run_scan(monkeypatch, D, ctx, cfg, idx, k)
    print("test_device_fill k=%d fill=%g: tables %.2f s, all %.2f s" % (k, fill, t_fill, time.time() - t0))


@pytest.mark.gpu
def test_device_batch_shapes(syn, monkeypatch):
    """the same expectations on other batch shapes (k = 16, fill 0.7): reads of one length (no scan order), one read, 129 reads (a
    half-filled last workgroup of k_seed_scan), and a batch staged in the second input slot while another one sits in the first"""
    D, ctx = syn
    k, fill = 16, 0.7
    cfg = config(k, fill, "device")
    ctx.use_synthetic_filter(S.TABLE_OF_K[k], fill)
    same = [i for i, r in enumerate(cfg.reads) if len(r[1]) == 333]
    assert len(same) >= 40
    ragged = list(range(3, 3 + 129))
    for idx in (same, [len(cfg.reads) - 1], ragged):
        _env(monkeypatch, ctx, 0)
        ctx.upload(D.make_reads([cfg.reads[i] for i in idx])); ctx.run()
        _check_dump(ctx, cfg, idx, bits=True)
        assert ctx.timing().probes_t1 == cfg.probe_counter(idx)
        _run_scan(monkeypatch, D, ctx, cfg, idx, k)
    first, second = list(range(200, 330)), list(range(330, 400))
    for scan in (0, 1):
        _env(monkeypatch, ctx, scan)
        ctx.select_slot(0); ctx.upload(D.make_reads([cfg.reads[i] for i in first]))
        ctx.select_slot(1); ctx.upload(D.make_reads([cfg.reads[i] for i in second]))
        for slot, idx in ((1, second), (0, first)):
            ctx.select_slot(slot); ctx.run(); t = ctx.timing()
            _check_dump(ctx, cfg, idx, bits=scan == 0)
            if scan:
                assert (t.windows, t.probes_t1) == cfg.counters(_default_look(k), idx)[:2]
            else:
                assert t.probes_t1 == cfg.probe_counter(idx)
    ctx.select_slot(0)


@pytest.mark.gpu
def test_device_upload_routes(syn, monkeypatch, tmp_path):
    """k = 16, fill 0.7: the host-packed upload, the ASCII upload, upload_text and upload_fastq stage the same strands -- reads with lower
    case, N, IUPAC letters and '*' among them: the same hit bits and seeds on both paths, dumped behind every route"""
    D, ctx = syn
    k, fill = 16, 0.7
    cfg = config(k, fill, "device")
    ctx.use_synthetic_filter(S.TABLE_OF_K[k], fill)
    idx = [i for i in range(len(cfg.reads)) if i % 8 in (2, 3)][:60] + list(range(0, 40))
    recs = [cfg.reads[i] for i in idx]
    assert any(b"*" in r[1] for r in recs) and any(b"n" in r[1] for r in recs) and any(b"R" in r[1] for r in recs)
    blob = b"".join(r[1] for r in recs)
    off = (C.c_uint64 * len(recs))(); ln = (C.c_uint32 * len(recs))(); o = 0
    for j, r in enumerate(recs):
        off[j] = o; ln[j] = len(r[1]); o += len(r[1])
    buf = C.create_string_buffer(blob, len(blob) + 64)
    fq = tmp_path / "routes.fq"
    fq.write_bytes(b"".join(b"@" + r[0] + b"\n" + r[1] + b"\n+\n" + b"I" * len(r[1]) + b"\n" for r in recs if len(r[1])))
    fq_idx = [i for i, r in zip(idx, recs) if len(r[1])]

    def packed():
        monkeypatch.delenv("DSB_UPLOAD_TEXT", raising=False); ctx.reload_env(); ctx.upload(D.make_reads(recs)); return idx

    def ascii_():
        monkeypatch.setenv("DSB_UPLOAD_TEXT", "1"); ctx.reload_env(); ctx.upload(D.make_reads(recs)); return idx

    def text():
        ctx.upload_text(C.cast(buf, C.c_void_p), len(blob), off, ln, len(recs)); return idx

    def fastq():
        assert ctx.upload_fastq(str(fq)) == len(fq_idx); return fq_idx

    for route in (packed, ascii_, text, fastq):
        for scan in (0, 1):
            _env(monkeypatch, ctx, scan)
            ids = route()
            ctx.run()
            _check_dump(ctx, cfg, ids, bits=scan == 0)
            t = ctx.timing()
            if scan:
                assert (t.windows, t.probes_t1) == cfg.counters(_default_look(k), ids)[:2], route.__name__
            else:
                assert t.probes_t1 == cfg.probe_counter(ids), route.__name__
    monkeypatch.delenv("DSB_UPLOAD_TEXT", raising=False); ctx.reload_env()


@pytest.mark.gpu
@pytest.mark.parametrize("setting", [None, "0", "3", "8"])
def test_device_summary(demo, oracle, monkeypatch, setting):
    """the summary of table 0 (DSB_EK_SUMMARY unset, off, finest, coarsest) on the demo index: 300 demo reads and the designed reads give
    the oracle's bits and seeds on both paths; the summary only saves table reads, so the work counters are those of the host's count
    (k_seed_scan: the windows that pass the filter under the default look setting) and the same at every setting"""
    import desamba_amd as D
    if setting is None:
        monkeypatch.delenv("DSB_EK_SUMMARY", raising=False)
    else:
        monkeypatch.setenv("DSB_EK_SUMMARY", setting)
    recs = D.read_fastq(demo["fastq"], 300) + S.make_reads(16, n_reads=160)
    k = 16
    exp = []
    for nm, seq, q in recs:
        row = []
        for s in (1, 0):
            hit = np.frombuffer(bytes(oracle.exist_bits(seq, s)[:max(len(seq) - k + 1, 0)]) if len(seq) >= 40 else b"", dtype=np.uint8)
            row.append((hit, S.expected(hit, s)))
        exp.append(row)
    idx = D.Index(demo["index"]); ctx = D.Ctx(idx, 0)
    try:
        got = {}
        for scan in (0, 1):
            _env(monkeypatch, ctx, scan)
            ctx.upload(D.make_reads(recs)); ctx.run(); t = ctx.timing()
            got[scan] = (t.windows, t.probes_t1)
            for j in range(len(recs)):
                for s in (1, 0):
                    hit, seeds = exp[j][0 if s else 1]
                    assert ctx.exist_bits(j, s) == hit.tobytes(), (j, s)
                    assert ctx.seeds(j, s) == seeds, (j, s)
        want = 0
        for (nm, seq, q), row in zip(recs, exp):
            for s in (1, 0):
                base = S.StrandK(seq, s, k)
                if base.n:
                    hit = row[0 if s else 1][0]
                    cnt = S.asked(hit[::-1] if s == 0 else hit, S.LOOKS["default"])[0]
                    want += int(((cnt[::-1] if s == 0 else cnt) * base.okf).sum())
        assert got[1][0] == want
        ref = _summary_counters.setdefault("ref", got)
        assert got == ref, (setting, got, ref)
    finally:
        ctx.close(); idx.close()


_summary_counters = {}
