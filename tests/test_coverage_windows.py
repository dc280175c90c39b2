"""Per-window coverage of a classify run (k_ref_windows / k_window_count, dsb_*_coverage_windows, classify --coverage-windows;
DESIGN 2.9.1).  The three integers per window are checked against the reference's own golden output (SAM FLAG, DES_FULL intervals)
and against a host recomputation from the run's hits (coverage_windows_lib, from the definition); the table against a Python
rendering of the same integers.  Everything is compared exactly."""
import gzip
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT
from coverage_windows_lib import HEADER, as_matrix, check_invariants, first_windows, host_windows, table
from reductions_lib import accumulate, counted_records

CLI = os.path.join(ROOT, "desamba_amd", "bin", "deSAMBA")
SYNTH = os.path.join(GOLDEN, "synth")
NODES = os.path.join(GOLDEN, "analysis", "nodes.dmp")


def ref_table(idx):
    n = idx.n_ref
    return [idx.ref_name(r) for r in range(n)], [idx.ref_len(r) for r in range(n)]


# ---------------------------------------------------------------- host side (no GPU)

def test_n_windows(demo):
    import desamba_amd as D
    idx = D.Index(demo["index"])
    _, lens = ref_table(idx)
    assert any(L % 64 for L in lens) and any(L > 1000 for L in lens)
    for W in (1, 63, 64, 1000, 2 ** 31 - 1):
        assert D.n_coverage_windows(idx, W) == first_windows(lens, W)[-1] > 0
    assert D.n_coverage_windows(idx, 1) == sum(lens)
    assert D.n_coverage_windows(idx, 2 ** 31 - 1) == sum(1 for L in lens if L)
    assert D.n_coverage_windows(idx, 0) == 0
    assert D.lib().dsb_coverage_n_windows(None, 1000) == 0
    idx.close()


def test_windows_format(demo):
    import numpy as np
    import desamba_amd as D
    idx = D.Index(demo["index"])
    names, lens = ref_table(idx)
    n = idx.n_ref
    W = 1000
    assert n >= 8 and lens[0] > 2 * W and lens[0] % W and lens[5] > W
    first = first_windows(lens, W)
    cov = np.zeros(n, dtype=D.COVERAGE_DTYPE)
    win = np.zeros(first[-1], dtype=D.WINDOW_DTYPE)
    cov[0] = (3, 150, 420, 61); cov[2] = (1, 0, 0, 30); cov[5] = (7, lens[5], 3 * lens[5] + 17, 0); cov[n - 1] = (2, 1, 1, 59)
    cov[3] = (0, 5, 5, 5)                       # numreads 0: no rows, whatever the rest says
    win[first[0] + 1] = (3, 420, 150)
    win[first[1] - 1] = (1, 2 * (lens[0] % W), lens[0] % W)      # the short last window, fully covered at depth 2
    win[first[3]] = (9, 9, 9)
    win[first[5]] = (7, 3 * W, W)
    win[first[n] - 1] = (2, 1, 1)
    got = D.format_coverage_windows(idx, cov, win, W)
    assert got == table(names, lens, [int(x) for x in cov["numreads"]], as_matrix(win), W)
    lines = got.splitlines()
    rows = sum(first[r + 1] - first[r] for r in (0, 2, 5, n - 1))
    assert lines[0] + b"\n" == HEADER and len(lines) == 1 + rows
    nm = names[0].encode()
    assert lines[1] == b"\t".join([nm, b"0", b"1000", b"0", b"0", b"0", b"0"])           # a window of zeros is a row
    assert lines[2] == b"\t".join([nm, b"1000", b"2000", b"3", b"150", b"15", b"0.42"])
    last = lines[first[1]].split(b"\t")                                                   # reference 0's last window
    assert last[1:3] == [b"%d" % (lens[0] - lens[0] % W), b"%d" % lens[0]] and last[5:] == [b"100", b"2"]
    assert not any(l.startswith(names[3].encode() + b"\t") for l in lines)
    # one window per reference when W >= every LN
    big = max(lens)
    fb = first_windows(lens, big)
    assert fb[-1] == n
    wb = np.zeros(n, dtype=D.WINDOW_DTYPE)
    wb[0] = (3, 420, 150); wb[5] = (7, 3 * lens[5] + 17, lens[5])
    gb = D.format_coverage_windows(idx, cov, wb, big)
    assert gb == table(names, lens, [int(x) for x in cov["numreads"]], as_matrix(wb), big)
    assert gb.count(b"\n") == 1 + 4 and gb.splitlines()[1].split(b"\t")[1:3] == [b"0", b"%d" % lens[0]]
    # the table of no reads is the header alone; a short buffer gives -1
    assert D.format_coverage_windows(idx, np.zeros(n, dtype=D.COVERAGE_DTYPE), win, W) == HEADER
    pc, pw = cov.ctypes.data_as(D.C.c_void_p), win.ctypes.data_as(D.C.c_void_p)
    buf = D.C.create_string_buffer(len(got) + 1)
    f = D.lib().dsb_coverage_windows_format
    assert f(idx.h, pc, pw, W, buf, len(got) - 1) == -1
    assert f(idx.h, pc, pw, W, buf, 10) == -1
    assert f(idx.h, pc, pw, W, buf, len(got) + 1) == len(got)
    assert f(idx.h, pc, pw, 0, buf, len(got) + 1) == -1
    idx.close()


def test_windows_null_handles(built):
    import numpy as np
    import desamba_amd as D
    L = D.lib()
    out = np.zeros(4, dtype=D.WINDOW_DTYPE)
    p = out.ctypes.data_as(D.C.c_void_p)
    n = D.C.c_size_t(0)
    assert L.dsb_ctx_enable_coverage_windows(None, 1000) == D.DSB_EINVAL
    assert L.dsb_ctx_coverage_windows(None, p, 4, D.C.byref(n)) == D.DSB_EINVAL
    assert L.dsb_multi_enable_coverage_windows(None, 1000) == D.DSB_EINVAL
    assert L.dsb_multi_coverage_windows(None, p, 4, D.C.byref(n)) == D.DSB_EINVAL
    buf = D.C.create_string_buffer(64)
    assert L.dsb_coverage_windows_format(None, p, p, 1000, buf, 64) == -1


def test_cli_window_size_needs_the_file(demo, tmp_path):
    fq = os.path.join(SYNTH, "ngs150.fq")
    p = subprocess.run([CLI, "classify", "--coverage-window-size", "100", demo["index"], fq, "-o", str(tmp_path / "x.sam")], stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"--coverage-windows" in p.stderr
    for bad in ("0", "2147483648", "12x", "-5"):
        p = subprocess.run([CLI, "classify", "--coverage-windows", str(tmp_path / "w.tsv"), "--coverage-window-size", bad, demo["index"], fq,
                            "-o", str(tmp_path / "x.sam")], stderr=subprocess.PIPE)
        assert p.returncode != 0 and b"--coverage-window-size" in p.stderr, bad


# ---------------------------------------------------------------- on the GPU

def cli(tmp_path, files, extra=(), tag="run", env=None, index=None):
    out = tmp_path / (tag + ".out")
    e = dict(os.environ); e.update(env or {})
    p = subprocess.run([CLI, "classify"] + list(extra) + [index or os.path.join(ROOT, "data", "demo", "index")] + [str(f) for f in files] + ["-o", str(out)],
                       stderr=subprocess.PIPE, env=e)
    assert p.returncode == 0, p.stderr
    return out.read_bytes()


def golden_ngs150_records(names):
    """ngs150 from the reference's golden files: FLAG / MAPQ from the SAM, ts / te from DES_FULL, matched by position"""
    ref_id = {n: r for r, n in enumerate(names)}
    sam = {}
    order = []
    for line in open(os.path.join(SYNTH, "ngs150.ubfree.sam"), "rb").read().splitlines():
        f = line.split(b"\t")
        flag = int(f[1])
        if f[0] not in sam:
            sam[f[0]] = []; order.append(f[0])
        if flag & 4 or flag & 0x100:
            continue
        sam[f[0]].append((f[2].decode(), int(f[3]), int(f[4])))
    des = {}
    cur = None
    for line in open(os.path.join(SYNTH, "ngs150.desfull.ubfree.txt"), "rb").read().splitlines():
        if not line.strip():
            cur = None; continue
        if cur is None:
            cur = line.split(b"\t")[0]; des[cur] = []; continue
        f = line.split()
        des[cur].append((f[3].decode(), int(f[4][3:]), int(f[5][3:])))
    assert list(des) == order
    records = []
    for name in order:
        recs = sam[name]
        assert len(des[name]) >= len(recs)
        for (rname, pos, mq), (dname, ts, te) in zip(recs, des[name]):
            assert rname == dname and pos == ts, name
            records.append((ref_id[rname], ts, te, mq))
    assert len(records) > 100
    return records


@pytest.mark.gpu
def test_cli_windows_equal_the_reference_s(demo, tmp_path):
    import desamba_amd as D
    idx = D.Index(demo["index"])
    names, lens = ref_table(idx)
    W = 1000
    records = golden_ngs150_records(names)
    assert any(min(ts, lens[r]) // W != (min(te, lens[r]) - 1) // W for r, ts, te, _ in records if te > ts)   # records across a window boundary
    cov = accumulate(len(names), records, lens)
    exp, _ = host_windows(lens, records, W)
    cli(tmp_path, [os.path.join(SYNTH, "ngs150.fq")], ["--coverage-windows", str(tmp_path / "win.tsv")])     # (the default size)
    got = (tmp_path / "win.tsv").read_bytes()
    assert got == table(names, lens, [c[0] for c in cov], exp, W)
    assert got.count(b"\n") > 100
    idx.close()


def run_and_check(D, idx, lens, ctx, recs, W, label):
    """one classify of recs with windows of W bases on ctx (coverage on): windows == host recomputation, and the three invariants"""
    ctx.reset_history(); ctx.enable_coverage_windows(W)
    res = ctx.classify(D.make_reads(recs), strict=False)
    rec = counted_records(res, len(recs))
    exp, empty = host_windows(lens, rec, W)
    win = ctx.coverage_windows()
    got = as_matrix(win)
    assert got.shape == exp.shape == (D.n_coverage_windows(idx, W), 3), (label, W)
    bad = (got != exp).any(axis=1).nonzero()[0]
    assert len(bad) == 0, (label, W, len(bad), int(bad[0]), got[bad[0]].tolist(), exp[bad[0]].tolist())
    check_invariants(lens, W, win, ctx.coverage(), empty)
    assert int(exp[:, 0].sum()) > 0, (label, W)
    return rec


SIZES = {"ngs150": (1, 37, 64, 100, 1000, 100000), "overhang": (1, 37, 64, 100, 1000, 100000), "heavy": (37, 64, 100, 1000, 100000),
         "pb": (37, 64, 100, 1000, 100000),
         # 4095 / 4096: either side of the size from which k_window_count gives a window to the whole wavefront
         "ont20k": (37, 64, 100, 1000, 4095, 4096, 100000)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SIZES))
def test_windows_equal_host_recomputation(demo, name):
    import desamba_amd as D
    idx = D.Index(demo["index"])
    names, lens = ref_table(idx)
    assert max(lens) > 100000                                # (W = 100000: a window of more words than one wavefront's chunk)
    recs = D.read_fastq(os.path.join(SYNTH, name + ".fq"))
    ctx = D.Ctx(idx, 0)
    ctx.enable_coverage()
    for W in SIZES[name]:
        rec = run_and_check(D, idx, lens, ctx, recs, W, name)
        span = [(min(ts, lens[r]), min(te, lens[r])) for r, ts, te, _ in rec]
        assert any(e > s and s // W != (e - 1) // W for s, e in span) or W >= 4095, (name, W)
        if name == "ont20k" and W == 100:
            assert any((e - 1) // W - s // W >= 64 for s, e in span if e > s)   # more than 64 windows: the lane stride loops
        if name == "overhang":
            assert any(te > lens[r] - 200 for r, ts, te, _ in rec)              # a record at a reference's end (the clip at LN)
    ctx.close(); idx.close()


@pytest.mark.gpu
def test_windows_strain_index(strain, tmp_path):
    import desamba_amd as D
    fq = tmp_path / "long.fq"
    subprocess.check_call([os.path.join(ROOT, "tools", "readsim"), strain["index"], str(fq), "384", "50000", "0.15", "8181", "ont"])
    idx = D.Index(strain["index"])
    names, lens = ref_table(idx)
    assert len(lens) >= 10 and min(lens) > 100000
    recs = D.read_fastq(str(fq)) + D.read_fastq(strain["fastq"])
    ctx = D.Ctx(idx, 0)
    ctx.enable_coverage()
    for W in (1000, 100000):
        rec = run_and_check(D, idx, lens, ctx, recs, W, "strain")
        assert sum(1 for r, ts, te, _ in rec if te - ts > 40000) > 100
    ctx.close(); idx.close()


@pytest.mark.gpu
def test_windows_accumulate_independent_of_batches(demo):
    import numpy as np
    import desamba_amd as D
    idx = D.Index(demo["index"])
    names, lens = ref_table(idx)
    W = 100
    recs = D.read_fastq(os.path.join(SYNTH, "pb.fq")) + D.read_fastq(os.path.join(SYNTH, "ngs150.fq"))
    hist = lambda s: max([len(x[1]) for x in recs[:s]], default=0)
    ctx = D.Ctx(idx, 0)
    with pytest.raises(D.DsbError) as e:
        ctx.enable_coverage_windows(W)                      # coverage is off
    assert e.value.code == D.DSB_EINVAL
    ctx.enable_coverage()
    with pytest.raises(D.DsbError) as e:
        ctx.coverage_windows()                              # windows are off
    assert e.value.code == D.DSB_EINVAL
    ctx.enable_coverage_windows(W)
    assert not as_matrix(ctx.coverage_windows()).any()
    res = ctx.classify(D.make_reads(recs))
    one = as_matrix(ctx.coverage_windows())
    cov_one = ctx.coverage()
    assert (one == as_matrix(ctx.coverage_windows())).all()  # fetching changes nothing
    assert (one == host_windows(lens, counted_records(res, len(recs)), W)[0]).all() and one.any()
    # three batches
    ctx.reset_coverage()
    assert not as_matrix(ctx.coverage_windows()).any() and not ctx.coverage().view("<u8").any()
    cuts = [0, 41, 230, len(recs)]
    for a, b in zip(cuts, cuts[1:]):
        ctx.set_history(hist(a))
        ctx.classify(D.make_reads(recs[a:b]))
    assert (as_matrix(ctx.coverage_windows()) == one).all()
    assert (ctx.coverage() == cov_one).all()
    # another window size: windows, bitmap and per-reference counters start again
    ctx.enable_coverage_windows(64)
    assert len(ctx.coverage_windows()) == D.n_coverage_windows(idx, 64) != len(one)
    assert not as_matrix(ctx.coverage_windows()).any() and not ctx.coverage().view("<u8").any()
    # windows off: coverage stays
    ctx.enable_coverage_windows(0)
    with pytest.raises(D.DsbError) as e:
        ctx.coverage_windows()
    assert e.value.code == D.DSB_EINVAL
    assert not ctx.coverage().view("<u8").any()
    ctx.close()
    # two input slots: the second batch staged while the first runs, the windows fetched between them
    ctx = D.Ctx(idx, 0, input_slots=2)
    ctx.enable_coverage(); ctx.enable_coverage_windows(W)
    parts = [D.make_reads(recs[:150]), D.make_reads(recs[150:])]
    ctx.select_slot(0); ctx.set_history(0); ctx.upload(parts[0])
    ctx.select_slot(1); ctx.set_history(hist(150)); ctx.upload(parts[1])
    ctx.select_slot(0); ctx.run(); ctx.fetch()
    mid = as_matrix(ctx.coverage_windows())
    ctx.select_slot(1); ctx.run(); ctx.fetch()
    assert (as_matrix(ctx.coverage_windows()) == one).all() and (mid != one).any() and mid.any()
    assert (ctx.coverage() == cov_one).all()
    ctx.enable_coverage(False)
    with pytest.raises(D.DsbError) as e:
        ctx.coverage_windows()
    assert e.value.code == D.DSB_EINVAL
    with pytest.raises(D.DsbError) as e:
        ctx.enable_coverage_windows(W)
    assert e.value.code == D.DSB_EINVAL
    ctx.close(); idx.close()


@pytest.mark.gpu
def test_windows_several_contexts(demo, tmp_path, monkeypatch):
    import desamba_amd as D
    idx = D.Index(demo["index"])
    names, lens = ref_table(idx)
    W = 100
    recs = D.read_fastq(os.path.join(SYNTH, "ont20k.fq")) + D.read_fastq(os.path.join(SYNTH, "pb.fq")) + D.read_fastq(os.path.join(SYNTH, "ngs_e14.fq"))
    ctx = D.Ctx(idx, 0)
    ctx.enable_coverage(); ctx.enable_coverage_windows(W)
    ctx.classify(D.make_reads(recs))
    one = as_matrix(ctx.coverage_windows())
    cov = ctx.coverage()
    ctx.close()
    monkeypatch.setenv("DSB_SHARD_CHUNK_READS", "30")        # (read when the contexts are made: many chunks on both)
    m = D.Multi(idx, [0, 0])
    m.enable_coverage()
    with pytest.raises(D.DsbError) as e:
        m.coverage_windows()
    assert e.value.code == D.DSB_EINVAL
    m.enable_coverage_windows(W)
    m.classify(D.make_reads(recs))
    assert min(m.last_calls()) > 0
    assert (as_matrix(m.coverage_windows()) == one).all() and one.any()
    assert (as_matrix(m.coverage_windows()) == one).all()
    assert (m.coverage() == cov).all()
    m.close()
    monkeypatch.delenv("DSB_SHARD_CHUNK_READS")
    files = [os.path.join(SYNTH, n + ".fq") for n in ("ont20k", "pb", "ngs_e14")]
    env = {"DSB_CLI_BATCH_KB": "128"}
    size = ["--coverage-window-size", str(W)]
    cli(tmp_path, files, ["--coverage-windows", str(tmp_path / "g0.tsv")] + size, tag="g0", env=env)
    cli(tmp_path, files, ["-g", "0,0", "--coverage-windows", str(tmp_path / "g00.tsv")] + size, tag="g00", env=env)
    exp = table(names, lens, [int(x) for x in cov["numreads"]], one, W)
    assert (tmp_path / "g0.tsv").read_bytes() == (tmp_path / "g00.tsv").read_bytes() == exp
    idx.close()


@pytest.mark.gpu
def test_cli_outputs_unchanged_by_windows(demo, tmp_path):
    names = ["ont20k", "ngs_e14", "pb", "appc", "wrapq", "ngs150"]
    files = []
    for i, n in enumerate(names):
        src = os.path.join(SYNTH, n + ".fq")
        if i % 2:
            dst = tmp_path / (n + ".fq.gz")
            with gzip.open(dst, "wb") as f:
                f.write(open(src, "rb").read())
            files.append(dst)
        else:
            files.append(src)
    env = {"DSB_CLI_BATCH_KB": "256"}
    out = lambda tag: ["--taxonomy", NODES, "--report", str(tmp_path / (tag + ".report")), "--coverage", str(tmp_path / (tag + ".tsv"))]
    win = lambda tag: ["--coverage-windows", str(tmp_path / (tag + ".win"))]
    sam_a = cli(tmp_path, files, out("a"), "a", env)
    sam_b = cli(tmp_path, files, out("b") + win("b"), "b", env)
    sam_c = cli(tmp_path, files, win("c"), "c", env)                                   # windows without --coverage FILE
    assert sam_a == open(os.path.join(SYNTH, "multi6.ubfree.sam"), "rb").read()
    assert sam_b == sam_a and sam_c == sam_a
    assert (tmp_path / "a.report").read_bytes() == (tmp_path / "b.report").read_bytes() != b""
    assert (tmp_path / "a.tsv").read_bytes() == (tmp_path / "b.tsv").read_bytes() and (tmp_path / "a.tsv").read_bytes().count(b"\n") > 10
    w = (tmp_path / "b.win").read_bytes()
    assert w == (tmp_path / "c.win").read_bytes() and w.startswith(HEADER) and w.count(b"\n") > 100
    # the table's references are the --coverage table's, each with all its windows
    refs = [l.split(b"\t")[0] for l in (tmp_path / "a.tsv").read_bytes().splitlines()[1:]]
    seen = []
    for l in w.splitlines()[1:]:
        if not seen or seen[-1] != l.split(b"\t")[0]:
            seen.append(l.split(b"\t")[0])
    assert seen == refs
    des = cli(tmp_path, files, ["-f", "DES_FULL"], "des", env)
    assert des == cli(tmp_path, files, ["-f", "DES_FULL"] + win("d"), "deswin", env)
    assert (tmp_path / "d.win").read_bytes() == w
