"""Per-reference coverage of a classify run (k_ref_cover / k_cover_count, dsb_*_coverage, classify --coverage).
The four integers per reference are checked against the reference's own golden output (SAM FLAG / MAPQ, DES_FULL intervals) and
against a host recomputation from the run's hits; the table against a Python rendering of the same integers."""
import gzip
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT
from reductions_lib import accumulate, counted_records

CLI = os.path.join(ROOT, "desamba_amd", "bin", "deSAMBA")
SYNTH = os.path.join(GOLDEN, "synth")
NODES = os.path.join(GOLDEN, "analysis", "nodes.dmp")
FIELDS = ("numreads", "covbases", "aligned_bases", "mapq_sum")
HEADER = b"#rname\tstartpos\tendpos\tnumreads\tcovbases\tcoverage\tmeandepth\tmeanmapq\n"


def table(names, lens, cov):
    """the expected --coverage file from the four integers per reference"""
    out = [HEADER]
    for r, (nr, cb, ab, mq) in enumerate(cov):
        if nr:
            L = lens[r]
            out.append(b"%s\t1\t%d\t%d\t%d\t%s\t%s\t%s\n" % (names[r].encode(), L, nr, cb, (b"%g" % (100.0 * cb / L)),
                                                                  (b"%g" % (ab / L)), (b"%.1f" % (mq / nr))))
    return b"".join(out)


def ref_table(idx):
    n = idx.n_ref
    return [idx.ref_name(r) for r in range(n)], [idx.ref_len(r) for r in range(n)]


def as_tuples(cov):
    return [tuple(int(x[f]) for f in FIELDS) for x in cov]


# ---------------------------------------------------------------- host side (no GPU)

def test_coverage_format(demo):
    import numpy as np
    import desamba_amd as D
    idx = D.Index(demo["index"])
    names, lens = ref_table(idx)
    n = idx.n_ref
    assert n >= 8
    cov = np.zeros(n, dtype=D.COVERAGE_DTYPE)
    rows = {0: (3, 150, 420, 61), 2: (1, 0, 0, 30), 5: (7, lens[5], 3 * lens[5] + 17, 0), n - 1: (2, 1, 1, 59)}
    for r, v in rows.items():
        cov[r] = v
    cov[3] = (0, 5, 5, 5)                       # numreads 0: no row, whatever the rest says
    got = D.format_coverage(idx, cov)
    exp = table(names, lens, [tuple(int(x) for x in c) for c in cov])
    assert got == exp
    lines = got.splitlines()
    assert lines[0] + b"\n" == HEADER and len(lines) == 1 + len(rows)
    f = lines[1].split(b"\t")
    assert f[:5] == [names[0].encode(), b"1", b"%d" % lens[0], b"3", b"150"] and f[7] == b"20.3"
    assert lines[2].split(b"\t")[4:] == [b"0", b"0", b"0", b"30.0"]      # a counted record with an empty interval
    assert lines[3].split(b"\t")[5] == b"100"
    # the table of no reads is the header alone; a short buffer gives -1
    assert D.format_coverage(idx, np.zeros(n, dtype=D.COVERAGE_DTYPE)) == HEADER
    buf = D.C.create_string_buffer(len(got) - 1)
    assert D.lib().dsb_coverage_format(idx.h, cov.ctypes.data_as(D.C.c_void_p), buf, len(got) - 1) == -1
    assert D.lib().dsb_coverage_format(idx.h, cov.ctypes.data_as(D.C.c_void_p), buf, 10) == -1
    buf = D.C.create_string_buffer(len(got) + 1)
    assert D.lib().dsb_coverage_format(idx.h, cov.ctypes.data_as(D.C.c_void_p), buf, len(got) + 1) == len(got)
    idx.close()


def test_coverage_null_handles(built):
    import numpy as np
    import desamba_amd as D
    L = D.lib()
    out = np.zeros(4, dtype=D.COVERAGE_DTYPE)
    p = out.ctypes.data_as(D.C.c_void_p)
    assert L.dsb_ctx_coverage(None, p) == D.DSB_EINVAL
    assert L.dsb_multi_coverage(None, p) == D.DSB_EINVAL
    assert L.dsb_ctx_enable_coverage(None, 1) == D.DSB_EINVAL
    assert L.dsb_ctx_reset_coverage(None) == D.DSB_EINVAL
    assert L.dsb_multi_enable_coverage(None, 1) == D.DSB_EINVAL


# ---------------------------------------------------------------- on the GPU

def cli(tmp_path, files, extra=(), tag="run", env=None, index=None):
    out = tmp_path / (tag + ".out")
    e = dict(os.environ); e.update(env or {})
    p = subprocess.run([CLI, "classify"] + list(extra) + [index or os.path.join(ROOT, "data", "demo", "index")] + [str(f) for f in files] + ["-o", str(out)],
                       stderr=subprocess.PIPE, env=e)
    assert p.returncode == 0, p.stderr
    return out.read_bytes()


def golden_ngs150_table(idx):
    """ngs150 from the reference's golden files: FLAG / MAPQ from the SAM, ts / te from DES_FULL, matched by position"""
    names, lens = ref_table(idx)
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
    return names, lens, accumulate(len(names), records, lens)


@pytest.mark.gpu
def test_cli_coverage_equals_the_reference_s(demo, tmp_path):
    import desamba_amd as D
    idx = D.Index(demo["index"])
    names, lens, exp = golden_ngs150_table(idx)
    cli(tmp_path, [os.path.join(SYNTH, "ngs150.fq")], ["--coverage", str(tmp_path / "cov.tsv")])
    got = (tmp_path / "cov.tsv").read_bytes()
    assert got == table(names, lens, exp)
    assert got.count(b"\n") > 10
    idx.close()


@pytest.mark.gpu
def test_coverage_equals_host_recomputation(demo):
    import desamba_amd as D
    idx = D.Index(demo["index"])
    names, lens = ref_table(idx)
    ctx = D.Ctx(idx, 0)
    ctx.enable_coverage()
    seen = [0] * idx.n_ref
    near_end = 0
    for name in ("ont20k", "pb", "overhang", "manyanchors", "heavy", "appc"):
        recs = D.read_fastq(os.path.join(SYNTH, name + ".fq"))
        ctx.reset_history(); ctx.reset_coverage()
        res = ctx.classify(D.make_reads(recs), strict=False)
        rec = counted_records(res, len(recs))
        exp = accumulate(idx.n_ref, rec, lens)
        got = as_tuples(ctx.coverage())
        assert got == exp, name
        assert sum(x[0] for x in got) == len(rec) > 0
        assert all(g[1] <= lens[r] for r, g in enumerate(got))
        near_end += sum(1 for r, ts, te, _ in rec if te > lens[r] - 200)
        for r, g in enumerate(got):
            seen[r] += g[1]
    assert near_end > 0                                     # (overhang: a read past a reference's end; the hits stop at LN, the clip is a guard)
    # a reference whose length is not a multiple of 64 next to one that starts on the next word, both covered
    assert any(lens[r] % 64 and seen[r] and seen[r + 1] for r in range(idx.n_ref - 1))
    ctx.close(); idx.close()


@pytest.mark.gpu
def test_coverage_accumulates_independent_of_batches(demo):
    import desamba_amd as D
    idx = D.Index(demo["index"])
    recs = D.read_fastq(os.path.join(SYNTH, "pb.fq")) + D.read_fastq(os.path.join(SYNTH, "ngs150.fq"))
    hist = lambda s: max([len(x[1]) for x in recs[:s]], default=0)
    ctx = D.Ctx(idx, 0)
    with pytest.raises(D.DsbError) as e:
        ctx.coverage()
    assert e.value.code == D.DSB_EINVAL
    with pytest.raises(D.DsbError) as e:
        ctx.reset_coverage()
    assert e.value.code == D.DSB_EINVAL
    ctx.enable_coverage()
    res = ctx.classify(D.make_reads(recs))
    one = as_tuples(ctx.coverage())
    assert one == as_tuples(ctx.coverage())                 # fetching changes nothing
    assert one == accumulate(idx.n_ref, counted_records(res, len(recs)), ref_table(idx)[1])
    # three batches
    ctx.reset_coverage()
    assert not ctx.coverage().view("<u8").any()
    cuts = [0, 41, 230, len(recs)]
    for a, b in zip(cuts, cuts[1:]):
        ctx.set_history(hist(a))
        ctx.classify(D.make_reads(recs[a:b]))
    assert as_tuples(ctx.coverage()) == one
    ctx.close()
    # two input slots: the second batch staged while the first runs, the coverage fetched between them
    ctx = D.Ctx(idx, 0, input_slots=2)
    ctx.enable_coverage()
    parts = [D.make_reads(recs[:150]), D.make_reads(recs[150:])]
    ctx.select_slot(0); ctx.set_history(0); ctx.upload(parts[0])
    ctx.select_slot(1); ctx.set_history(hist(150)); ctx.upload(parts[1])
    ctx.select_slot(0); ctx.run(); ctx.fetch()
    mid = as_tuples(ctx.coverage())
    ctx.select_slot(1); ctx.run(); ctx.fetch()
    assert as_tuples(ctx.coverage()) == one and mid != one and sum(x[0] for x in mid) > 0
    ctx.enable_coverage(False)
    with pytest.raises(D.DsbError) as e:
        ctx.coverage()
    assert e.value.code == D.DSB_EINVAL
    ctx.close(); idx.close()


@pytest.mark.gpu
def test_coverage_several_contexts(demo, tmp_path, monkeypatch):
    import desamba_amd as D
    idx = D.Index(demo["index"])
    recs = D.read_fastq(os.path.join(SYNTH, "ont20k.fq")) + D.read_fastq(os.path.join(SYNTH, "pb.fq")) + D.read_fastq(os.path.join(SYNTH, "ngs_e14.fq"))
    ctx = D.Ctx(idx, 0)
    ctx.enable_coverage()
    ctx.classify(D.make_reads(recs))
    one = as_tuples(ctx.coverage())
    ctx.close()
    monkeypatch.setenv("DSB_SHARD_CHUNK_READS", "30")        # (read when the contexts are made: many chunks on both)
    m = D.Multi(idx, [0, 0])
    with pytest.raises(D.DsbError) as e:
        m.coverage()
    assert e.value.code == D.DSB_EINVAL
    m.enable_coverage()
    m.classify(D.make_reads(recs))
    assert min(m.last_calls()) > 0
    assert as_tuples(m.coverage()) == one
    assert as_tuples(m.coverage()) == one
    m.close()
    monkeypatch.delenv("DSB_SHARD_CHUNK_READS")
    files = [os.path.join(SYNTH, n + ".fq") for n in ("ont20k", "pb", "ngs_e14")]
    env = {"DSB_CLI_BATCH_KB": "128"}
    cli(tmp_path, files, ["--coverage", str(tmp_path / "g0.tsv")], tag="g0", env=env)
    cli(tmp_path, files, ["-g", "0,0", "--coverage", str(tmp_path / "g00.tsv")], tag="g00", env=env)
    names, lens = ref_table(idx)
    assert (tmp_path / "g0.tsv").read_bytes() == (tmp_path / "g00.tsv").read_bytes() == table(names, lens, one)
    idx.close()


@pytest.mark.gpu
def test_cli_outputs_unchanged_by_coverage(demo, tmp_path):
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
    cov = lambda tag: ["--coverage", str(tmp_path / (tag + ".tsv"))]
    tax = lambda tag: ["--taxonomy", NODES, "--report", str(tmp_path / (tag + ".report"))]
    sam = {}
    sam["plain"] = cli(tmp_path, files, [], "plain", env)
    sam["cov"] = cli(tmp_path, files, cov("cov"), "cov", env)
    sam["tax"] = cli(tmp_path, files, tax("tax"), "tax", env)
    sam["taxcov"] = cli(tmp_path, files, tax("taxcov") + cov("taxcov"), "taxcov", env)
    assert sam["plain"] == open(os.path.join(SYNTH, "multi6.ubfree.sam"), "rb").read()
    assert sam["cov"] == sam["tax"] == sam["taxcov"] == sam["plain"]
    assert (tmp_path / "tax.report").read_bytes() == (tmp_path / "taxcov.report").read_bytes() != b""
    des = cli(tmp_path, files, ["-f", "DES_FULL"], "des", env)
    des_cov = cli(tmp_path, files, ["-f", "DES_FULL"] + cov("descov"), "descov", env)
    assert des == des_cov
    c = (tmp_path / "cov.tsv").read_bytes()
    assert c.count(b"\n") > 10 and c == (tmp_path / "taxcov.tsv").read_bytes() == (tmp_path / "descov.tsv").read_bytes()


@pytest.mark.gpu
def test_coverage_strain_index(strain, tmp_path):
    import desamba_amd as D
    fq = tmp_path / "long.fq"
    subprocess.check_call([os.path.join(ROOT, "tools", "readsim"), strain["index"], str(fq), "384", "50000", "0.15", "8181", "ont"])
    idx = D.Index(strain["index"])
    names, lens = ref_table(idx)
    assert len(lens) >= 10 and min(lens) > 100000           # (4.4 Mbp in 15 genomes: references of a hundred thousand words and more)
    recs = D.read_fastq(str(fq)) + D.read_fastq(strain["fastq"])
    ctx = D.Ctx(idx, 0)
    ctx.enable_coverage()
    res = ctx.classify(D.make_reads(recs), strict=False)
    exp = accumulate(idx.n_ref, counted_records(res, len(recs)), lens)
    got = as_tuples(ctx.coverage())
    assert got == exp
    assert sum(1 for g in got if g[1] > 50000) >= 5
    ctx.close(); idx.close()
