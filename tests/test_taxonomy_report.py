"""Per-read taxa on the GPU (k_read_taxon) and the abundance report of a run (classify --taxonomy --report / --report-base,
dsb_report_*): the report must equal what `deSAMBA analysis ana_meta[_base]` prints for the SAM of the same run, without the
leading "Current read <SAM>.temp\\t<SAM>.temp\\t" -- checked against the reference's printouts of the golden read sets
(tests/golden/analysis/*.ubfree.ana_meta[_base].txt) and against the two-step pipeline on the run's own SAM."""
import gzip
import os
import random
import shutil
import subprocess
import zlib

import pytest

from conftest import GOLDEN, ROOT
from reductions_lib import nodes_table, walk_golden_sam

CLI = os.path.join(ROOT, "desamba_amd", "bin", "deSAMBA")
ANA = os.path.join(GOLDEN, "analysis")
NODES = os.path.join(ANA, "nodes.dmp")
SYNTH = os.path.join(GOLDEN, "synth")


def strip_prefix(text):
    """analysis prints 'Current read <SAM>.temp\\t<SAM>.temp\\t' first; the in-run report leaves it out"""
    if not text.startswith(b"Current read "):
        return text
    parts = text.split(b"\t", 2)
    return parts[2] if len(parts) == 3 else b""


def analysis(sam_path, nodes, by_base):
    p = subprocess.run([CLI, "analysis", "ana_meta_base" if by_base else "ana_meta", sam_path, nodes], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr
    return strip_prefix(p.stdout)


def trimmed_nodes(path):
    """a nodes.dmp with taxids missing and a smaller max_tid (500000 + 1 000 000): some reference taxids lie above it"""
    lines = [l for l in open(NODES) if int(l.split("|")[0]) < 500000]
    lines = [l for i, l in enumerate(lines) if i == 0 or i % 5]
    lines.append("500000\t|\t1\t|\tspecies\t|\t\t|\t0\t|\n")
    with open(path, "w") as f:
        f.writelines(lines)
    return str(path)


# ---------------------------------------------------------------- host side (no GPU)

def test_taxonomy_loader(built, tmp_path):
    import desamba_amd as D
    T = D.Taxonomy(NODES)
    table = nodes_table(NODES)
    last = int(open(NODES).read().splitlines()[-1].split("|")[0])
    assert T.max_tid == last + 1000000
    for tid in random.Random(3).sample(sorted(table), 60) + [1]:
        assert T.parent(tid) == (0 if tid == 1 else table[tid]), tid
    assert T.parent(T.max_tid - 1) == 0xffffffff and T.parent(T.max_tid + 5) == 0xffffffff
    T.close()
    cyc = tmp_path / "cycle.dmp"
    cyc.write_text("1\t|\t1\t|\tno rank\t|\n7\t|\t8\t|\tgenus\t|\n8\t|\t9\t|\tgenus\t|\n9\t|\t7\t|\tgenus\t|\n")
    with pytest.raises(D.DsbError) as e:
        D.Taxonomy(str(cyc))
    assert e.value.code == D.DSB_EINVAL
    h = D.C.c_void_p()
    assert D.lib().dsb_taxonomy_load_any(str(cyc).encode(), D.C.byref(h)) == 0      # (what analysis uses: it never looked for cycles)
    D.lib().dsb_taxonomy_close(h)
    with pytest.raises(D.DsbError) as e:
        D.Taxonomy(str(tmp_path / "missing.dmp"))
    assert e.value.code == D.DSB_EIO


def make_batch(D, n_ref, rng, names, max_q=2000):
    """hand-built hits: ties in AS between the primary and later records, supplementary and secondary records, a first
    record of score 0, q_ed beyond the read (a '-' in the CIGAR), reads without hits"""
    reads, rrs, hits = [], [], []
    for name in names:
        L = rng.randint(100, max_q)
        kind = rng.random()
        nh = 0 if kind < 0.15 else rng.randint(1, 9)
        first = len(hits)
        top = rng.choice([0, 80, 200, 200, 350]) if kind < 0.3 else rng.choice([80, 200, 350])
        for k in range(nh):
            h = D.DsbHit()
            h.ref_ID = rng.randrange(n_ref) if rng.random() > 0.02 else n_ref + 3
            q0 = rng.randint(0, L // 2)
            h.q_st, h.q_ed = q0, (L + 1 if rng.random() < 0.1 else rng.randint(q0 + 1, L))
            h.t_st = rng.randint(0, 10000); h.t_ed = h.t_st + (h.q_ed - h.q_st)
            h.sum_score = top if k == 0 else rng.choice([top, top, top - 3, max(top - 10, 0), 60])
            h.direction = rng.randint(0, 1); h.primary = 1 if k == 0 else rng.choice([2, 3])
            h.pri_index = 0 if k == 0 else rng.choice([0, 1, 1, 2, 3, 5, 6, 9])
            hits.append(h)
        rr = D.DsbReadResult(); rr.first = first if nh else 0; rr.n = nh
        rrs.append(rr)
        reads.append((name, b"A" * L, b"I" * L))
    return reads, rrs, hits


def as_result(D, rrs, hits):
    R = (D.DsbReadResult * max(len(rrs), 1))(*rrs)
    H = (D.DsbHit * max(len(hits), 1))(*hits) if hits else (D.DsbHit * 1)()
    res = D.DsbResult(); res.reads = D.C.cast(R, D.C.POINTER(D.DsbReadResult)); res.hits = D.C.cast(H, D.C.POINTER(D.DsbHit)); res.n_hits = len(hits)
    res._keep = (R, H)
    return res


@pytest.mark.parametrize("nodes", ["golden", "trimmed"])
@pytest.mark.parametrize("max_sec", [0, 1, 5])
@pytest.mark.parametrize("case", ["mixed", "dup_names", "last_classified", "last_unclassified", "empty"])
def test_host_report_equals_analysis_of_the_sam(demo, tmp_path, nodes, max_sec, case):
    """dsb_report_add with taxa = NULL (every read walked on the host over the records dsb_format_sam writes for it) against
    `deSAMBA analysis` on that SAM, fed in batches of unequal size"""
    import desamba_amd as D
    nodes_path = NODES if nodes == "golden" else trimmed_nodes(tmp_path / "nodes.dmp")
    idx = D.Index(demo["index"])
    rng = random.Random(zlib.crc32(("%s %d %s" % (nodes, max_sec, case)).encode()))
    n = {"mixed": 300, "dup_names": 300, "last_classified": 40, "last_unclassified": 40, "empty": 0}[case]
    names = [b"r%d" % i for i in range(n)]
    if case == "dup_names":
        names = [b"r%d" % (i // 3 if i % 7 else i // 2) for i in range(n)]
    reads, rrs, hits = make_batch(D, idx.n_ref, rng, names)
    if case in ("last_classified", "last_unclassified") and n:
        last = rrs[-1]
        if case == "last_unclassified":
            last.n = 0
        elif last.n == 0:
            h = D.DsbHit(); h.ref_ID = 0; h.q_st, h.q_ed = 0, 50; h.sum_score = 200; h.primary = 1
            last.first, last.n = len(hits), 1; hits.append(h)
    T = D.Taxonomy(nodes_path)
    rep = D.Report(T)
    sam = []
    cuts = sorted(set([0, n] + [rng.randint(0, n) for _ in range(4)]))
    for a, b in zip(cuts, cuts[1:]):
        sub_rr, sub_h = [], []
        for rr in rrs[a:b]:
            c = D.DsbReadResult(); c.first = len(sub_h); c.n = rr.n
            sub_h.extend(hits[rr.first:rr.first + rr.n]); sub_rr.append(c)
        rd = D.make_reads(reads[a:b]); res = as_result(D, sub_rr, sub_h)
        rep.add(idx, rd, res, None, max_sec)
        sam.append(D.format_sam(idx, rd, res, max_sec))
    (tmp_path / "run.sam").write_bytes(b"".join(sam))
    for by_base in (False, True):
        exp = analysis(str(tmp_path / "run.sam"), nodes_path, by_base)
        assert rep.text(by_base) == exp, (case, by_base)
        if n == 0:
            assert exp == b""
    rep.close(); T.close(); idx.close()


def test_report_without_taxonomy_is_refused(built, tmp_path):
    p = subprocess.run([CLI, "classify", "--report", str(tmp_path / "r.txt"), os.path.join(ROOT, "data", "demo", "index"), os.path.join(SYNTH, "pb.fq")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 1 and b"--taxonomy" in p.stderr and not (tmp_path / "r.txt").exists()


# ---------------------------------------------------------------- on the GPU

def cli_run(tmp_path, files, extra=(), nodes=NODES, tag="run", env=None):
    out, r, rb = tmp_path / (tag + ".sam"), tmp_path / (tag + ".report"), tmp_path / (tag + ".report_base")
    e = dict(os.environ); e.update(env or {})
    p = subprocess.run([CLI, "classify", "--taxonomy", nodes, "--report", str(r), "--report-base", str(rb)] + list(extra) +
                       [os.path.join(ROOT, "data", "demo", "index")] + [str(f) for f in files] + ["-o", str(out)], stderr=subprocess.PIPE, env=e)
    assert p.returncode == 0, p.stderr
    return out, r.read_bytes(), rb.read_bytes()


def golden(name, by_base):
    return strip_prefix(open(os.path.join(ANA, "%s.ubfree.ana_meta%s.txt" % (name, "_base" if by_base else "")), "rb").read())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pb", "ngs150", "ont20k", "appc"])
def test_cli_report_equals_the_reference_s(demo, tmp_path, name):
    out, r, rb = cli_run(tmp_path, [os.path.join(SYNTH, name + ".fq")])
    assert r == golden(name, False) and rb == golden(name, True)
    assert out.read_bytes() == open(os.path.join(SYNTH, name + ".ubfree.sam"), "rb").read()


@pytest.mark.gpu
def test_cli_report_many_batches_files_and_gzip(demo, tmp_path):
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
    out, r, rb = cli_run(tmp_path, files, env={"DSB_CLI_BATCH_KB": "256"})
    assert out.read_bytes() == open(os.path.join(SYNTH, "multi6.ubfree.sam"), "rb").read()
    assert r == golden("multi6", False) and rb == golden("multi6", True)


def two_step(tmp_path, sam, nodes=NODES):
    return analysis(str(sam), nodes, False), analysis(str(sam), nodes, True)


@pytest.mark.gpu
def test_cli_report_equals_two_step_pipeline(demo, tmp_path):
    multi4 = [os.path.join(SYNTH, n + ".fq") for n in ("pb", "ngs_e14", "ngs150", "appc")]
    # -g 0,0: two workers, small batches, the ordered writer
    out, r, rb = cli_run(tmp_path, multi4, ["-g", "0,0"], tag="g00", env={"DSB_CLI_BATCH_KB": "128"})
    assert out.read_bytes() == open(os.path.join(SYNTH, "multi4.ubfree.sam"), "rb").read()
    assert (r, rb) == two_step(tmp_path, out)
    # every record twice (adjacent reads of one name), cut into batches of 64 KB: duplicates straddle batch boundaries
    dup = tmp_path / "dup.fq"
    recs = open(os.path.join(SYNTH, "pb.fq"), "rb").read().splitlines(True)
    with open(dup, "wb") as f:
        for i in range(0, len(recs), 4):
            f.write(b"".join(recs[i:i + 4]) * 2)
    out, r, rb = cli_run(tmp_path, [dup], tag="dup", env={"DSB_CLI_BATCH_KB": "64"})
    assert (r, rb) == two_step(tmp_path, out)
    assert out.read_bytes().count(b"\n") == 2 * open(os.path.join(SYNTH, "pb.ubfree.sam"), "rb").read().count(b"\n")
    # -r 0 / -r 1, and -f DES -r 1 (whose report is that of -f SAM -r 1)
    for rr in ("0", "1"):
        out, r, rb = cli_run(tmp_path, multi4, ["-r", rr], tag="r" + rr)
        assert (r, rb) == two_step(tmp_path, out), rr
    _, rd, rbd = cli_run(tmp_path, multi4, ["-f", "DES", "-r", "1"], tag="des")
    assert (rd, rbd) == (r, rb)
    # a trimmed nodes.dmp: taxids missing, a smaller max_tid
    tn = trimmed_nodes(tmp_path / "trimmed.dmp")
    out, r, rb = cli_run(tmp_path, multi4, nodes=tn, tag="trim")
    assert (r, rb) == two_step(tmp_path, out, tn)
    # an empty input file: empty reports
    (tmp_path / "empty.fq").write_bytes(b"")
    out, r, rb = cli_run(tmp_path, [tmp_path / "empty.fq"], tag="empty")
    assert out.read_bytes() == b"" and r == b"" and rb == b""


@pytest.mark.gpu
def test_python_taxa_and_report(demo, tmp_path):
    import numpy as np
    import desamba_amd as D
    idx = D.Index(demo["index"])
    T = D.Taxonomy(NODES)
    table = nodes_table(NODES)
    ctx = D.Ctx(idx, 0)
    reads = D.make_reads(D.read_fastq(os.path.join(SYNTH, "pb.fq")))
    ctx.classify(reads)
    with pytest.raises(D.DsbError) as e:
        ctx.taxa()
    assert e.value.code == D.DSB_EINVAL
    ctx.set_taxonomy(T)
    for name in ("pb", "ngs150", "ont20k", "appc"):
        recs = D.read_fastq(os.path.join(SYNTH, name + ".fq"))
        exp = walk_golden_sam(os.path.join(SYNTH, name + ".ubfree.sam"), table, T.max_tid)
        assert len(exp) == len(recs)
        ctx.reset_history()
        reads = D.make_reads(recs)
        res = ctx.classify(reads)
        got = ctx.taxa()
        assert got.dtype == np.uint32 and list(got) == exp, name
        assert (got > 0).sum() > len(recs) // 4
        # the report through the Python object, fed the device records: the CLI's report of the same file
        rep = D.Report(T)
        rep.add(idx, reads, res, ctx.taxa(records=True), 5)
        _, r, rb = cli_run(tmp_path, [os.path.join(SYNTH, name + ".fq")], tag=name)
        assert rep.text() == r and rep.text(by_base=True) == rb, name
        rep.close()
        # another batch split
        ctx.reset_history()
        parts = []
        for s in range(0, len(recs), 97):
            ctx.set_history(max([len(x[1]) for x in recs[:s]], default=0))
            ctx.classify(D.make_reads(recs[s:s + 97]))
            parts.extend(ctx.taxa())
        assert parts == exp, name
    m = D.Multi(idx, [0, 0])
    m.set_taxonomy(T)
    recs = D.read_fastq(os.path.join(SYNTH, "appc.fq"))
    m.classify(D.make_reads(recs))
    assert list(m.taxa()) == walk_golden_sam(os.path.join(SYNTH, "appc.ubfree.sam"), table, T.max_tid)
    m.close(); ctx.set_taxonomy(None); ctx.close(); T.close(); idx.close()
