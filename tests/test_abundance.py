"""Per-reference abundance by EM (k_em_collect, the class build and k_em_class / k_em_ref; dsb_*_abundance, classify --abundance;
DESIGN 2.10).  A numpy EM written from the definition is the yardstick: candidate sets are built from the reference's golden
DES_FULL (every hit with its AS) or from the run's own hits, and the GPU's counts must equal it exactly and its estimates within a
relative 1e-9.  The doubles themselves must be bitwise equal across batch splits, input slots, contexts and runs."""
import gzip
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT
from reductions_lib import candidate_set, check_against, classes_of, em, sets_from_result

CLI = os.path.join(ROOT, "desamba_amd", "bin", "deSAMBA")
SYNTH = os.path.join(GOLDEN, "synth")
NODES = os.path.join(GOLDEN, "analysis", "nodes.dmp")
HEADER = b"#rname\ttaxid\tlength\tnumreads\tuniqreads\testreads\treadshare\tcopyshare\n"


# ---------------------------------------------------------------- the definition, in numpy

def taxid_of(name):
    """the second '|' field as strtok / strtoul read it, 0 if absent"""
    f = [x for x in name.split("|") if x]
    if len(f) < 2:
        return 0
    d = ""
    for ch in f[1].lstrip(" \t"):
        if not ch.isdigit():
            break
        d += ch
    return int(d) if d else 0


def table(names, lens, ab, summ):
    out = [b"#reads=%d\tclassified=%d\tclasses=%d\titerations=%d\tconverged=%s\tmax_change=%s\tmin_frac=%s\n" % (
        summ["reads"], summ["classified"], summ["classes"], summ["iterations"], b"yes" if summ["converged"] else b"no",
        (b"%.6e" % summ["max_change"]), (b"%.3f" % (summ["min_permille"] / 1000.0))), HEADER]
    for r, x in enumerate(ab):
        if x["numreads"]:
            out.append(b"%s\t%d\t%d\t%d\t%d\t%.3f\t%.6e\t%.6e\n" % (names[r].encode(), taxid_of(names[r]), lens[r], x["numreads"], x["uniqreads"],
                                                                  x["est_reads"], x["read_share"], x["copy_share"]))
    return b"".join(out)


def ref_table(idx):
    n = idx.n_ref
    return [idx.ref_name(r) for r in range(n)], [idx.ref_len(r) for r in range(n)]


# ---------------------------------------------------------------- host side (no GPU)

def test_em_closed_form():
    # {A}: 70, {B}: 30, {A, B}: 100 with L_A = L_B: the shared reads split 70:30 at the fixed point -> 140 / 60
    a, it, conv, chg = em({(0,): 70, (1,): 30, (0, 1): 100}, [1000, 1000], tol=1e-9)
    assert conv and chg < 1e-9 and it > 5
    assert abs(200 * a[0] - 140) < 1e-6 and abs(200 * a[1] - 60) < 1e-6
    # a reference in no class stays 0; a class of one reference alone keeps its reads
    a, it, conv, _ = em({(2,): 10}, [5, 5, 5])
    assert list(a) == [0.0, 0.0, 1.0] and it == 1 and conv
    # the candidate sets
    assert candidate_set([(3, 100), (1, 96), (1, 50), (7, 94), (9, 100)], 9, 950) == (1, 3)
    assert candidate_set([(3, 100), (1, 96)], 9, 1000) == (3,)
    assert candidate_set([(12, 100)], 9, 950) == ()


def test_abundance_format(demo):
    import numpy as np
    import desamba_amd as D
    idx = D.Index(demo["index"])
    names, lens = ref_table(idx)
    n = idx.n_ref
    ab = np.zeros(n, dtype=D.ABUNDANCE_DTYPE)
    ab[0] = (12, 3, 10.25, 0.125, 3.5e-7)
    ab[4] = (1, 1, 1.0 / 3.0, 1.0 / 7.0, 1e-300)
    ab[n - 1] = (5, 0, 0.0, 0.0, 0.0)
    ab[2] = (0, 0, 9.0, 0.5, 0.5)                        # numreads 0: no row
    summ = dict(reads=100, classified=18, classes=7, iterations=33, converged=1, max_change=0.0078125, min_permille=950)
    got = D.format_abundance(idx, ab, summ)
    assert got == table(names, lens, ab, summ)
    lines = got.splitlines()
    assert lines[0] == b"#reads=100\tclassified=18\tclasses=7\titerations=33\tconverged=yes\tmax_change=7.812500e-03\tmin_frac=0.950"
    assert lines[1] + b"\n" == HEADER and len(lines) == 5
    assert lines[2].split(b"\t")[3:] == [b"12", b"3", b"10.250", b"1.250000e-01", b"3.500000e-07"]
    assert lines[3].split(b"\t")[5:] == [b"0.333", b"1.428571e-01", b"1.000000e-300"]
    assert int(lines[2].split(b"\t")[1]) == taxid_of(names[0]) > 0
    summ["converged"] = 0
    assert b"converged=no" in D.format_abundance(idx, ab, summ)
    summ["converged"] = 1
    # a short buffer gives -1
    s = D.DsbAbundanceSummary(**{f: summ[f] for f in D.SUMMARY_FIELDS})
    buf = D.C.create_string_buffer(len(got))
    assert D.lib().dsb_abundance_format(idx.h, ab.ctypes.data_as(D.C.c_void_p), D.C.byref(s), buf, len(got)) == -1
    buf = D.C.create_string_buffer(len(got) + 1)
    assert D.lib().dsb_abundance_format(idx.h, ab.ctypes.data_as(D.C.c_void_p), D.C.byref(s), buf, len(got) + 1) == len(got)
    idx.close()


def test_abundance_null_handles_and_ranges(built):
    import desamba_amd as D
    L = D.lib()
    assert L.dsb_ctx_abundance(None, None, None, None) == D.DSB_EINVAL
    assert L.dsb_multi_abundance(None, None, None, None) == D.DSB_EINVAL
    assert L.dsb_ctx_enable_abundance(None, 1, 950) == D.DSB_EINVAL
    assert L.dsb_ctx_reset_abundance(None) == D.DSB_EINVAL
    assert L.dsb_multi_enable_abundance(None, 1, 950) == D.DSB_EINVAL
    assert L.dsb_abundance_format(None, None, None, None, 0) == -1
    for bad in (0, 0.0004, 1.5, -0.2):
        with pytest.raises(ValueError):
            D._permille(bad)
    assert D._permille(1.0) == 1000 and D._permille(0.95) == 950 and D._permille(0.001) == 1


def test_cli_refuses_bad_min_frac(built, tmp_path):
    for bad in ("0", "1.5", "abc", "-0.1", "0.95x", "0.0001"):
        p = subprocess.run([CLI, "classify", "--abundance", str(tmp_path / "a.tsv"), "--abundance-min-frac", bad, "nowhere", "nothing.fq"],
                           stderr=subprocess.PIPE, stdout=subprocess.PIPE)
        assert p.returncode != 0 and b"--abundance-min-frac" in p.stderr, bad


# ---------------------------------------------------------------- on the GPU

def cli(tmp_path, files, extra=(), tag="run", env=None, index=None):
    out = tmp_path / (tag + ".out")
    e = dict(os.environ); e.update(env or {})
    p = subprocess.run([CLI, "classify"] + list(extra) + [index or os.path.join(ROOT, "data", "demo", "index")] + [str(f) for f in files] + ["-o", str(out)],
                       stderr=subprocess.PIPE, env=e)
    assert p.returncode == 0, p.stderr
    return out.read_bytes()


def golden_desfull_sets(name, names, permille):
    """every read's candidate set from the reference's DES_FULL golden output (all hits with their AS)"""
    ref_id = {n: r for r, n in enumerate(names)}
    sets, cur = [], None
    for line in open(os.path.join(SYNTH, name + ".desfull.ubfree.txt"), "rb").read().splitlines():
        if not line.strip():
            if cur is not None:
                sets.append(candidate_set(cur, len(names), permille))
            cur = None
            continue
        if cur is None:
            cur = []
            continue
        f = line.split()
        cur.append((ref_id[f[3].decode()], int(f[8])))
    if cur is not None:
        sets.append(candidate_set(cur, len(names), permille))
    return sets


@pytest.mark.gpu
def test_abundance_equals_the_reference_s_hits(demo):
    import desamba_amd as D
    idx = D.Index(demo["index"])
    names, lens = ref_table(idx)
    recs = D.read_fastq(os.path.join(SYNTH, "ngs150.fq"))
    for frac in (0.95, 1.0):
        sets = golden_desfull_sets("ngs150", names, int(frac * 1000 + 0.5))
        assert len(sets) == len(recs)
        ctx = D.Ctx(idx, 0)
        ctx.enable_abundance(min_frac=frac)
        ctx.classify(D.make_reads(recs))
        ab, summ = ctx.abundance(max_iter=200, tol=0)
        assert summ["reads"] == len(recs) and summ["min_permille"] == int(frac * 1000 + 0.5)
        check_against(ab, summ, sets, lens, "ngs150 %g" % frac)
        assert summ["classes"] > 10 and sum(1 for s in sets if len(s) > 1) > 0
        ctx.close()
    idx.close()


@pytest.mark.gpu
def test_abundance_equals_host_em_on_own_hits(demo, strain, tmp_path):
    import desamba_amd as D
    idx = D.Index(demo["index"])
    names, lens = ref_table(idx)
    ctx = D.Ctx(idx, 0)
    for name in ("pb", "ont20k", "heavy"):
        recs = D.read_fastq(os.path.join(SYNTH, name + ".fq"))
        for frac in (1.0, 0.95):
            p = int(frac * 1000 + 0.5)
            ctx.enable_abundance(min_frac=frac)                  # (on again: emptied)
            ctx.reset_history()
            res = ctx.classify(D.make_reads(recs), strict=False)
            sets = sets_from_result(res, len(recs), idx.n_ref, p)
            ab, summ = ctx.abundance(max_iter=200, tol=0)
            check_against(ab, summ, sets, lens, "%s %g" % (name, frac))
    ctx.close(); idx.close()
    # 50-kbp reads of the strain index (references of a hundred kbp and more)
    fq = tmp_path / "long.fq"
    subprocess.check_call([os.path.join(ROOT, "tools", "readsim"), strain["index"], str(fq), "256", "50000", "0.12", "4242", "ont"])
    idx = D.Index(strain["index"])
    names, lens = ref_table(idx)
    recs = D.read_fastq(str(fq))
    ctx = D.Ctx(idx, 0)
    for frac in (1.0, 0.95):
        ctx.enable_abundance(min_frac=frac)
        ctx.reset_history()
        res = ctx.classify(D.make_reads(recs), strict=False)
        sets = sets_from_result(res, len(recs), idx.n_ref, int(frac * 1000 + 0.5))
        ab, summ = ctx.abundance(max_iter=200, tol=0)
        check_against(ab, summ, sets, lens, "strain %g" % frac)
        if frac == 0.95:
            # the default stop: converged within max_iter, the state after the iteration that met tol
            ab2, s2 = ctx.abundance()
            a, it, conv, chg = em(classes_of(sets), lens)
            assert s2["iterations"] == it and s2["converged"] == int(conv) and conv
            assert abs(s2["max_change"] - chg) <= 1e-9 * max(chg, 1e-12) + 1e-15
    ctx.close(); idx.close()


def mutate(rng, seq, err):
    """readsim's error model (profile ont): per source base at rate err, 35 % deletion, 40 % substitution (uniform over ACGT,
    may be silent), 25 % insertion after the base"""
    import numpy as np
    n = len(seq)
    u = rng.random(n)
    ev = rng.random(n)
    hit = u < err
    dele = hit & (ev < 0.35)
    sub = hit & (ev >= 0.35) & (ev < 0.75)
    ins = hit & (ev >= 0.75)
    s = seq.copy()
    s[sub] = rng.integers(0, 4, int(sub.sum()))
    keep = ~dele
    cnt = keep.astype(np.int64) + ins
    out = np.repeat(s, cnt)
    # the inserted base follows its source base: the second copy of each inserted position is replaced
    ends = np.cumsum(cnt) - 1
    pos = ends[ins & keep]
    out[pos] = rng.integers(0, 4, len(pos))
    return out


def decode(codes):
    import numpy as np
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.asarray(codes, dtype=np.int64)].tobytes()


def revcomp(codes):
    return (3 - codes[::-1])


def sample(rng, genome, n, length, err, tag):
    out = []
    for i in range(n):
        st = int(rng.integers(0, len(genome) - length))
        s = mutate(rng, genome[st:st + length], err)
        if rng.random() < 0.5:
            s = revcomp(s)
        out.append(("%s_%d_%d" % (tag, i, st), decode(s), b"5" * len(s)))
    return out


def write_fasta(path, recs):
    with open(path, "wb") as f:
        for name, codes in recs:
            seq = decode(codes)
            f.write(b">" + name.encode() + b"\n")
            for k in range(0, len(seq), 80):
                f.write(seq[k:k + 80] + b"\n")


@pytest.mark.gpu
def test_abundance_known_truth(built, tmp_path):
    """A, B = A with its second half replaced, and an unrelated C; reads 70:30 from A and B: the reads of the shared half tie"""
    import numpy as np
    import desamba_amd as D
    rng = np.random.default_rng(20261016)
    A = rng.integers(0, 4, 200000).astype(np.uint8)
    B = A.copy(); B[100000:] = rng.integers(0, 4, 100000)
    Cg = rng.integers(0, 4, 120000).astype(np.uint8)
    write_fasta(str(tmp_path / "abc.fa"), [("tid|101|A", A), ("tid|102|B", B), ("tid|103|C", Cg)])
    D.build_index(str(tmp_path / "abc.fa"), str(tmp_path / "index"))
    recs = sample(rng, A, 2800, 5000, 0.08, "A") + sample(rng, B, 1200, 5000, 0.08, "B") + sample(rng, Cg, 300, 5000, 0.08, "C")
    order = rng.permutation(len(recs))
    recs = [recs[i] for i in order]
    idx = D.Index(str(tmp_path / "index"))
    names, lens = ref_table(idx)
    assert names == ["tid|101|A", "tid|102|B", "tid|103|C"]
    ctx = D.Ctx(idx, 0)
    ctx.enable_abundance()
    res = ctx.classify(D.make_reads(recs), strict=False)
    ab, summ = ctx.abundance()
    assert summ["converged"] and summ["classified"] > 0.97 * len(recs)
    est = ab["est_reads"]
    share = est[0] / (est[0] + est[1])
    prim = [0, 0, 0]
    for i in range(len(recs)):
        rr = res.reads[i]
        if rr.n:
            prim[res.hits[rr.first].ref_ID] += 1
    prim_share = prim[0] / (prim[0] + prim[1])
    print("A's share of A + B: truth 0.700, EM %.4f, primary records only %.4f (%d classes, %d iterations)" % (share, prim_share, summ["classes"], summ["iterations"]))
    assert abs(share - 0.70) <= 0.04
    assert abs(prim_share - 0.70) > abs(share - 0.70)
    assert ab["numreads"][0] > ab["uniqreads"][0] > 0 and ab["uniqreads"][1] > 0
    assert abs(est[2] - 300) < 15
    ctx.close(); idx.close()


def det_reads():
    import desamba_amd as D
    return D.read_fastq(os.path.join(SYNTH, "pb.fq")) + D.read_fastq(os.path.join(SYNTH, "ngs150.fq")) + D.read_fastq(os.path.join(SYNTH, "ont20k.fq"))


@pytest.mark.gpu
def test_abundance_bitwise_independent_of_batches_slots_contexts(demo, monkeypatch):
    import desamba_amd as D
    idx = D.Index(demo["index"])
    recs = det_reads()
    hist = lambda s: max([len(x[1]) for x in recs[:s]], default=0)
    ctx = D.Ctx(idx, 0)
    with pytest.raises(D.DsbError) as e:
        ctx.abundance()
    assert e.value.code == D.DSB_EINVAL
    with pytest.raises(D.DsbError) as e:
        ctx.reset_abundance()
    assert e.value.code == D.DSB_EINVAL
    ctx.enable_abundance()
    ctx.classify(D.make_reads(recs))
    one, s1 = ctx.abundance()
    assert s1["classified"] > 100 and s1["reads"] == len(recs)
    again, s_again = ctx.abundance()                            # fetching changes nothing
    assert again.tobytes() == one.tobytes() and s_again == s1
    for bad in (dict(max_iter=0), dict(tol=-1.0), dict(tol=float("nan"))):
        with pytest.raises(D.DsbError) as e:
            ctx.abundance(**bad)
        assert e.value.code == D.DSB_EINVAL
    # three batches
    ctx.reset_abundance()
    empty, se = ctx.abundance()
    assert not empty["numreads"].any() and not empty["est_reads"].any() and se["classified"] == se["reads"] == se["classes"] == 0
    cuts = [0, 41, 230, len(recs)]
    for a, b in zip(cuts, cuts[1:]):
        ctx.set_history(hist(a))
        ctx.classify(D.make_reads(recs[a:b]))
    three, s3 = ctx.abundance()
    assert three.tobytes() == one.tobytes() and s3 == s1
    ctx.close()
    # a second identical run
    ctx = D.Ctx(idx, 0)
    ctx.enable_abundance()
    ctx.classify(D.make_reads(recs))
    rep, sr = ctx.abundance()
    assert rep.tobytes() == one.tobytes() and sr == s1
    ctx.close()
    # two input slots, fetched between them
    ctx = D.Ctx(idx, 0, input_slots=2)
    ctx.enable_abundance()
    parts = [D.make_reads(recs[:150]), D.make_reads(recs[150:])]
    ctx.select_slot(0); ctx.set_history(0); ctx.upload(parts[0])
    ctx.select_slot(1); ctx.set_history(hist(150)); ctx.upload(parts[1])
    ctx.select_slot(0); ctx.run(); ctx.fetch()
    mid, sm = ctx.abundance()
    ctx.select_slot(1); ctx.run(); ctx.fetch()
    two, s2 = ctx.abundance()
    assert two.tobytes() == one.tobytes() and s2 == s1 and sm["reads"] == 150
    ctx.enable_abundance(False)
    with pytest.raises(D.DsbError) as e:
        ctx.abundance()
    assert e.value.code == D.DSB_EINVAL
    ctx.close()
    # two contexts on one device, many chunks on both
    monkeypatch.setenv("DSB_SHARD_CHUNK_READS", "30")
    m = D.Multi(idx, [0, 0])
    with pytest.raises(D.DsbError) as e:
        m.abundance()
    assert e.value.code == D.DSB_EINVAL
    m.enable_abundance()
    m.classify(D.make_reads(recs))
    assert min(m.last_calls()) > 0
    mm, smm = m.abundance()
    assert mm.tobytes() == one.tobytes() and smm == s1
    m.reset_abundance()
    assert m.abundance()[1]["classified"] == 0
    m.close()
    idx.close()


@pytest.mark.gpu
def test_cli_abundance_tables_and_unchanged_outputs(demo, tmp_path):
    import desamba_amd as D
    names_ = ["ont20k", "ngs_e14", "pb", "appc", "wrapq", "ngs150"]
    files = []
    for i, n in enumerate(names_):
        src = os.path.join(SYNTH, n + ".fq")
        if i % 2:
            dst = tmp_path / (n + ".fq.gz")
            with gzip.open(dst, "wb") as f:
                f.write(open(src, "rb").read())
            files.append(dst)
        else:
            files.append(src)
    env = {"DSB_CLI_BATCH_KB": "128"}
    ab = lambda tag: ["--abundance", str(tmp_path / (tag + ".tsv"))]
    extra = lambda tag: ["--taxonomy", NODES, "--report", str(tmp_path / (tag + ".report")), "--coverage", str(tmp_path / (tag + ".cov"))]
    plain = cli(tmp_path, files, extra("plain"), "plain", env)
    g0 = cli(tmp_path, files, extra("g0") + ab("g0"), "g0", env)
    g00 = cli(tmp_path, files, ["-g", "0,0"] + ab("g00"), "g00", env)
    assert plain == g0 == g00 == open(os.path.join(SYNTH, "multi6.ubfree.sam"), "rb").read()
    assert (tmp_path / "plain.report").read_bytes() == (tmp_path / "g0.report").read_bytes() != b""
    assert (tmp_path / "plain.cov").read_bytes() == (tmp_path / "g0.cov").read_bytes() != b""
    t0, t00 = (tmp_path / "g0.tsv").read_bytes(), (tmp_path / "g00.tsv").read_bytes()
    assert t0 == t00 and t0.count(b"\n") > 10
    des = cli(tmp_path, files, ["-f", "DES_FULL"], "des", env)
    des_ab = cli(tmp_path, files, ["-f", "DES_FULL", "--abundance-min-frac", "1"] + ab("des"), "desab", env)
    assert des == des_ab
    # the table is the library's rendering of the library's numbers: the same reads through the Python API
    idx = D.Index(demo["index"])
    names, lens = ref_table(idx)
    recs = []
    for n in names_:
        recs += D.read_fastq(os.path.join(SYNTH, n + ".fq"))
    ctx = D.Ctx(idx, 0)
    ctx.enable_abundance()
    ctx.classify(D.make_reads(recs), strict=False)
    a, s = ctx.abundance()
    assert table(names, lens, a, s) == t0
    ctx.enable_abundance(min_frac=1.0)
    ctx.reset_history()
    ctx.classify(D.make_reads(recs), strict=False)
    a1, s1 = ctx.abundance()
    assert table(names, lens, a1, s1) == (tmp_path / "des.tsv").read_bytes()
    ctx.close(); idx.close()


@pytest.mark.gpu
def test_abundance_edge_cases(demo, tmp_path):
    import numpy as np
    import desamba_amd as D
    # an empty input
    (tmp_path / "empty.fq").write_bytes(b"")
    cli(tmp_path, [tmp_path / "empty.fq"], ["--abundance", str(tmp_path / "empty.tsv")], "empty")
    assert (tmp_path / "empty.tsv").read_bytes() == (b"#reads=0\tclassified=0\tclasses=0\titerations=0\tconverged=yes\tmax_change=0.000000e+00\t"
                                                     b"min_frac=0.950\n" + HEADER)
    # every read unclassified
    rng = np.random.default_rng(5)
    recs = [("u%d" % i, decode(rng.integers(0, 4, 3000)), b"5" * 3000) for i in range(40)]
    with open(tmp_path / "rand.fq", "wb") as f:
        for n, s, q in recs:
            f.write(b"@" + n.encode() + b"\n" + s + b"\n+\n" + q + b"\n")
    cli(tmp_path, [tmp_path / "rand.fq"], ["--abundance", str(tmp_path / "rand.tsv")], "rand")
    assert (tmp_path / "rand.tsv").read_bytes().startswith(b"#reads=40\tclassified=0\tclasses=0\titerations=0\tconverged=yes")
    assert (tmp_path / "rand.tsv").read_bytes().count(b"\n") == 2


@pytest.mark.gpu
def test_abundance_identical_copies(built, tmp_path):
    """80 identical copies of one genome under distinct taxids: reads whose sets hold more than 64 references (the second
    selection pass of k_em_collect); the copies must get bitwise-equal estimates"""
    import numpy as np
    import desamba_amd as D
    rng = np.random.default_rng(77)
    G = rng.integers(0, 4, 20000).astype(np.uint8)
    other = rng.integers(0, 4, 40000).astype(np.uint8)
    write_fasta(str(tmp_path / "copies.fa"), [("tid|%d|copy%d" % (500 + i, i), G) for i in range(80)] + [("tid|999|other", other)])
    D.build_index(str(tmp_path / "copies.fa"), str(tmp_path / "index"))
    recs = sample(rng, G, 60, 3000, 0.05, "G") + sample(rng, other, 20, 3000, 0.05, "O")
    idx = D.Index(str(tmp_path / "index"))
    names, lens = ref_table(idx)
    ctx = D.Ctx(idx, 0, max_sec_N=100)
    ctx.enable_abundance()
    res = ctx.classify(D.make_reads(recs), strict=False)
    sets = sets_from_result(res, len(recs), idx.n_ref, 950)
    biggest = max(len(s) for s in sets)
    print("largest candidate set: %d references" % biggest)
    ab, summ = ctx.abundance(max_iter=200, tol=0)
    check_against(ab, summ, sets, lens, "copies")
    got = [ab["est_reads"][r] for r in range(80) if ab["numreads"][r]]
    assert len(set(x.tobytes() for x in got)) == 1
    assert biggest > 64
    ctx.close(); idx.close()
