"""Each read assigned to one reference by its EM posterior (k_em_assign_class / k_em_assign_read behind the solve, the ordinal log,
dsb_*_abundance_assign, dsb_format_assign, classify --abundance-reads).  The yardstick is abundance_assign_lib's
model over the run's own hits and the read_share the same call returned: ref_ID and n_cand equal read for read, posterior within a
relative 1e-12.  The records must be bitwise equal, in input order, across batch splits, input slots, contexts and the CLI."""
import gzip
import os
import subprocess

import pytest

import abundance_assign_lib as M
from conftest import GOLDEN, ROOT
from reductions_lib import sets_from_result

CLI = os.path.join(ROOT, "desamba_amd", "bin", "deSAMBA")
SYNTH = os.path.join(GOLDEN, "synth")
NODES = os.path.join(GOLDEN, "analysis", "nodes.dmp")
NONE_REC = (M.NONE, 0, 0.0)


def ref_lens(idx):
    return [idx.ref_len(r) for r in range(idx.n_ref)]


def as_tuples(recs):
    return [(int(r["ref_ID"]), int(r["n_cand"]), float(r["posterior"])) for r in recs]


# ---------------------------------------------------------------- without a GPU

def test_model_by_hand():
    # {0, 2} with shares 0.5 / 0.25 and lengths 1000 / 250: w = 5e-4, 1e-3 -> reference 2, posterior 2/3
    rec = M.assign_one((0, 2), [0.5, 0.25, 0.25], [1000.0, 1.0, 250.0])
    assert rec[:2] == (2, 2) and rec[2] == 1e-3 / (5e-4 + 1e-3) and not rec[3]
    assert M.assign_one((1, 3), [0, 0.25, 0, 0.25], [1.0, 8.0, 1.0, 8.0])[:3] == (1, 2, 0.5)      # a bitwise tie: the smallest ref_ID
    assert M.assign_one((1, 3), [0, 0.0, 0, 0.0], [1.0, 8.0, 1.0, 8.0])[:3] == (1, 2, 0.0)       # every share underflowed
    assert M.assign_one((), [1.0], [1.0]) == (M.NONE, 0, 0.0, False)
    assert M.assign_one((0, 1), [0.5, 0.5 * (1 + 2e-16)], [1.0, 1.0])[3]                         # one ulp apart: a near-tie
    assert M.assign_one((4,), [0, 0, 0, 0, 0.125], [1.0] * 5)[:3] == (4, 1, 1.0)


def test_format_assign(demo, built, tmp_path):
    import numpy as np
    import build_lib
    import desamba_amd as D
    assert D.C.sizeof(D.DsbReadAssign) == 16 == np.dtype(D.ASSIGN_DTYPE).itemsize and D.DSB_ASSIGN_NONE == M.NONE
    idx = D.Index(demo["index"])
    name0, name3 = idx.ref_name(0), idx.ref_name(3)
    tid = lambda n: int(n.split("|")[1])
    reads = D.make_reads([("r1", b"ACGT" * 10, None), ("r2 with a comment", b"A" * 7, b"5" * 7), ("r3", b"C" * 9, None)])
    recs = np.zeros(3, dtype=D.ASSIGN_DTYPE)
    recs[0] = (3, 2, 2.0 / 3.0)
    recs[1] = (M.NONE, 0, 0.0)
    recs[2] = (0, 1, 1.0)
    got = D.format_assign(idx, reads, recs)
    assert got == ("r1\t%s\t%d\t2\t0.666667\n" % (name3, tid(name3))).encode() + b"r2 with a comment\t*\t0\t0\t0.000000\n" + \
        ("r3\t%s\t%d\t1\t1.000000\n" % (name0, tid(name0))).encode()
    line = got.split(b"\n")[0] + b"\n"
    L = D.lib()
    arg = (idx.h, D.C.byref(reads[0]), recs[0:1].ctypes.data_as(D.C.c_void_p))
    assert L.dsb_format_assign(*arg, D.C.create_string_buffer(len(line)), len(line)) == -1          # a cap that is too small
    assert L.dsb_format_assign(*arg, D.C.create_string_buffer(len(line) + 1), len(line) + 1) == len(line)
    assert L.dsb_format_assign(None, None, None, None, 0) == -1
    recs[0]["ref_ID"] = idx.n_ref                                                                     # no reference of the index
    assert L.dsb_format_assign(*arg, D.C.create_string_buffer(4096), 4096) == -1
    with pytest.raises(ValueError):
        D.format_assign(idx, reads, recs)
    with pytest.raises(ValueError):
        D.format_assign(idx, reads, recs[:2])
    idx.close()
    # a reference name without a taxid: taxid 0 (an index made by the host emulation of the builder)
    rng = np.random.default_rng(3)
    M.write_fasta(str(tmp_path / "two.fa"), [("plain_name", rng.integers(0, 4, 3000)), ("tid|77|named", rng.integers(0, 4, 3000))])
    os.makedirs(tmp_path / "index")
    build_lib.emu_build(str(tmp_path / "two.fa"), str(tmp_path / "index"))
    idx = D.Index(str(tmp_path / "index"))
    assert [idx.ref_name(r) for r in range(idx.n_ref)] == ["plain_name", "tid|77|named"]
    recs = np.zeros(2, dtype=D.ASSIGN_DTYPE)
    recs[0] = (0, 1, 1.0); recs[1] = (1, 2, 0.5)
    assert D.format_assign(idx, D.make_reads([("a", b"ACGT", None), ("b", b"ACGT", None)]), recs) == \
        b"a\tplain_name\t0\t1\t1.000000\nb\ttid|77|named\t77\t2\t0.500000\n"
    idx.close()


def test_assign_null_handles(built):
    import desamba_amd as D
    L = D.lib()
    n = D.C.c_size_t(0)
    assert L.dsb_ctx_set_batch_ordinal(None, 0) == D.DSB_EINVAL
    assert L.dsb_ctx_abundance_assign(None, None, None, None, None, 0, D.C.byref(n)) == D.DSB_EINVAL
    assert L.dsb_multi_abundance_assign(None, None, None, None, None, 0, D.C.byref(n)) == D.DSB_EINVAL


def test_cli_refuses_abundance_reads_without_a_file_and_names_it(built, tmp_path):
    p = subprocess.run([CLI, "classify", "nowhere", os.path.join(SYNTH, "ngs150.fq"), "--abundance-reads"], stderr=subprocess.PIPE, stdout=subprocess.PIPE)
    assert p.returncode != 0 and b"--abundance-reads" in p.stderr
    p = subprocess.run([CLI, "classify", "-h"], stderr=subprocess.PIPE, stdout=subprocess.PIPE)
    assert b"--abundance-reads FILE" in p.stderr and b"in memory" in p.stderr


# ---------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def env(demo):
    import desamba_amd as D
    idx = D.Index(demo["index"])
    yield D, idx, ref_lens(idx)
    idx.close()


def run_and_check(D, ctx, recs, lens, permille, label, strict=False):
    """one batch through ctx (abundance on), the records against the model; abundance() before and after is bitwise the table the
    call itself returned"""
    res = ctx.classify(D.make_reads(recs), strict=strict)
    sets = sets_from_result(res, len(recs), len(lens), permille)
    before, s_before = ctx.abundance()
    ab, summ, got = ctx.abundance_assign()
    after, s_after = ctx.abundance()
    assert before.tobytes() == ab.tobytes() == after.tobytes() and s_before == summ == s_after, label
    want = M.check(got, sets, ab, summ, lens, label)
    return got, sets, ab, summ, want


@pytest.mark.gpu
@pytest.mark.parametrize("frac", [0.95, 1.0])
def test_assign_equals_the_model_on_own_hits(env, frac):
    D, idx, lens = env
    ctx = D.Ctx(idx, 0)
    for name in ("ngs150", "pb", "ont20k"):
        recs = D.read_fastq(os.path.join(SYNTH, name + ".fq"))
        ctx.enable_abundance(min_frac=frac)                      # (on again: store and log emptied)
        ctx.reset_history()
        got, sets, ab, summ, want = run_and_check(D, ctx, recs, lens, int(frac * 1000 + 0.5), "%s %g" % (name, frac))
        assert summ["classified"] > 0 and len(got) == len(recs)
        if name == "ngs150":
            assert any(len(s) > 1 for s in sets)                 # reads with a choice to make
        # two reads of one class: bitwise-equal records
        seen = {}
        for s, r in zip(sets, got):
            assert seen.setdefault(s, r.tobytes()) == r.tobytes()
    ctx.close()


@pytest.mark.gpu
def test_assign_known_truth(built, tmp_path):
    """A, B = A with its second half replaced, and an unrelated C; 2800 : 1200 : 300 reads of 5 kbp (the index and reads of
    test_abundance.py's known-truth case)"""
    import numpy as np
    import desamba_amd as D
    rng = np.random.default_rng(20261016)
    A = rng.integers(0, 4, 200000).astype(np.uint8)
    B = A.copy(); B[100000:] = rng.integers(0, 4, 100000)
    Cg = rng.integers(0, 4, 120000).astype(np.uint8)
    M.write_fasta(str(tmp_path / "abc.fa"), [("tid|101|A", A), ("tid|102|B", B), ("tid|103|C", Cg)])
    D.build_index(str(tmp_path / "abc.fa"), str(tmp_path / "index"))
    recs = M.sample(rng, A, 2800, 5000, 0.08, "A") + M.sample(rng, B, 1200, 5000, 0.08, "B") + M.sample(rng, Cg, 300, 5000, 0.08, "C")
    recs = [recs[i] for i in rng.permutation(len(recs))]
    idx = D.Index(str(tmp_path / "index"))
    lens = ref_lens(idx)
    ctx = D.Ctx(idx, 0)
    ctx.enable_abundance()
    got, sets, ab, summ, want = run_and_check(D, ctx, recs, lens, 950, "A/B/C")
    assert summ["converged"] and summ["classified"] > 0.97 * len(recs)
    n_private = n_shared = n_unclassified = 0
    shared_post = set()
    for (name, _, _), r, w in zip(recs, got, want):
        src, _, st = name.split("_")
        st = int(st)
        if r["ref_ID"] == M.NONE:                                # (the classifier's doing, not the assignment's: counted, bounded above)
            n_unclassified += 1
            continue
        if src == "C" or st >= 100000:                           # wholly inside a private half, or inside C
            assert r["n_cand"] == 1 and r["posterior"] == 1.0 and r["ref_ID"] == "ABC".index(src), name
            n_private += 1
        elif st + 5000 <= 100000:                                # wholly inside the shared half
            assert r["n_cand"] == 2 and r["ref_ID"] == 0, (name, r)
            assert abs(r["posterior"] - w[2]) <= M.REL * w[2] and 0.5 < r["posterior"] < 1.0, (name, r, w)
            shared_post.add(r["posterior"].tobytes())
            n_shared += 1
    print("A/B/C: %d private, %d shared (posterior %r), %d unclassified" % (n_private, n_shared, [np.frombuffer(x)[0] for x in shared_post], n_unclassified))
    assert n_private > 1500 and n_shared > 1500 and len(shared_post) == 1
    per_ref = np.bincount(got["ref_ID"][got["ref_ID"] != M.NONE], minlength=3)
    assert per_ref.sum() == summ["classified"] == len(recs) - n_unclassified
    ctx.close(); idx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("copies", [80, 64, 65])
def test_assign_identical_copies(built, tmp_path, copies):
    """identical copies of one genome under distinct taxids (test_abundance.py's fixture shape): 80 is the set longer than a
    wavefront, 64 and 65 the two sides of that boundary.  Equal shares and lengths: bitwise-equal weights, so the smallest ref_ID."""
    import numpy as np
    import desamba_amd as D
    rng = np.random.default_rng(77)
    G = rng.integers(0, 4, 20000).astype(np.uint8)
    other = rng.integers(0, 4, 40000).astype(np.uint8)
    M.write_fasta(str(tmp_path / "copies.fa"), [("tid|%d|copy%d" % (500 + i, i), G) for i in range(copies)] + [("tid|999|other", other)])
    D.build_index(str(tmp_path / "copies.fa"), str(tmp_path / "index"))
    recs = M.sample(rng, G, 60, 3000, 0.05, "G") + M.sample(rng, other, 20, 3000, 0.05, "O")
    idx = D.Index(str(tmp_path / "index"))
    lens = ref_lens(idx)
    ctx = D.Ctx(idx, 0, max_sec_N=100)
    ctx.enable_abundance()
    got, sets, ab, summ, want = run_and_check(D, ctx, recs, lens, 950, "%d copies" % copies)
    g = got[:60]
    print("%d copies: n_cand of the copies' reads %r, posteriors %r" % (copies, sorted(set(g["n_cand"].tolist())), sorted(set(g["posterior"].tolist()))))
    assert (g["n_cand"] == copies).all()
    assert (g["ref_ID"] == 0).all()
    assert len(set(x.tobytes() for x in g["posterior"])) == 1 and 0.0 < g["posterior"][0] <= 1.0 / copies * (1 + 1e-9)
    o = got[60:]
    assert (o["ref_ID"] == copies).all() and (o["n_cand"] == 1).all() and (o["posterior"] == 1.0).all()
    ctx.close(); idx.close()


def det_reads():
    import desamba_amd as D
    return D.read_fastq(os.path.join(SYNTH, "pb.fq")) + D.read_fastq(os.path.join(SYNTH, "ngs150.fq")) + D.read_fastq(os.path.join(SYNTH, "ont20k.fq"))


def cli(tmp_path, files, extra=(), tag="run", env=None, index=None):
    out = tmp_path / (tag + ".out")
    e = dict(os.environ); e.update(env or {})
    p = subprocess.run([CLI, "classify"] + list(extra) + [index or os.path.join(ROOT, "data", "demo", "index")] + [str(f) for f in files] + ["-o", str(out)],
                       stderr=subprocess.PIPE, env=e)
    assert p.returncode == 0, p.stderr
    return out.read_bytes(), p.stderr


@pytest.mark.gpu
def test_assign_order_across_batches_slots_contexts_cli(env, tmp_path, monkeypatch):
    import numpy as np
    D, idx, lens = env
    recs = det_reads()
    n = len(recs)
    hist = lambda s: max([len(x[1]) for x in recs[:s]], default=0)
    ctx = D.Ctx(idx, 0)
    with pytest.raises(D.DsbError) as e:
        ctx.abundance_assign()                                   # abundance is off
    assert e.value.code == D.DSB_EINVAL
    ctx.enable_abundance()
    assert len(ctx.abundance_assign()[2]) == 0                   # nothing run yet
    one, sets, ab1, s1, _ = run_and_check(D, ctx, recs, lens, 950, "one batch", strict=True)
    assert len(one) == n and s1["classified"] > 100
    again = ctx.abundance_assign()
    assert again[0].tobytes() == ab1.tobytes() and again[1] == s1 and again[2].tobytes() == one.tobytes()   # asking twice changes nothing
    # reads = NULL counts; cap < n is DSB_ECAP; bad options are refused
    L = D.lib()
    cnt = D.C.c_size_t(0)
    assert L.dsb_ctx_abundance_assign(ctx.h, None, None, None, None, 0, D.C.byref(cnt)) == 0 and cnt.value == n
    out = np.zeros(idx.n_ref, dtype=D.ABUNDANCE_DTYPE); summ = D.DsbAbundanceSummary(); short = np.zeros(n, dtype=D.ASSIGN_DTYPE)
    cnt = D.C.c_size_t(0)
    assert L.dsb_ctx_abundance_assign(ctx.h, None, out.ctypes.data_as(D.C.c_void_p), D.C.byref(summ), short.ctypes.data_as(D.C.c_void_p), n - 1,
                                      D.C.byref(cnt)) == D.DSB_ECAP and cnt.value == n
    assert L.dsb_ctx_abundance_assign(ctx.h, None, None, None, short.ctypes.data_as(D.C.c_void_p), n, D.C.byref(cnt)) == D.DSB_EINVAL
    with pytest.raises(D.DsbError) as e:
        ctx.abundance_assign(max_iter=0)
    assert e.value.code == D.DSB_EINVAL
    # batches of 1 / 7 / the rest
    ctx.reset_abundance()
    assert len(ctx.abundance_assign()[2]) == 0                   # reset_abundance clears the log
    cuts = [0, 1, 8, n]
    for a, b in zip(cuts, cuts[1:]):
        ctx.set_history(hist(a))
        ctx.classify(D.make_reads(recs[a:b]))
    ab3, s3, three = ctx.abundance_assign()
    assert three.tobytes() == one.tobytes() and ab3.tobytes() == ab1.tobytes() and s3 == s1
    ctx.close()
    # two input slots run in reverse order: input order with set_batch_ordinal, run order without
    for with_ordinal in (True, False):
        ctx = D.Ctx(idx, 0, input_slots=2)
        ctx.enable_abundance()
        parts = [D.make_reads(recs[:150]), D.make_reads(recs[150:])]
        ctx.select_slot(0); ctx.set_history(0); ctx.upload(parts[0])
        ctx.select_slot(1); ctx.set_history(hist(150)); ctx.upload(parts[1])
        if with_ordinal:
            ctx.select_slot(0); ctx.set_batch_ordinal(0)
            ctx.select_slot(1); ctx.set_batch_ordinal(150)
        ctx.select_slot(1); ctx.run(); ctx.fetch()
        ctx.select_slot(0); ctx.run(); ctx.fetch()
        ab2, s2, two = ctx.abundance_assign()
        assert ab2.tobytes() == ab1.tobytes() and s2 == s1
        if with_ordinal:
            assert two.tobytes() == one.tobytes()
            # the ordinal held for that run alone: the same slot run again is numbered behind everything collected so far (the
            # same reads once more: the same sets, under the shares of the larger run)
            ctx.run(); ctx.fetch()
            more = ctx.abundance_assign()[2]
            assert len(more) == n + 150 and more["n_cand"][n:].tobytes() == one["n_cand"][:150].tobytes()
            assert more["n_cand"][:n].tobytes() == one["n_cand"].tobytes()
        else:
            assert two.tobytes() == np.concatenate([one[150:], one[:150]]).tobytes()
        ctx.close()
    # an ordinal no batch covered is "none"
    ctx = D.Ctx(idx, 0)
    ctx.enable_abundance()
    ctx.set_history(0); ctx.upload(D.make_reads(recs[:150])); ctx.set_batch_ordinal(0); ctx.run(); ctx.fetch()
    ctx.set_history(hist(150)); ctx.upload(D.make_reads(recs[150:])); ctx.set_batch_ordinal(155); ctx.run(); ctx.fetch()
    gap = ctx.abundance_assign()[2]
    assert len(gap) == n + 5 and as_tuples(gap[150:155]) == [NONE_REC] * 5
    assert gap[:150].tobytes() == one[:150].tobytes() and gap[155:].tobytes() == one[150:].tobytes()
    ctx.close()
    # two contexts on one device, many chunks on both; a second call goes on counting
    monkeypatch.setenv("DSB_SHARD_CHUNK_READS", "30")
    m = D.Multi(idx, [0, 0])
    with pytest.raises(D.DsbError) as e:
        m.abundance_assign()
    assert e.value.code == D.DSB_EINVAL
    m.enable_abundance()
    m.classify(D.make_reads(recs))
    assert min(m.last_calls()) > 0
    abm, sm, mm = m.abundance_assign()
    assert mm.tobytes() == one.tobytes() and abm.tobytes() == ab1.tobytes() and sm == s1
    assert m.abundance()[0].tobytes() == ab1.tobytes()
    m.reset_history()
    m.classify(D.make_reads(recs[:40]))
    assert m.abundance_assign()[2]["n_cand"].tobytes() == np.concatenate([one, one[:40]])["n_cand"].tobytes()   # (other shares now)
    m.reset_abundance()
    assert len(m.abundance_assign()[2]) == 0
    m.reset_history()
    m.classify(D.make_reads(recs))
    assert m.abundance_assign()[2].tobytes() == one.tobytes()
    m.close()
    monkeypatch.delenv("DSB_SHARD_CHUNK_READS")
    # the CLI, -g 0 against -g 0,0, many batches, two input files: the library's lines for the library's records
    M.write_fastq(tmp_path / "a.fq", recs[:200]); M.write_fastq(tmp_path / "b.fq", recs[200:])
    files = [tmp_path / "a.fq", tmp_path / "b.fq"]
    e = {"DSB_CLI_BATCH_KB": "128"}
    sam0, err0 = cli(tmp_path, files, ["-g", "0", "--abundance-reads", str(tmp_path / "g0.reads")], "g0", e)
    sam00, _ = cli(tmp_path, files, ["-g", "0,0", "--abundance-reads", str(tmp_path / "g00.reads"), "--abundance", str(tmp_path / "g00.tsv")], "g00", e)
    want = D.format_assign(idx, D.make_reads(recs), one)
    assert (tmp_path / "g0.reads").read_bytes() == (tmp_path / "g00.reads").read_bytes() == want and want.count(b"\n") == n
    assert sam0 == sam00
    assert (tmp_path / "g00.tsv").read_bytes() == D.format_abundance(idx, ab1, s1)
    low = sum(1 for r in one if r["ref_ID"] != M.NONE and r["posterior"] < 0.5)
    assert (b"; %d reads assigned with posterior < 0.5\n" % low) in err0


@pytest.mark.gpu
def test_assign_unclassified_reads_and_resets(env, tmp_path):
    import numpy as np
    D, idx, lens = env
    rng = np.random.default_rng(5)
    rnd = M.random_reads(rng, 6, 3000)
    pb = D.read_fastq(os.path.join(SYNTH, "pb.fq"))[:40]
    ctx = D.Ctx(idx, 0)
    ctx.enable_abundance()
    # unclassified reads first and last in a batch, then alone in a batch
    recs = rnd[:2] + pb + rnd[2:4]
    ctx.reset_history()
    got, sets, ab, summ, _ = run_and_check(D, ctx, recs, lens, 950, "first and last")
    assert as_tuples(got[:2]) == as_tuples(got[-2:]) == [NONE_REC] * 2 and summ["classified"] == sum(1 for s in sets if s) > 20
    ctx.set_history(max(len(r[1]) for r in recs))
    ctx.classify(D.make_reads(rnd[4:5]), strict=False)
    ab2, s2, got2 = ctx.abundance_assign()
    assert len(got2) == len(recs) + 1 and as_tuples(got2[-1:]) == [NONE_REC] and got2[:-1].tobytes() == got.tobytes()
    assert ab2.tobytes() == ab.tobytes() and s2["reads"] == summ["reads"] + 1
    # all reads unclassified: the EM never runs
    ctx.reset_abundance()
    assert len(ctx.abundance_assign()[2]) == 0                   # an empty store
    ctx.classify(D.make_reads(rnd), strict=False)
    ab0, s0, got0 = ctx.abundance_assign()
    assert as_tuples(got0) == [NONE_REC] * len(rnd) and s0["classified"] == s0["iterations"] == 0 and s0["reads"] == len(rnd)
    assert not ab0["numreads"].any()
    # enabling again with another threshold: emptied, and the other candidate sets
    ctx.enable_abundance(min_frac=0.5)
    assert len(ctx.abundance_assign()[2]) == 0
    ngs = D.read_fastq(os.path.join(SYNTH, "ngs150.fq"))
    ctx.reset_history()
    got5, sets5, _, s5, _ = run_and_check(D, ctx, ngs, lens, 500, "0.5")
    assert s5["min_permille"] == 500
    ctx.enable_abundance(min_frac=1.0)
    ctx.reset_history()
    got1, sets1, _, _, _ = run_and_check(D, ctx, ngs, lens, 1000, "1.0")
    assert got1["n_cand"].sum() < got5["n_cand"].sum()
    ctx.enable_abundance(False)
    with pytest.raises(D.DsbError) as e:
        ctx.abundance_assign()
    assert e.value.code == D.DSB_EINVAL
    ctx.close()
    # the CLI: an empty input, and an input of unclassified reads only
    (tmp_path / "empty.fq").write_bytes(b"")
    cli(tmp_path, [tmp_path / "empty.fq"], ["--abundance-reads", str(tmp_path / "empty.reads")], "empty")
    assert (tmp_path / "empty.reads").read_bytes() == b""
    M.write_fastq(tmp_path / "rand.fq", rnd)
    _, err = cli(tmp_path, [tmp_path / "rand.fq"], ["--abundance-reads", str(tmp_path / "rand.reads")], "rand")
    assert (tmp_path / "rand.reads").read_bytes() == b"".join(b"%s\t*\t0\t0\t0.000000\n" % r[0].encode() for r in rnd)
    assert b"0 classified reads" in err and b"; 0 reads assigned with posterior < 0.5" in err


def readsim(index, path, n, length, err, seed, prof):
    subprocess.check_call([os.path.join(ROOT, "tools", "readsim"), index, str(path), str(n), str(length), str(err), str(seed), prof])


@pytest.fixture(scope="module")
def long_reads(demo, tmp_path_factory):
    """the `long` set of tests/test_run_reductions.py: heavy.fq, 4096 fresh ONT 20-kbp reads, manyanchors.fq among them"""
    import desamba_amd as D
    d = tmp_path_factory.mktemp("assign")
    readsim(demo["index"], d / "ont.fq", 4096, 20000, 0.15, 8642, "ont")
    ont = D.read_fastq(str(d / "ont.fq"))
    return D.read_fastq(os.path.join(SYNTH, "heavy.fq")) + ont[:2000] + D.read_fastq(os.path.join(SYNTH, "manyanchors.fq")) + ont[2000:]


# (row, knobs, taken(t)): each check fails if the knobs were ignored
PATHS = [
    ("step_limit", {"DSB_STEP_LIMIT_RT": "3000"}, lambda t: t.n_retry > 0),                                       # second run
    ("hout_cap", {"DSB_HOUT_CAP": "8"}, lambda t: t.n_regrow > 0),                                                # regrown hit buffer
    ("heavy_mw", {"DSB_HEAVY_FIRST": "16", "DSB_HEAVY_MW": "8"}, lambda t: t.n_early == 16 and t.n_heavy_mw == 8),   # early launch
]


@pytest.mark.gpu
@pytest.mark.parametrize("row", [r[0] for r in PATHS])
def test_assign_on_forced_classify_paths(env, long_reads, monkeypatch, row):
    """two batches per row: one log entry per batch (the second runs and the run after a regrown hit buffer add none), so the
    records number exactly the reads, in run order, and equal the model over the run's own hits"""
    import numpy as np
    D, idx, lens = env
    _, knobs, taken = next(r for r in PATHS if r[0] == row)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    recs = long_reads
    cut = 4096                                                   # (the early launch needs a batch of 4096 reads)
    assert len(recs) > cut
    ctx = D.Ctx(idx, 0)
    ctx.enable_abundance()
    sets = []
    for a, b in ((0, cut), (cut, len(recs))):
        ctx.set_history(max([len(x[1]) for x in recs[:a]], default=0))
        part = recs[a:b]
        res = ctx.classify(D.make_reads(part))
        if a == 0:
            assert taken(ctx.timing()), row
        sets += sets_from_result(res, len(part), idx.n_ref, 950)
    ab, summ, got = ctx.abundance_assign()
    assert len(got) == len(recs) == summ["reads"]
    M.check(got, sets, ab, summ, lens, row)
    assert ctx.abundance()[0].tobytes() == ab.tobytes()
    ctx.close()


@pytest.mark.gpu
def test_cli_other_outputs_unchanged_by_abundance_reads(env, tmp_path):
    """a multi-batch run over plain and gzip files: SAM, --coverage, --abundance, --kraken-out and --report byte for byte the same
    with and without --abundance-reads"""
    D, idx, lens = env
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
    e = {"DSB_CLI_BATCH_KB": "128"}
    exts = (".report", ".cov", ".tsv", ".kraken")
    old = lambda tag: ["--taxonomy", NODES, "--report", str(tmp_path / (tag + ".report")), "--coverage", str(tmp_path / (tag + ".cov")),
                       "--abundance", str(tmp_path / (tag + ".tsv")), "--kraken-out", str(tmp_path / (tag + ".kraken"))]
    plain, err_plain = cli(tmp_path, files, old("plain"), "plain", e)
    with_, err_with = cli(tmp_path, files, old("with") + ["--abundance-reads", str(tmp_path / "with.reads")], "with", e)
    assert plain == with_ == open(os.path.join(SYNTH, "multi6.ubfree.sam"), "rb").read()
    for ext in exts:
        assert (tmp_path / ("plain" + ext)).read_bytes() == (tmp_path / ("with" + ext)).read_bytes() != b"", ext
    assert b"posterior" not in err_plain and b"reads assigned with posterior < 0.5" in err_with
    # --abundance-min-frac is honoured, with --abundance-reads alone
    cli(tmp_path, files, ["--abundance-reads", str(tmp_path / "one.reads"), "--abundance-min-frac", "1"], "one", e)
    a, b = (tmp_path / "with.reads").read_bytes(), (tmp_path / "one.reads").read_bytes()
    cand = lambda t: sum(int(ln.split(b"\t")[3]) for ln in t.splitlines())
    assert a.count(b"\n") == b.count(b"\n") == sum(len(D.read_fastq(os.path.join(SYNTH, n + ".fq"))) for n in names_)
    assert cand(b) < cand(a)
