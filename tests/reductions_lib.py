"""The host yardsticks of the run-wide results of classify, shared by the tests: per-reference coverage (accumulate over
counted_records), abundance (candidate_set / em / check_against over sets_from_result) and per-read taxa (walk_golden_sam over
a SAM, golden or made by a run).  Plain Python / numpy written from the definitions, never from the device code."""


# ---------------------------------------------------------------- coverage

def union_len(iv):
    tot, cur_s, cur_e = 0, None, None
    for s, e in sorted(iv):
        if cur_e is None or s > cur_e:
            if cur_e is not None:
                tot += cur_e - cur_s
            cur_s, cur_e = s, e
        else:
            cur_e = max(cur_e, e)
    return tot + (cur_e - cur_s if cur_e is not None else 0)


def accumulate(n_ref, records, lens):
    """records: (ref, t_st, t_ed, mapq) of every counted record -> [(numreads, covbases, aligned_bases, mapq_sum)] per reference"""
    iv = [[] for _ in range(n_ref)]
    cnt = [[0, 0, 0] for _ in range(n_ref)]
    for ref, ts, te, mq in records:
        L = lens[ref]
        s, e = min(ts, L), min(te, L)
        cnt[ref][0] += 1; cnt[ref][2] += mq
        if e > s:
            iv[ref].append((s, e)); cnt[ref][1] += e - s
    return [(c[0], union_len(iv[r]), c[1], c[2]) for r, c in enumerate(cnt)]


def mapq_pri(h, n):
    d = (h[0].sum_score - h[1].sum_score) & 0xffffffff if n > 1 else 0
    if n == 1 or d > 5:
        return 30
    v = (d << 2) & 0xffffffff
    return v - (1 << 32) if v >= 1 << 31 else v


def counted_records(res, n_reads):
    """the records dsb_format_sam prints without FLAG 0x100: the primary and the supplementary ones (pri_index 0)"""
    out = []
    for i in range(n_reads):
        rr = res.reads[i]
        if not rr.n:
            continue
        h = [res.hits[rr.first + k] for k in range(rr.n)]
        mq = mapq_pri(h, rr.n)
        for k, c in enumerate(h):
            if k == 0 or c.pri_index == 0:
                out.append((c.ref_ID, c.t_st, c.t_ed, mq if k == 0 else min(mq, 30)))
    return out


# ---------------------------------------------------------------- abundance

def candidate_set(hits, n_ref, permille):
    """hits: (ref_ID, AS) of one read -> its candidate set (sorted tuple; empty: the read takes no part)"""
    hits = [(r, s) for r, s in hits if r < n_ref]
    if not hits:
        return ()
    smax = max(s for _, s in hits)
    return tuple(sorted({r for r, s in hits if s * 1000 >= smax * permille}))


def classes_of(sets):
    out = {}
    for s in sets:
        if s:
            out[s] = out.get(s, 0) + 1
    return out


def em(classes, lens, max_iter=10000, tol=0.01, trace=None):
    """the EM of DESIGN 2.10 over {set: count}: (a, iterations, converged, last max change); trace (a list): gets the max change
    of every iteration"""
    import numpy as np
    n_ref = len(lens)
    L = np.array([float(x) if x else 1.0 for x in lens])
    keys = sorted(classes)
    c = np.array([classes[k] for k in keys], dtype=np.float64)
    N = c.sum()
    a = np.zeros(n_ref)
    if not keys:
        return a, 0, True, 0.0
    flat_ref = np.concatenate([np.array(k, dtype=np.int64) for k in keys])
    flat_cls = np.concatenate([np.full(len(k), i, dtype=np.int64) for i, k in enumerate(keys)])
    present = np.bincount(flat_ref, minlength=n_ref) > 0
    a[present] = 1.0 / present.sum()
    chg = 0.0
    for it in range(1, max_iter + 1):
        w = a / L
        denom = np.bincount(flat_cls, weights=w[flat_ref], minlength=len(keys))
        coef = np.where(denom > 0, c / np.where(denom > 0, denom, 1.0), 0.0)
        t = np.bincount(flat_ref, weights=coef[flat_cls], minlength=n_ref)
        an = w * t / N
        chg = float(np.max(np.abs(an - a)) * N)
        if trace is not None:
            trace.append(chg)
        a = an
        if chg < tol:
            return a, it, True, chg
    return a, max_iter, False, chg


def counts_of(classes, n_ref):
    numreads, uniq = [0] * n_ref, [0] * n_ref
    for s, c in classes.items():
        for r in s:
            numreads[r] += c
        if len(s) == 1:
            uniq[s[0]] += c
    return numreads, uniq


def check_against(ab, summ, sets, lens, label="", tiny=None):
    """GPU result (max_iter=200, tol=0) against the numpy EM over the same candidate sets; tiny: estimates numpy puts at or below
    it may have underflowed to 0 (references that lose every class over 200 iterations, at scale), the others must be > 0"""
    import numpy as np
    n_ref = len(lens)
    cl = classes_of(sets)
    nr, ur = counts_of(cl, n_ref)
    assert list(ab["numreads"]) == nr, label
    assert list(ab["uniqreads"]) == ur, label
    assert summ["classified"] == sum(cl.values()), label
    assert summ["classes"] == len(cl), label
    a, it, _, _ = em(cl, lens, max_iter=200, tol=0.0)
    assert summ["iterations"] == 200 and not summ["converged"], label
    N = sum(cl.values())
    exp = N * a
    got = ab["est_reads"]
    assert np.all(np.abs(got - exp) <= 1e-9 * np.maximum(np.abs(exp), 1e-300) + 1e-12), (label, np.max(np.abs(got - exp)))
    if tiny is None:
        assert np.all((got > 0) == (np.array(nr) > 0)), label
    else:
        big = exp > tiny
        assert np.all((got[big] > 0) == (np.array(nr)[big] > 0)) and np.all(got[~big] <= 2 * tiny), label


def sets_from_result(res, n_reads, n_ref, permille):
    out = []
    for i in range(n_reads):
        rr = res.reads[i]
        out.append(candidate_set([(res.hits[rr.first + k].ref_ID, res.hits[rr.first + k].sum_score) for k in range(rr.n)], n_ref, permille))
    return out


# ---------------------------------------------------------------- taxa

def nodes_table(path):
    parent = {}
    for line in open(path):
        f = [x.strip() for x in line.split("|")]
        parent[int(f[0])] = int(f[1])
    return parent


def walk_golden_sam(path, table, max_tid):
    """the per-read taxon recomputed from the golden SAM (a path, or the bytes of a SAM a run made): the walk over each read's
    own records"""
    def tid_of(rname):
        f = [x for x in rname.split(b"|") if x]
        return int(f[1]) if len(f) > 1 else 0

    def descends(t, held):
        p = t
        while True:
            if p == held:
                return True
            if p < 1 or p == 0xffffffff or p > max_tid:
                return False
            p = 0 if p == 1 else table.get(p, 0xffffffff)
    groups = []
    for line in (path if isinstance(path, bytes) else open(path, "rb").read()).splitlines():
        f = [x for x in line.split(b"\t") if x]
        if groups and groups[-1][0] == f[0]:
            groups[-1][1].append(f)
        else:
            groups.append((f[0], [f]))
    out = []
    for _, recs in groups:
        f0 = recs[0]
        if f0[2].startswith(b"*") or tid_of(f0[2]) > max_tid:
            out.append(0); continue
        tid, score = tid_of(f0[2]), int(f0[11].split(b":")[2])
        for f in recs[1:] if score else []:
            t = tid_of(f[2])
            if int(f[11].split(b":")[2]) == score and t <= max_tid and descends(t, tid):
                tid = t
        out.append(tid)
    return out
