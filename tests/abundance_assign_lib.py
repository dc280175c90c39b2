"""The host yardstick of the per-read assignment by EM posterior, and the synthetic genomes and reads its tests
share.  Plain Python written from the definition, never from the device code: the candidate sets come from a run's own hits
(reductions_lib.sets_from_result), the shares from the read_share the same abundance_assign call returned, and every weight, sum
and quotient is one IEEE double operation in a plain loop over ascending ref_ID (np.sum would add pairwise)."""

NONE = 0xffffffff
REL = 1e-12


def assign_one(cset, share, L):
    """(ref_ID, n_cand, posterior, near) of one candidate set (ascending tuple); near: the largest weight has a runner-up within a
    relative REL that is not bitwise equal to it, so that a last-bit difference in a share could move the argmax"""
    if not cset:
        return (NONE, 0, 0.0, False)
    w = [float(share[s]) / float(L[s]) for s in cset]
    d = 0.0
    for x in w:
        d += x
    best = 0
    for j in range(1, len(w)):
        if w[j] > w[best]:                                   # (strictly: equal weights stay with the smallest ref_ID)
            best = j
    near = any(x != w[best] and w[best] - x < REL * w[best] for x in w)
    if d == 0.0:
        return (cset[0], len(cset), 0.0, near)
    return (cset[best], len(cset), w[best] / d, near)


def model(sets, share, lens):
    """one record per read, and the records by class"""
    L = [float(x) if x else 1.0 for x in lens]
    by_class = {}
    out = []
    for s in sets:
        if s not in by_class:
            by_class[s] = assign_one(s, share, L)
        out.append(by_class[s])
    return out, by_class


def check(records, sets, ab, summ, lens, label=""):
    """the hard assertion, read for read: ref_ID and n_cand equal, posterior within a relative REL.  A read is left out of the
    ref_ID comparison only when its two largest model weights lie within a relative REL of each other without being bitwise equal;
    such reads are counted, the count is printed and may not exceed 0.1 % of the classified reads."""
    want, _ = model(sets, ab["read_share"], lens)
    assert len(records) == len(want), (label, len(records), len(want))
    classified = sum(1 for s in sets if s)
    assert summ["classified"] == classified, label
    near = 0
    for i, (rec, w) in enumerate(zip(records, want)):
        ref, n_cand, post = int(rec["ref_ID"]), int(rec["n_cand"]), float(rec["posterior"])
        assert n_cand == w[1], (label, i, n_cand, w)
        if w[3] and ref != w[0]:
            near += 1
            assert ref in sets[i], (label, i, ref, sets[i])
        else:
            assert ref == w[0], (label, i, ref, w, sets[i])
            assert abs(post - w[2]) <= REL * abs(w[2]), (label, i, post, w)
    print("%s: %d reads, %d classified, %d left out of the ref_ID comparison as near-ties" % (label, len(want), classified, near))
    assert near <= 0.001 * classified, (label, near, classified)
    return want


# ---------------------------------------------------------------- synthetic genomes and reads (the shapes of tests/test_abundance.py)

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
    ends = np.cumsum(cnt) - 1
    pos = ends[ins & keep]
    out[pos] = rng.integers(0, 4, len(pos))
    return out


def decode(codes):
    import numpy as np
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.asarray(codes, dtype=np.int64)].tobytes()


def sample(rng, genome, n, length, err, tag):
    """n reads of `length` source bases; the name carries the tag, the number and the start on the genome"""
    out = []
    for i in range(n):
        st = int(rng.integers(0, len(genome) - length))
        s = mutate(rng, genome[st:st + length], err)
        if rng.random() < 0.5:
            s = 3 - s[::-1]
        out.append(("%s_%d_%d" % (tag, i, st), decode(s), b"5" * len(s)))
    return out


def write_fasta(path, recs):
    with open(path, "wb") as f:
        for name, codes in recs:
            seq = decode(codes)
            f.write(b">" + name.encode() + b"\n")
            for k in range(0, len(seq), 80):
                f.write(seq[k:k + 80] + b"\n")


def write_fastq(path, recs):
    with open(path, "wb") as f:
        for n, s, q in recs:
            f.write(b"@" + (n if isinstance(n, bytes) else n.encode()) + b"\n" + s + b"\n+\n" + (q if q is not None else b"5" * len(s)) + b"\n")


def random_reads(rng, n, length, tag="u"):
    """reads of random sequence: unclassified on any index of the tests"""
    return [("%s%d" % (tag, i), decode(rng.integers(0, 4, length)), b"5" * length) for i in range(n)]
