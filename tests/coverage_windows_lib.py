"""The host yardstick of the per-window coverage, shared by the tests: plain numpy written from the definition in
include/desamba_amd.h, never from the device code.  Per reference a difference array gives the depth of every base and a boolean
array the union of the intervals; both are summed per window."""
import numpy as np

FIELDS = ("starts", "aligned_bases", "covbases")
HEADER = b"#rname\tstart\tend\tnumreads\tcovbases\tcoverage\tmeandepth\n"


def n_windows(L, W):
    return -(-L // W)


def first_windows(lens, W):
    """first_r for r = 0 .. n_ref (the last entry is the total)"""
    first = [0]
    for L in lens:
        first.append(first[-1] + n_windows(L, W))
    return first


def host_windows(lens, records, W):
    """records: (ref, t_st, t_ed, ...) of every counted record -> (array [n_win, 3] of (starts, aligned_bases, covbases),
    the number of counted records with an empty interval per reference)"""
    first = first_windows(lens, W)
    out = np.zeros((first[-1], 3), dtype=np.uint64)
    by_ref = {}
    empty = [0] * len(lens)
    for rec in records:
        ref, ts, te = rec[0], rec[1], rec[2]
        L = lens[ref]
        s, e = min(ts, L), min(te, L)
        if e > s:
            by_ref.setdefault(ref, []).append((s, e))
        else:
            empty[ref] += 1
    for ref, iv in by_ref.items():
        L = lens[ref]
        diff = np.zeros(L + 1, dtype=np.int64)
        union = np.zeros(L, dtype=bool)
        starts = np.zeros(n_windows(L, W), dtype=np.int64)
        for s, e in iv:
            diff[s] += 1; diff[e] -= 1
            union[s:e] = True
            starts[s // W] += 1
        depth = np.cumsum(diff)[:L]
        at = np.arange(0, L, W)
        o = out[first[ref]:first[ref + 1]]
        o[:, 0] = starts
        o[:, 1] = np.add.reduceat(depth, at)
        o[:, 2] = np.add.reduceat(union.astype(np.int64), at)
    return out, empty


def as_matrix(win):
    """Ctx / Multi.coverage_windows() as the [n_win, 3] matrix host_windows gives"""
    return np.stack([win[f] for f in FIELDS], axis=1).astype(np.uint64)


def check_invariants(lens, W, win, cov, empty):
    """per reference, over its windows: aligned_bases and covbases sum to the reference's, starts to numreads minus the empty records"""
    first = first_windows(lens, W)
    assert len(win) == first[-1]
    m = as_matrix(win)
    csum = np.concatenate([np.zeros((1, 3), dtype=np.uint64), np.cumsum(m, axis=0, dtype=np.uint64)])
    per_ref = csum[first[1:]] - csum[first[:-1]]
    assert list(per_ref[:, 1]) == [int(x) for x in cov["aligned_bases"]]
    assert list(per_ref[:, 2]) == [int(x) for x in cov["covbases"]]
    assert list(per_ref[:, 0]) == [int(x) - empty[r] for r, x in enumerate(cov["numreads"])]


def table(names, lens, numreads, win, W):
    """the expected --coverage-windows file: win an [n_win, 3] matrix (or list of triples) of (starts, aligned_bases, covbases)"""
    out = [HEADER]
    first = 0
    for r, L in enumerate(lens):
        nw = n_windows(L, W)
        if numreads[r]:
            for j in range(nw):
                s, e = j * W, min((j + 1) * W, L)
                st, ab, cb = (int(x) for x in win[first + j])
                out.append(b"%s\t%d\t%d\t%d\t%d\t%s\t%s\n" % (names[r].encode(), s, e, st, cb, b"%g" % (100.0 * cb / (e - s)), b"%g" % (ab / (e - s))))
        first += nw
    return b"".join(out)
