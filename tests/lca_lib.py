"""The host yardstick of the LCA classification: per-read records (read_lca over a read's hits), the run's rows and
summary (counts), Kraken's per-read line and Kraken's report.  Plain Python written from the definition and the report rules,
never from the device code: the LCA is found as the deepest member of the intersection of the candidates' ancestor chains."""

CLASSIFIED, NO_TAXON, AMBIGUOUS = 1, 2, 4
NONE = 0xffffffff
LETTER = {"superkingdom": "D", "domain": "D", "kingdom": "K", "phylum": "P", "class": "C", "order": "O", "family": "F", "genus": "G",
          "species": "S"}


def load_nodes(path):
    """nodes.dmp -> (parent, rank, max_tid) as the loader reads it: max_tid = the last line's taxid + 1 000 000, parent[1] = 0"""
    parent, rank, last = {}, {}, 0
    for line in open(path):
        f = [x.strip() for x in line.split("|")]
        if not f[0]:
            continue
        last = int(f[0])
        parent[last] = int(f[1]); rank[last] = f[2]
    parent[1] = 0; rank[1] = "root"
    return parent, rank, last + 1000000


def load_names(path):
    names = {}
    for line in open(path):
        f = [x.strip("\t") for x in line.rstrip("\n").split("|")]
        if len(f) >= 4 and f[3] == "scientific name" and int(f[0]) not in names:
            names[int(f[0])] = f[1]
    return names


def ref_taxid(name):
    """the taxid of a reference name: the second '|' field as strtok / strtoul read it (0 if absent); NONE for a name that would
    not come back from the SAM text as it is"""
    if not name or name[0] == "*" or "\t" in name or "\n" in name:
        return NONE
    f = [x for x in name.split("|") if x]
    if len(f) < 2:
        return 0
    d = ""
    for ch in f[1].lstrip(" \t"):
        if not ch.isdigit():
            break
        d += ch
    return int(d) if d else 0


def chain(parent, max_tid, t):
    """[t, parent(t), ..., 1] for a rooted taxid, else None"""
    out, seen = [], set()
    while True:
        if t < 1 or t > max_tid or t in seen:
            return None
        out.append(t); seen.add(t)
        if t == 1:
            return out
        t = parent.get(t, NONE)


def depth(parent, max_tid, t):
    c = chain(parent, max_tid, t)
    return None if c is None else len(c) - 1


def read_lca(hits, ref_tid, parent, max_tid, permille, cache=None):
    """hits: (ref_ID, AS) of one read; ref_tid: the taxid of each reference (n_ref of them) -> (taxid, S_max, n_pass, depth, flags)"""
    hits = [(r, s) for r, s in hits if r < len(ref_tid)]
    if not hits:
        return (0, 0, 0, 0, 0)
    smax = max(s for _, s in hits)
    passing = [r for r, s in hits if s * 1000 >= smax * permille]
    cache = {} if cache is None else cache
    tids = set()
    for r in passing:
        t = ref_tid[r]
        if t not in cache:
            cache[t] = chain(parent, max_tid, t)
        if cache[t] is not None:
            tids.add(t)
    if not tids:
        return (0, smax, len(passing), 0, CLASSIFIED | NO_TAXON)
    common = None
    for t in tids:
        common = set(cache[t]) if common is None else common & set(cache[t])
    first = cache[next(iter(tids))]
    node = next(x for x in first if x in common)              # the chain runs from deep to shallow: its first common member is the deepest
    return (node, smax, len(passing), len(chain(parent, max_tid, node)) - 1, CLASSIFIED | (AMBIGUOUS if len(tids) > 1 else 0))


def hits_of(res, i):
    rr = res.reads[i]
    return [(res.hits[rr.first + k].ref_ID, res.hits[rr.first + k].sum_score) for k in range(rr.n)]


def records(res, n_reads, ref_tid, parent, max_tid, permille):
    """the model over a batch's own hits (a DsbResult)"""
    import ctypes as C
    import numpy as np
    cache = {}
    if n_reads == 0:
        return []
    nh = int(res.n_hits)
    ref, score = [], []
    if nh:                                                    # (dsb_hit: eight 32-bit words, ref_ID the first, sum_score the sixth)
        raw = np.frombuffer((C.c_uint8 * (nh * 32)).from_address(C.addressof(res.hits.contents)), dtype=np.uint32).reshape(nh, 8)
        ref, score = raw[:, 0].tolist(), raw[:, 5].tolist()
    out = []
    for i in range(n_reads):
        rr = res.reads[i]
        out.append(read_lca([(ref[k], score[k]) for k in range(rr.first, rr.first + rr.n)] if rr.n else [], ref_tid, parent, max_tid, permille, cache))
    return out


def as_tuples(lca):
    """Ctx.lca()'s array as the model's tuples"""
    return [(int(x["taxid"]), int(x["score"]), int(x["n_pass"]), int(x["depth"]), int(x["flags"])) for x in lca]


def counts(recs, parent, max_tid, permille):
    """records (tuples) -> ([(taxid, clade, direct)] ascending, summary dict)"""
    direct, clade = {}, {}
    for t, _, _, _, _ in recs:
        if t:
            direct[t] = direct.get(t, 0) + 1
    for t, c in direct.items():
        for a in chain(parent, max_tid, t):
            clade[a] = clade.get(a, 0) + c
    rows = [(t, clade[t], direct.get(t, 0)) for t in sorted(clade)]
    summ = dict(reads=len(recs), classified=sum(1 for r in recs if r[0]), no_taxon=sum(1 for r in recs if r[4] & NO_TAXON),
                ambiguous=sum(1 for r in recs if r[4] & AMBIGUOUS), min_permille=permille)
    return rows, summ


def rows_as_tuples(rows):
    return [(int(r["taxid"]), int(r["clade_reads"]), int(r["direct_reads"])) for r in rows]


def kraken_line(name, length, rec):
    name = name if isinstance(name, bytes) else name.encode()
    return b"%s\t%s\t%d\t%d\t%d:%d\n" % (b"C" if rec[0] else b"U", name, rec[0], length, rec[1], rec[2])


def report(rows, summ, parent, rank, names=None):
    """Kraken's report of rows [(taxid, clade, direct)] (any order)"""
    if not summ["reads"]:
        return b""
    out = []
    reads = summ["reads"]
    u = reads - summ["classified"]
    if u > 0:
        out.append("%6.2f\t%d\t%d\tU\t0\tunclassified\n" % (100.0 * u / reads, u, u))
    by = {t: (c, d) for t, c, d in rows if c > 0}
    kids = {}
    for t in by:
        if t != 1 and parent.get(t) in by:
            kids.setdefault(parent[t], []).append(t)

    def walk(t, dep, letter, num):
        c, d = by[t]
        name = names[t] if names and t in names else str(t)
        out.append("%6.2f\t%d\t%d\t%s%s\t%d\t%s%s\n" % (100.0 * c / reads, c, d, letter, str(num) if num else "", t, "  " * dep, name))
        for k in sorted(kids.get(t, []), key=lambda x: (-by[x][0], x)):
            lt = LETTER.get(rank.get(k, ""))
            if lt:
                walk(k, dep + 1, lt, 0)
            else:
                walk(k, dep + 1, letter, num + 1)
    if 1 in by:
        import sys
        sys.setrecursionlimit(max(sys.getrecursionlimit(), 20000))
        walk(1, 0, "R", 0)
    return "".join(out).encode()
