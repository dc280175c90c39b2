#!/bin/bash
# Cost of `classify --cigar-sam --cigar-checkpoint` on a GPU box, on the workload of tests/tools/identity_cost.sh: READS x
# LEN ONT reads at 15 % errors (default 65536 x 50 kbp) of the demo index, defaults.  One rocprofv3 kernel trace each (no counters) of
# a run with --identity (k_hit_edits), with --cigar-sam (k_hit_align) and with --cigar-sam --cigar-checkpoint (k_hit_align_ck), the
# aligned SAM going to /dev/null; then the alignment flags of the first 4096 reads in both modes at the default room, beside the
# plan rule's count of the same records.  Every GPU step runs under its own time limit and the script ends at the first failure.
# What it prints is also written to profiles/r09_alignment_checkpoint_cost.txt (PROFILE=file for another place).
#   [READS=65536] [LEN=50000] tests/tools/alignment_checkpoint_cost.sh [outdir (default: a new temporary directory)]
cd "$(dirname "$0")/../.."
ROOT=$PWD; OUT=$(realpath -m "${1:-$(mktemp -d)}"); READS=${READS:-65536}; LEN=${LEN:-50000}; mkdir -p "$OUT"
G=$ROOT/desamba_amd/bin/deSAMBA; I=$ROOT/data/demo/index; FQ=/dev/shm/alnck.fq
PROFILE=${PROFILE:-$ROOT/profiles/r09_alignment_checkpoint_cost.txt}
echo "output: $OUT"
exec > >(tee "$PROFILE") 2>&1
echo "tests/tools/alignment_checkpoint_cost.sh: READS=$READS LEN=$LEN, demo index, band 256, cap 300 permille, trace 2048 KiB per wavefront"
t() { timeout -k 10 "$@"; }
trace() {   # trace <tag> <classify options ...>
	tag=$1; shift
	rm -rf "$OUT/prof_$tag"
	(cd /tmp && t 900 rocprofv3 --kernel-trace --stats -d "$OUT/prof_$tag" -o run --output-format csv -- "$G" classify "$@" "$I" "$FQ" -o /dev/shm/alnck_$tag.sam) > "$OUT/prof_$tag.log" 2>&1 || return 1
	echo "== rocprofv3, $tag: $(grep processed "$OUT/prof_$tag.log")"
	f=$(find "$OUT/prof_$tag" -name "*kernel_stats.csv" | head -1)
	grep -E "Name|k_ident_list|k_hit_edits|k_hit_align|k_ident_ref|k_classify\(" "$f" | sed -E "s/\([^\"]*\)//" | cut -c1-200
	rm -rf "$OUT/prof_$tag"
}
fin() { rm -f "$FQ" /dev/shm/alnck_head.fq /dev/shm/alnck_*.sam /dev/shm/alnck.tsv; }
t 300 python -c "import __graft_entry__ as g; g.demo_dir()" > "$OUT/demo.log" 2>&1 || exit 1
t 300 python tools/gen_fastq.py "$I" "$FQ" "$READS" "$LEN" 0.15 1001 ont 16 || exit 1
trace ident --identity /dev/shm/alnck.tsv || { fin; exit 1; }
trace full --cigar-sam /dev/null || { fin; exit 1; }
trace checkpoint --cigar-sam /dev/null --cigar-checkpoint || { fin; exit 1; }
cmp /dev/shm/alnck_ident.sam /dev/shm/alnck_full.sam && cmp /dev/shm/alnck_ident.sam /dev/shm/alnck_checkpoint.sam && echo "SAM identical with --identity, --cigar-sam and --cigar-sam --cigar-checkpoint"
echo "== flags of the first 4096 reads, both modes at the default room"
head -n 16384 "$FQ" > /dev/shm/alnck_head.fq   # (the reader takes a file whole)
t 600 python - "$I" /dev/shm/alnck_head.fq <<'PY' || { fin; exit 1; }
import sys, time
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import numpy as np
import desamba_amd as D
import align_ck_lib as K
import align_lib as A
idx = D.Index(sys.argv[1])
recs = D.read_fastq(sys.argv[2], 4096)
reads = D.make_reads(recs)
ctx = D.Ctx(idx, 0)
ctx.enable_identity(); ctx.enable_alignment()
name = {A.OPS: "OPS", A.NOTRACE: "NOTRACE", A.NOROOM: "NOROOM", A.UNALIGNED: "UNALIGNED"}
for mode, tag in ((D.DSB_ALN_MODE_FULL, "full"), (D.DSB_ALN_MODE_CHECKPOINT, "checkpoint")):
    ctx.alignment_mode(mode); ctx.reset_identity(); ctx.reset_history()
    t0 = time.time()
    res = ctx.classify(reads)
    aln, ops = ctx.alignment(res.n_hits)
    wall = time.time() - t0
    ident = ctx.identity(res.n_hits)
    live = aln["flags"] != 0
    cnt = {name[f]: int((aln["flags"][live] == f).sum()) for f in name}
    print("%s (first 4096 reads, %d bases): %d counted records, %r; batch wall %.2f s" % (tag, sum(len(r[1]) for r in recs), int(live.sum()), cnt, wall))
    has = aln["flags"] == A.OPS
    if has.any():
        print("  operations per record with a path: mean %.0f, max %d; %d operations copied back (%.1f MiB) for %d used" % (
            aln["n_ops"][has].mean(), aln["n_ops"][has].max(), len(ops), len(ops) * 4 / 2 ** 20, int(aln["n_ops"][has].sum())))
    if mode == D.DSB_ALN_MODE_CHECKPOINT:
        al = [(int(r["q_len"]), int(r["t_len"]), int(r["edits"])) for r, a in zip(ident, aln) if a["flags"] in (A.OPS, A.NOTRACE, A.NOROOM)]
        plans = [K.plan(n, m) for n, m, e in al]
        print("  plan rule: %d aligned records, %d without a plan; K %d .. %d, checkpoints %d .. %d; edits %d .. %d; segments walked per record: mean %.2f" % (
            len(al), sum(1 for p in plans if p is None), min(p[0] for p in plans if p), max(p[0] for p in plans if p), min(p[1] for p in plans if p),
            max(p[1] for p in plans if p), min(e for n, m, e in al), max(e for n, m, e in al),
            np.mean([(e - 1) // p[0] + 1 for (n, m, e), p in zip(al, plans) if p and e])))
ctx.close(); idx.close()
PY
fin
