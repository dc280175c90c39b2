#!/bin/bash
# Cost of `classify --identity --identity-refs` on a GPU box, the set-up of tests/tools/lca_cost.sh: READS x LEN ONT reads
# (default 65536 x 50 kbp) of the demo index and, unless MBP=0, of the synthetic strain collection of bench.py's headline (MBP Mbp, built
# here).  Per index: the CLI without and with the identity flags, runs alternated, SAM compared; the share of records with each flag
# at the defaults; then a rocprofv3 kernel trace of one run with the flags: k_ident_list, k_hit_edits and k_ident_ref beside k_classify.
# Every GPU step runs under its own time limit and the script ends at the first failure.  What it prints is also written to
# profiles/r07_identity_cost.txt (PROFILE=file for another place).
#   [READS=65536] [LEN=50000] tests/tools/identity_cost.sh [outdir (default: a new temporary directory)] [MBP]
cd "$(dirname "$0")/../.."
ROOT=$PWD; OUT=$(realpath -m "${1:-$(mktemp -d)}"); MBP=${2:-320}; READS=${READS:-65536}; LEN=${LEN:-50000}; mkdir -p "$OUT"
G=$ROOT/desamba_amd/bin/deSAMBA; I=$ROOT/data/demo/index
PROFILE=${PROFILE:-$ROOT/profiles/r07_identity_cost.txt}   # what the script prints is kept here as well (logs and traces stay in outdir)
echo "output: $OUT"
exec > >(tee "$PROFILE") 2>&1
echo "tests/tools/identity_cost.sh: READS=$READS LEN=$LEN MBP=$MBP"
t() { timeout -k 10 "$@"; }
visit() {   # visit <tag> <index> <fastq>
	echo "== CLI, alternated ($1: $READS x $LEN)"
	for rep in 1 2 3; do
		t 600 "$G" classify "$2" "$3" -o /dev/shm/ident_plain.sam 2> "$OUT/$1_plain$rep.log" || return 1
		echo "plain$rep: $(grep processed "$OUT/$1_plain$rep.log")"
		t 900 "$G" classify --identity /dev/shm/ident.tsv --identity-refs "$OUT/$1_refs.tsv" "$2" "$3" -o /dev/shm/ident_on.sam 2> "$OUT/$1_ident$rep.log" || return 1
		echo "identity$rep: $(grep processed "$OUT/$1_ident$rep.log")"
	done
	cmp /dev/shm/ident_plain.sam /dev/shm/ident_on.sam && echo "SAM identical with and without the identity flags"
	# flags: 1 EXACT, 2 OVER, 4 SKEW, 8 EMPTY (column 11); reads without hits have rname *
	awk -F'\t' '$2 != "*" { n++; if ($11 == 1) ex++; if ($11 == 2) ov++; if ($11 == 4) sk++; if ($11 == 8) em++; if ($11 < 2) { s += $10; a++ } }
		END { printf "records %d: EXACT %.4f OVER %.4f SKEW %.4f EMPTY %.4f, mean identity of the aligned ones %.4f\n", n, ex / (n ? n : 1), ov / (n ? n : 1), sk / (n ? n : 1), em / (n ? n : 1), s / (a ? a : 1) }' /dev/shm/ident.tsv
	echo "references in the table: $(($(wc -l < "$OUT/$1_refs.tsv") - 1))"
	echo "== rocprofv3 ($1)"
	rm -rf "$OUT/prof_$1"
	(cd /tmp && t 900 rocprofv3 --kernel-trace --stats -d "$OUT/prof_$1" -o run --output-format csv -- "$G" classify --identity /dev/shm/ident.tsv --identity-refs "$OUT/$1_refs.tsv" "$2" "$3" -o /dev/shm/ident_prof.sam) > "$OUT/prof_$1.log" 2>&1 || return 1
	f=$(find "$OUT/prof_$1" -name "*kernel_stats.csv" | head -1); cp "$f" "$OUT/$1_kernel_stats.csv"
	grep -E "Name|k_ident_list|k_hit_edits|k_ident_ref|k_classify\(" "$OUT/$1_kernel_stats.csv" | sed -E "s/\([^\"]*\)//" | cut -c1-200
	rm -rf "$OUT/prof_$1"
}
t 300 python -c "import __graft_entry__ as g; g.demo_dir()" > "$OUT/demo.log" 2>&1 || exit 1
t 300 python tools/gen_fastq.py "$I" /dev/shm/ident.fq "$READS" "$LEN" 0.15 1001 ont 16 || exit 1
visit demo "$I" /dev/shm/ident.fq; rc=$?
rm -f /dev/shm/ident.fq /dev/shm/ident_plain.sam /dev/shm/ident_on.sam /dev/shm/ident_prof.sam /dev/shm/ident.tsv
[ $rc = 0 ] || exit $rc
[ "$MBP" = 0 ] && exit 0
H=/tmp/ident_headline; rm -rf "$H"; mkdir -p "$H"
t 900 python tools/synth_ref.py "$H/syn.fa" "$MBP" 11 3 60 12 2> /dev/null || exit 1
t 900 python -c "import sys; sys.path.insert(0, '.'); import desamba_amd as D; st = D.build_index('$H/syn.fa', '$H/index'); print('index built in %.1f s' % st.total_s)" || exit 1
rm -f "$H/syn.fa"
t 300 python tools/gen_fastq.py "$H/index" /dev/shm/ident_h.fq "$READS" "$LEN" 0.15 1001 ont 16 || exit 1
visit headline "$H/index" /dev/shm/ident_h.fq; rc=$?
rm -rf "$H" /dev/shm/ident_h.fq /dev/shm/ident_plain.sam /dev/shm/ident_on.sam /dev/shm/ident_prof.sam /dev/shm/ident.tsv
exit $rc
