#!/bin/bash
# Cost of `classify --coverage-windows` on a GPU box, the set-up of tests/tools/coverage_cost.sh: 65536 x 50 kbp ONT reads of
# the demo index and, unless MBP=0, of the synthetic strain collection of bench.py's headline (MBP Mbp, built here).  Per index: the CLI
# with --coverage alone (BASE: the deSAMBA binary of the commit to compare against; default: this tree's) against this tree's with
# --coverage --coverage-windows (1000-base windows), runs alternated, SAM and --coverage table compared; then a rocprofv3 kernel trace of
# one run with both options: k_ref_windows beside k_ref_cover per batch, k_window_count beside k_cover_count at the end of the run.
#   [BASE=/path/to/deSAMBA] tests/tools/coverage_windows_cost.sh [outdir (default: a new temporary directory)] [MBP]
cd "$(dirname "$0")/../.."
ROOT=$PWD; OUT=$(realpath -m "${1:-$(mktemp -d)}"); MBP=${2:-320}; mkdir -p "$OUT"
G=$ROOT/desamba_amd/bin/deSAMBA; BASE=${BASE:-$G}; I=$ROOT/data/demo/index
echo "output: $OUT"
echo "base: $BASE"
t() { timeout -k 10 "$@"; }
visit() {   # visit <tag> <index> <fastq>: the alternated CLI runs, then the kernel statistics of one run with both options
	echo "== CLI, alternated ($1)"
	for rep in 1 2 3; do
		t 300 "$BASE" classify --coverage "$OUT/base_$1.tsv" "$2" "$3" -o /dev/shm/covw_base.sam 2> "$OUT/$1_base$rep.log" || return 1
		echo "coverage$rep: $(grep processed "$OUT/$1_base$rep.log")"
		t 300 "$G" classify --coverage "$OUT/cov_$1.tsv" --coverage-windows "$OUT/win_$1.tsv" "$2" "$3" -o /dev/shm/covw_win.sam 2> "$OUT/$1_win$rep.log" || return 1
		echo "windows$rep: $(grep processed "$OUT/$1_win$rep.log")"
	done
	cmp /dev/shm/covw_base.sam /dev/shm/covw_win.sam && echo "SAM identical with and without --coverage-windows"
	cmp "$OUT/base_$1.tsv" "$OUT/cov_$1.tsv" && echo "--coverage table identical with and without --coverage-windows"
	echo "references in the table: $(($(wc -l < "$OUT/cov_$1.tsv") - 1)), windows: $(($(wc -l < "$OUT/win_$1.tsv") - 1))"
	# (the table's covbases come from k_cover_count, the windows' from k_window_count, both over the contexts' merged bitmap)
	awk -F'\t' 'NR == FNR { if (FNR > 1) c[$1] = $5; next } FNR > 1 { s[$1] += $5 } END { for (r in c) if (c[r] != s[r]) bad++; for (r in s) if (!(r in c)) bad++;
		print (bad ? bad " references whose windows do not sum to the table" : "covbases of the windows sum to the table\047s for every reference") }' "$OUT/cov_$1.tsv" "$OUT/win_$1.tsv"
	echo "== rocprofv3 ($1)"
	rm -rf "$OUT/prof_$1"
	(cd /tmp && t 600 rocprofv3 --kernel-trace --stats -d "$OUT/prof_$1" -o run --output-format csv -- "$G" classify --coverage "$OUT/cov_$1.tsv" --coverage-windows "$OUT/win_$1.tsv" "$2" "$3" -o /dev/shm/covw_prof.sam) > "$OUT/prof_$1.log" 2>&1 || return 1
	f=$(find "$OUT/prof_$1" -name "*kernel_stats.csv" | head -1); cp "$f" "$OUT/$1_kernel_stats.csv"
	f=$(find "$OUT/prof_$1" -name "*kernel_trace.csv" | head -1); cp "$f" "$OUT/$1_kernel_trace.csv"   # (start / end of every launch: which kernels ran side by side)
	grep -E "Name|k_ref_cover|k_ref_windows|k_cover|k_window|k_classify\(" "$OUT/$1_kernel_stats.csv" | sed -E "s/\([^\"]*\)//"
	rm -rf "$OUT/prof_$1"
}
t 300 python -c "import __graft_entry__ as g; g.demo_dir()" > "$OUT/demo.log" 2>&1 || exit 1
t 300 python tools/gen_fastq.py "$I" /dev/shm/covw.fq 65536 50000 0.15 1001 ont 16 || exit 1
visit demo "$I" /dev/shm/covw.fq; rc=$?
rm -f /dev/shm/covw.fq /dev/shm/covw_base.sam /dev/shm/covw_win.sam /dev/shm/covw_prof.sam
[ $rc = 0 ] || exit $rc
[ "$MBP" = 0 ] && exit 0
H=/tmp/covw_headline; rm -rf "$H"; mkdir -p "$H"
t 900 python tools/synth_ref.py "$H/syn.fa" "$MBP" 11 3 60 12 2> /dev/null || exit 1
t 900 python -c "import sys; sys.path.insert(0, '.'); import desamba_amd as D; st = D.build_index('$H/syn.fa', '$H/index'); print('index built in %.1f s' % st.total_s)" || exit 1
rm -f "$H/syn.fa"
t 300 python tools/gen_fastq.py "$H/index" /dev/shm/covw_h.fq 65536 50000 0.15 1001 ont 16 || exit 1
visit headline "$H/index" /dev/shm/covw_h.fq; rc=$?
rm -rf "$H" /dev/shm/covw_h.fq /dev/shm/covw_base.sam /dev/shm/covw_win.sam /dev/shm/covw_prof.sam
exit $rc
