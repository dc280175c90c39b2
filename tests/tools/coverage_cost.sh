#!/bin/bash
# Cost of `classify --coverage` on a GPU box.  65536 x 50 kbp ONT reads of the demo index (the tests/tools/cli_rate.sh
# set-up): the CLI rate without and with --coverage, runs alternated, outputs compared; then a rocprofv3 kernel trace of one run with
# --coverage on the demo index and, unless MBP=0, on the synthetic strain collection of bench.py's headline (MBP Mbp, built here).
#   tests/tools/coverage_cost.sh [outdir (default: a new temporary directory)] [MBP]
cd "$(dirname "$0")/../.."
ROOT=$PWD; OUT=$(realpath -m "${1:-$(mktemp -d)}"); MBP=${2:-320}; mkdir -p "$OUT"
G=$ROOT/desamba_amd/bin/deSAMBA; I=$ROOT/data/demo/index
echo "output: $OUT"
t() { timeout -k 10 "$@"; }
prof() {   # prof <tag> <index> <fastq>: kernel statistics of one CLI run with --coverage
	rm -rf "$OUT/prof_$1"
	(cd /tmp && t 600 rocprofv3 --kernel-trace --stats -d "$OUT/prof_$1" -o run --output-format csv -- "$G" classify --coverage "$OUT/cov_$1.tsv" "$2" "$3" -o /dev/shm/cov_prof.sam) > "$OUT/prof_$1.log" 2>&1 || return 1
	f=$(find "$OUT/prof_$1" -name "*kernel_stats.csv" | head -1); cp "$f" "$OUT/$1_kernel_stats.csv"
	grep -E "Name|k_ref_cover|k_cover|k_classify\(" "$OUT/$1_kernel_stats.csv" | sed -E "s/\([^\"]*\)//"
}
t 300 python -c "import __graft_entry__ as g; g.demo_dir()" > "$OUT/demo.log" 2>&1 || exit 1
t 300 python tools/gen_fastq.py "$I" /dev/shm/cov.fq 65536 50000 0.15 1001 ont 16 || exit 1
echo "== CLI, alternated"
for rep in 1 2 3; do
	t 300 "$G" classify "$I" /dev/shm/cov.fq -o /dev/shm/cov_plain.sam 2> "$OUT/cov_plain$rep.log" || exit 1
	echo "plain$rep: $(grep processed "$OUT/cov_plain$rep.log")"
	t 300 "$G" classify --coverage "$OUT/cov_demo.tsv" "$I" /dev/shm/cov.fq -o /dev/shm/cov_cov.sam 2> "$OUT/cov_cov$rep.log" || exit 1
	echo "coverage$rep: $(grep processed "$OUT/cov_cov$rep.log")"
done
cmp /dev/shm/cov_plain.sam /dev/shm/cov_cov.sam && echo "SAM identical with and without --coverage"
echo "references in the table: $(($(wc -l < "$OUT/cov_demo.tsv") - 1))"
echo "== rocprofv3, demo index"
prof demo "$I" /dev/shm/cov.fq || exit 1
rm -f /dev/shm/cov.fq /dev/shm/cov_plain.sam /dev/shm/cov_cov.sam /dev/shm/cov_prof.sam
[ "$MBP" = 0 ] && exit 0
echo "== rocprofv3, ${MBP}-Mbp strain collection (bench.py's headline index)"
H=/tmp/cov_headline; rm -rf "$H"; mkdir -p "$H"
t 900 python tools/synth_ref.py "$H/syn.fa" "$MBP" 11 3 60 12 2> /dev/null || exit 1
t 900 python -c "import sys; sys.path.insert(0, '.'); import desamba_amd as D; st = D.build_index('$H/syn.fa', '$H/index'); print('index built in %.1f s' % st.total_s)" || exit 1
rm -f "$H/syn.fa"
t 300 python tools/gen_fastq.py "$H/index" /dev/shm/cov_h.fq 65536 50000 0.15 1001 ont 16 || exit 1
prof headline "$H/index" /dev/shm/cov_h.fq; rc=$?
rm -rf "$H" /dev/shm/cov_h.fq /dev/shm/cov_prof.sam
exit $rc
