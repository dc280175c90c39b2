#!/bin/bash
# Cost of `classify --abundance` on a GPU box.  65536 x 50 kbp ONT reads of the demo index (the tests/tools/cli_rate.sh
# set-up): the CLI rate without and with --abundance, runs alternated, outputs compared; then a rocprofv3 kernel trace of one run with
# --abundance on the demo index and, unless MBP=0, on the synthetic strain collection of bench.py's headline (MBP Mbp, built here).
# The CLI's own line gives the end-of-run class build + EM (wall time of dsb_multi_abundance, its classes and iterations).
#   tests/tools/abundance_cost.sh [outdir (default: a new temporary directory)] [MBP]
cd "$(dirname "$0")/../.."
ROOT=$PWD; OUT=$(realpath -m "${1:-$(mktemp -d)}"); MBP=${2:-320}; mkdir -p "$OUT"
G=$ROOT/desamba_amd/bin/deSAMBA; I=$ROOT/data/demo/index
echo "output: $OUT"
t() { timeout -k 10 "$@"; }
prof() {   # prof <tag> <index> <fastq>: kernel statistics of one CLI run with --abundance
	rm -rf "$OUT/prof_$1"
	(cd /tmp && t 600 rocprofv3 --kernel-trace --stats -d "$OUT/prof_$1" -o run --output-format csv -- "$G" classify --abundance "$OUT/ab_$1.tsv" "$2" "$3" -o /dev/shm/ab_prof.sam) > "$OUT/prof_$1.log" 2>&1 || return 1
	grep "abundance:" "$OUT/prof_$1.log"
	f=$(find "$OUT/prof_$1" -name "*kernel_stats.csv" | head -1); cp "$f" "$OUT/$1_kernel_stats.csv"
	grep -E "Name|k_em_|rocprim|k_classify\(" "$OUT/$1_kernel_stats.csv" | sed -E "s/\([^\"]*\)//" | cut -c1-200
}
t 300 python -c "import __graft_entry__ as g; g.demo_dir()" > "$OUT/demo.log" 2>&1 || exit 1
t 300 python tools/gen_fastq.py "$I" /dev/shm/ab.fq 65536 50000 0.15 1001 ont 16 || exit 1
echo "== CLI, alternated"
for rep in 1 2 3; do
	t 300 "$G" classify "$I" /dev/shm/ab.fq -o /dev/shm/ab_plain.sam 2> "$OUT/ab_plain$rep.log" || exit 1
	echo "plain$rep: $(grep processed "$OUT/ab_plain$rep.log")"
	t 300 "$G" classify --abundance "$OUT/ab_demo.tsv" "$I" /dev/shm/ab.fq -o /dev/shm/ab_ab.sam 2> "$OUT/ab_ab$rep.log" || exit 1
	echo "abundance$rep: $(grep processed "$OUT/ab_ab$rep.log") | $(grep "abundance:" "$OUT/ab_ab$rep.log")"
done
cmp /dev/shm/ab_plain.sam /dev/shm/ab_ab.sam && echo "SAM identical with and without --abundance"
echo "references in the table: $(($(wc -l < "$OUT/ab_demo.tsv") - 2))"
head -1 "$OUT/ab_demo.tsv"
echo "== rocprofv3, demo index"
prof demo "$I" /dev/shm/ab.fq || exit 1
rm -f /dev/shm/ab.fq /dev/shm/ab_plain.sam /dev/shm/ab_ab.sam /dev/shm/ab_prof.sam
[ "$MBP" = 0 ] && exit 0
echo "== rocprofv3, ${MBP}-Mbp strain collection (bench.py's headline index)"
H=/tmp/ab_headline; rm -rf "$H"; mkdir -p "$H"
t 900 python tools/synth_ref.py "$H/syn.fa" "$MBP" 11 3 60 12 2> /dev/null || exit 1
t 900 python -c "import sys; sys.path.insert(0, '.'); import desamba_amd as D; st = D.build_index('$H/syn.fa', '$H/index'); print('index built in %.1f s' % st.total_s)" || exit 1
rm -f "$H/syn.fa"
t 300 python tools/gen_fastq.py "$H/index" /dev/shm/ab_h.fq 65536 50000 0.15 1001 ont 16 || exit 1
t 300 "$G" classify --abundance "$OUT/ab_headline.tsv" "$H/index" /dev/shm/ab_h.fq -o /dev/shm/ab_prof.sam 2> "$OUT/ab_headline.log" || exit 1
echo "headline, no profiler: $(grep processed "$OUT/ab_headline.log") | $(grep "abundance:" "$OUT/ab_headline.log")"
head -1 "$OUT/ab_headline.tsv"
echo "references in the table: $(($(wc -l < "$OUT/ab_headline.tsv") - 2))"
prof headline "$H/index" /dev/shm/ab_h.fq; rc=$?
rm -rf "$H" /dev/shm/ab_h.fq /dev/shm/ab_prof.sam
exit $rc
