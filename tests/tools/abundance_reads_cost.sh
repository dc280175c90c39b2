#!/bin/bash
# Cost of `classify --abundance-reads` on a GPU box.  65536 x 50 kbp ONT reads (the tests/tools/abundance_cost.sh
# set-up), two contexts on one device (the CLI's default), on the demo index and, unless MBP=0, on the synthetic strain collection
# of bench.py's headline (MBP Mbp, built here):
#   1. the CLI without and with --abundance-reads, PAIRS alternated pairs, the SAM compared every time ("processed in" is the
#      classify part; the end-of-run solve lies outside it);
#   2. the end-of-run wall time the CLI's own "abundance:" line reports -- dsb_multi_abundance (--abundance, by the binary of
#      $PARENT if that names a deSAMBA binary of the parent commit, else by this tree's) against dsb_multi_abundance_assign
#      (--abundance-reads), alternated pairs;
#   3. a rocprofv3 kernel trace, in a run of its own, of one run with --abundance-reads: k_em_assign_class beside k_em_class (same
#      launch shape, same classes) and k_em_assign_read beside k_em_keys (same shape, same records).
# Every GPU step runs under its own time limit and the script ends at the first failure.
#   [PARENT=path/to/deSAMBA] [PAIRS=6] [HPAIRS=3: pairs on the strain collection] tests/tools/abundance_reads_cost.sh [outdir (default: a new temporary directory)] [MBP]
cd "$(dirname "$0")/../.."
ROOT=$PWD; OUT=$(realpath -m "${1:-$(mktemp -d)}"); MBP=${2:-320}; PAIRS=${PAIRS:-6}; HPAIRS=${HPAIRS:-3}; mkdir -p "$OUT"
G=$ROOT/desamba_amd/bin/deSAMBA; I=$ROOT/data/demo/index
P=$G; ptag="this tree's build"
if [ -n "$PARENT" ] && [ -x "$PARENT" ]; then P=$PARENT; ptag="the parent commit's build"; fi
echo "output: $OUT"
t() { timeout -k 10 "$@"; }
pairs() {   # pairs <tag> <index> <fastq> <n>: steps 1 and 2
	echo "== $1: CLI without / with --abundance-reads, $4 alternated pairs"
	for rep in $(seq 1 "$4"); do
		t 300 "$G" classify "$2" "$3" -o /dev/shm/abr_plain.sam 2> "$OUT/$1_plain$rep.log" || return 1
		echo "plain$rep: $(grep processed "$OUT/$1_plain$rep.log")"
		t 300 "$G" classify --abundance-reads /dev/shm/abr.reads "$2" "$3" -o /dev/shm/abr_reads.sam 2> "$OUT/$1_reads$rep.log" || return 1
		echo "reads$rep: $(grep processed "$OUT/$1_reads$rep.log") | $(grep "abundance:" "$OUT/$1_reads$rep.log")"
		cmp /dev/shm/abr_plain.sam /dev/shm/abr_reads.sam && echo "  SAM identical" || return 1
	done
	echo "lines in the per-read file: $(wc -l < /dev/shm/abr.reads); posterior < 0.999999: $(awk -F'\t' '$2 != "*" && $5 < 0.999999' /dev/shm/abr.reads | wc -l)"
	echo "== $1: end of run, dsb_multi_abundance ($ptag) against dsb_multi_abundance_assign, $4 alternated pairs"
	for rep in $(seq 1 "$4"); do
		t 300 "$P" classify --abundance "$OUT/$1_parent.tsv" "$2" "$3" -o /dev/shm/abr_plain.sam 2> "$OUT/$1_eor_a$rep.log" || return 1
		echo "abundance$rep: $(grep "abundance:" "$OUT/$1_eor_a$rep.log")"
		t 300 "$G" classify --abundance "$OUT/$1_new.tsv" --abundance-reads /dev/shm/abr.reads "$2" "$3" -o /dev/shm/abr_reads.sam 2> "$OUT/$1_eor_b$rep.log" || return 1
		echo "assign$rep:    $(grep "abundance:" "$OUT/$1_eor_b$rep.log")"
		cmp "$OUT/$1_parent.tsv" "$OUT/$1_new.tsv" && echo "  abundance table identical" || return 1
	done
}
prof() {   # prof <tag> <index> <fastq>: kernel statistics of one CLI run with --abundance-reads
	rm -rf "$OUT/prof_$1"
	(cd /tmp && t 600 rocprofv3 --kernel-trace --stats -d "$OUT/prof_$1" -o run --output-format csv -- "$G" classify --abundance-reads /dev/shm/abr.reads "$2" "$3" -o /dev/shm/abr_prof.sam) > "$OUT/prof_$1.log" 2>&1 || return 1
	grep "abundance:" "$OUT/prof_$1.log"
	f=$(find "$OUT/prof_$1" -name "*kernel_stats.csv" | head -1); cp "$f" "$OUT/$1_kernel_stats.csv"
	grep -E "Name|k_em_|k_classify\(" "$OUT/$1_kernel_stats.csv" | sed -E "s/\([^\"]*\)//" | cut -c1-200
	rm -rf "$OUT/prof_$1"
}
t 300 python -c "import __graft_entry__ as g; g.demo_dir()" > "$OUT/demo.log" 2>&1 || exit 1
t 300 python tools/gen_fastq.py "$I" /dev/shm/abr.fq 65536 50000 0.15 1001 ont 16 || exit 1
pairs demo "$I" /dev/shm/abr.fq "$PAIRS" || exit 1
echo "== rocprofv3, demo index"
prof demo "$I" /dev/shm/abr.fq || exit 1
rm -f /dev/shm/abr.fq /dev/shm/abr_plain.sam /dev/shm/abr_reads.sam /dev/shm/abr_prof.sam /dev/shm/abr.reads
[ "$MBP" = 0 ] && exit 0
echo "== ${MBP}-Mbp strain collection (bench.py's headline index)"
H=/tmp/abr_headline; rm -rf "$H"; mkdir -p "$H"
t 900 python tools/synth_ref.py "$H/syn.fa" "$MBP" 11 3 60 12 2> /dev/null || exit 1
t 900 python -c "import sys; sys.path.insert(0, '.'); import desamba_amd as D; st = D.build_index('$H/syn.fa', '$H/index'); print('index built in %.1f s' % st.total_s)" || exit 1
rm -f "$H/syn.fa"
t 300 python tools/gen_fastq.py "$H/index" /dev/shm/abr_h.fq 65536 50000 0.15 1001 ont 16 || exit 1
pairs headline "$H/index" /dev/shm/abr_h.fq "$HPAIRS"; rc=$?
if [ $rc = 0 ]; then echo "== rocprofv3, headline index"; prof headline "$H/index" /dev/shm/abr_h.fq; rc=$?; fi
rm -rf "$H" /dev/shm/abr_h.fq /dev/shm/abr_plain.sam /dev/shm/abr_reads.sam /dev/shm/abr_prof.sam /dev/shm/abr.reads
exit $rc
