#!/bin/bash
# Cost of `classify --kraken-out --kraken-report` on a GPU box.  65536 x 50 kbp ONT reads of the demo index (the
# tests/tools/cli_rate.sh set-up): the CLI rate without and with the LCA flags, runs alternated, SAM compared; then a rocprofv3 kernel
# trace of one run with the LCA flags and --abundance (k_em_collect in the same trace is what k_read_lca + k_lca_count are held
# against) on the demo index and, unless MBP=0, on the synthetic strain collection of bench.py's headline (MBP Mbp, built here, with
# a taxonomy made from its reference names: strains of 4 under a genus, genera of 8 under a family).  The CLI's own line gives
# the end-of-run roll-up (wall time of dsb_multi_lca_counts, both calls).  Every GPU step runs under its own time limit and the
# script ends at the first failure.
#   tests/tools/lca_cost.sh [outdir (default: a new temporary directory)] [MBP]
cd "$(dirname "$0")/../.."
ROOT=$PWD; OUT=$(realpath -m "${1:-$(mktemp -d)}"); MBP=${2:-320}; mkdir -p "$OUT"
G=$ROOT/desamba_amd/bin/deSAMBA; I=$ROOT/data/demo/index; N=$ROOT/tests/golden/analysis/nodes.dmp
echo "output: $OUT"
t() { timeout -k 10 "$@"; }
prof() {   # prof <tag> <index> <fastq> <nodes.dmp>: kernel statistics of one CLI run with the LCA flags and --abundance
	rm -rf "$OUT/prof_$1"
	(cd /tmp && t 600 rocprofv3 --kernel-trace --stats -d "$OUT/prof_$1" -o run --output-format csv -- "$G" classify --taxonomy "$4" --kraken-out /dev/shm/lca_prof.kraken \
		--kraken-report "$OUT/lca_$1.kreport" --abundance "$OUT/lca_$1.tsv" "$2" "$3" -o /dev/shm/lca_prof.sam) > "$OUT/prof_$1.log" 2>&1 || return 1
	grep -E "lca:|abundance:" "$OUT/prof_$1.log"
	f=$(find "$OUT/prof_$1" -name "*kernel_stats.csv" | head -1); cp "$f" "$OUT/$1_kernel_stats.csv"
	grep -E "Name|k_read_lca|k_lca_|k_em_collect|k_read_taxon|k_classify\(" "$OUT/$1_kernel_stats.csv" | sed -E "s/\([^\"]*\)//" | cut -c1-200
}
t 300 python -c "import __graft_entry__ as g; g.demo_dir()" > "$OUT/demo.log" 2>&1 || exit 1
t 300 python tools/gen_fastq.py "$I" /dev/shm/lca.fq 65536 50000 0.15 1001 ont 16 || exit 1
echo "== CLI, alternated"
for rep in 1 2 3; do
	t 300 "$G" classify "$I" /dev/shm/lca.fq -o /dev/shm/lca_plain.sam 2> "$OUT/lca_plain$rep.log" || exit 1
	echo "plain$rep: $(grep processed "$OUT/lca_plain$rep.log")"
	t 300 "$G" classify --taxonomy "$N" --kraken-out /dev/shm/lca.kraken --kraken-report "$OUT/lca_demo.kreport" "$I" /dev/shm/lca.fq -o /dev/shm/lca_lca.sam 2> "$OUT/lca_lca$rep.log" || exit 1
	echo "lca$rep: $(grep processed "$OUT/lca_lca$rep.log") | $(grep "lca:" "$OUT/lca_lca$rep.log")"
done
cmp /dev/shm/lca_plain.sam /dev/shm/lca_lca.sam && echo "SAM identical with and without the LCA flags"
echo "per-read lines: $(wc -l < /dev/shm/lca.kraken), report lines: $(wc -l < "$OUT/lca_demo.kreport")"
head -3 "$OUT/lca_demo.kreport"
echo "== rocprofv3, demo index"
prof demo "$I" /dev/shm/lca.fq "$N" || exit 1
rm -f /dev/shm/lca.fq /dev/shm/lca_plain.sam /dev/shm/lca_lca.sam /dev/shm/lca_prof.sam /dev/shm/lca.kraken /dev/shm/lca_prof.kraken
[ "$MBP" = 0 ] && exit 0
echo "== rocprofv3, ${MBP}-Mbp strain collection (bench.py's headline index)"
H=/tmp/lca_headline; rm -rf "$H"; mkdir -p "$H"
t 900 python tools/synth_ref.py "$H/syn.fa" "$MBP" 11 3 60 12 2> /dev/null || exit 1
t 900 python -c "import sys; sys.path.insert(0, '.'); import desamba_amd as D; st = D.build_index('$H/syn.fa', '$H/index'); print('index built in %.1f s' % st.total_s)" || exit 1
rm -f "$H/syn.fa"
# a taxonomy over the collection's reference names: the k-th distinct taxid is a strain under genus 5000000 + k / 4 under family 6000000 + k / 32
t 300 python - "$H/index" "$H/nodes.dmp" <<'PY' || exit 1
import sys
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import desamba_amd as D
import lca_lib
idx = D.Index(sys.argv[1])
tids = sorted({t for t in (lca_lib.ref_taxid(idx.ref_name(r)) for r in range(idx.n_ref)) if 1 < t < 5000000})
rows = {1: (1, "no rank")}
for k, t in enumerate(tids):
    rows[t] = (5000000 + k // 4, "no rank"); rows[5000000 + k // 4] = (6000000 + k // 32, "genus"); rows[6000000 + k // 32] = (1, "family")
with open(sys.argv[2], "w") as f:
    for t in sorted(rows):
        f.write("%d\t|\t%d\t|\t%s\t|\t\t|\n" % (t, rows[t][0], rows[t][1]))
print("taxonomy: %d taxids of %d references" % (len(tids), idx.n_ref))
PY
t 300 python tools/gen_fastq.py "$H/index" /dev/shm/lca_h.fq 65536 50000 0.15 1001 ont 16 || exit 1
for rep in 1 2; do
	t 300 "$G" classify "$H/index" /dev/shm/lca_h.fq -o /dev/shm/lca_prof.sam 2> "$OUT/lca_headline_plain$rep.log" || exit 1
	echo "headline plain$rep: $(grep processed "$OUT/lca_headline_plain$rep.log")"
	t 300 "$G" classify --taxonomy "$H/nodes.dmp" --kraken-out /dev/shm/lca_prof.kraken --kraken-report "$OUT/lca_headline.kreport" "$H/index" /dev/shm/lca_h.fq -o /dev/shm/lca_prof.sam 2> "$OUT/lca_headline$rep.log" || exit 1
	echo "headline lca$rep: $(grep processed "$OUT/lca_headline$rep.log") | $(grep "lca:" "$OUT/lca_headline$rep.log")"
done
echo "report lines: $(wc -l < "$OUT/lca_headline.kreport")"; head -4 "$OUT/lca_headline.kreport"
prof headline "$H/index" /dev/shm/lca_h.fq "$H/nodes.dmp"; rc=$?
rm -rf "$H" /dev/shm/lca_h.fq /dev/shm/lca_prof.sam /dev/shm/lca_prof.kraken
exit $rc
