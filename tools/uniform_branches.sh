#!/bin/bash
# How the classify kernels branch (device-only compile to assembly, as tools/kernel_resources.sh compiles; nothing is written into the
# tree): per kernel the instruction count, the branches on the execution mask (a divergent `if` or loop: s_cbranch_execz/execnz), the
# scalar branches (s_cbranch_scc*/vcc*: a condition the compiler knows to be the same in all lanes), *_saveexec_b64, v_cmp* and
# v_readfirstlane.  A wave-uniform value that the compiler cannot see to be uniform costs a v_cmp, a saveexec and a mask branch per
# test; through DSB_UNI (dsb_classify_dev.h) it costs an s_cmp and a scalar branch.
# usage: tools/uniform_branches.sh [csrc-dir] [hipcc flags...]
src=${1:-$(dirname "$0")/../desamba_amd/csrc}; [ $# -gt 0 ] && shift
inc=$(dirname "$0")/../include
out=$(mktemp -d)
for k in 1 4 5; do              # the units of k_classify, k_classify_heavy<8> and k_anchor (dsb_gpu.hip)
	/opt/rocm/bin/hipcc -O3 -fno-strict-aliasing --offload-arch=gfx950 -std=c++17 -Wno-unused-value -I"$inc" -S --cuda-device-only -DDSB_KUNIT=$k "$@" \
		"$src/dsb_gpu.hip" -o "$out/x$k.s" 2> "$out/e$k.txt" &
done
wait
printf '%-20s %8s %8s %8s %8s %8s %8s\n' kernel insts mask_br scalar_br saveexec v_cmp v_rfl
for k in 1 4 5; do
	[ -s "$out/x$k.s" ] || { echo "unit $k did not compile:"; cat "$out/e$k.txt"; continue; }
	awk '
		/^_Z[0-9]+k_[a-z_]+.*:/ { s = $1; sub(/^_Z/, "", s); l = s + 0; name = substr(s, length(l "") + 1, l); rest = substr(s, length(l "") + 1 + l);
			if (match(rest, /^ILi[0-9]+E/)) name = name "<" substr(rest, 4, RLENGTH - 4) ">";      # the template argument: k_classify_heavy<8>
			in_k = 1; n = mb = sb = se = vc = rf = 0; next }
		in_k && /^\.Lfunc_end/ { printf "%-20s %8d %8d %8d %8d %8d %8d\n", name, n, mb, sb, se, vc, rf; in_k = 0; next }
		in_k && /^\t[a-z]/ && $1 !~ /^\./ {
			n++
			if ($1 ~ /^s_cbranch_exec/) mb++
			else if ($1 ~ /^s_cbranch_(scc|vcc)/) sb++
			else if ($1 ~ /_saveexec_b64$/) se++
			else if ($1 ~ /^v_cmpx?_/) vc++
			else if ($1 ~ /^v_readfirstlane/) rf++
		}' "$out/x$k.s"
done
rm -rf "$out"
