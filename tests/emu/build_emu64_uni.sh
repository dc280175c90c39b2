#!/bin/bash
# tests/emu/libdsbemu64_uni.so: the 64-lane emulation of build_emu64.sh, same sources, with the checking DSB_UNI of
# tests/emu/dsb_uni_check.h in front of the device code: every value that goes through DSB_UNI is compared across the lanes that are
# there (emu_uni_check.cpp).  No sanitizer runtime is linked or loaded (-fsanitize=thread: instrumentation hooks only, emu_simt.cpp).
set -e
cd "$(dirname "$0")/../.."
tmp=$(mktemp -d); trap 'rm -rf "$tmp"' EXIT
I="-Idesamba_amd/csrc -Iinclude -Itests/emu"
g++ -std=c++17 -O1 -g -fsanitize=thread -fno-strict-aliasing -fPIC -DDSB_HOST_EMU -DDSB_EMU_LANES=64 $I -include tests/emu/dsb_uni_check.h -c tests/emu/emu_classify.cpp -o "$tmp/classify.o" &
g++ -std=c++17 -O2 -g -fPIC -c tests/emu/emu_simt.cpp -o "$tmp/simt.o" &
g++ -std=c++17 -O2 -g -fPIC -c tests/emu/emu_uni_check.cpp -o "$tmp/uni.o" &
g++ -std=c++17 -O2 -fno-strict-aliasing -fPIC -DDSB_HOST_EMU $I -c desamba_amd/csrc/dsb_index.cpp -o "$tmp/index.o" &
wait
g++ -shared -o tests/emu/libdsbemu64_uni.so "$tmp/classify.o" "$tmp/simt.o" "$tmp/uni.o" "$tmp/index.o" -ldl
