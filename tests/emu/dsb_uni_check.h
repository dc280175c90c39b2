// TEST INFRASTRUCTURE: the checking definitions of DSB_UNI / DSB_UNI64 (desamba_amd/csrc/dsb_classify_dev.h: "all lanes that are here
// hold this value").  tests/emu/build_emu64_uni.sh puts this file in front of the device code (-include) in a second build of the
// 64-lane emulation; every DSB_UNI then hands its value to tests/emu/emu_uni_check.cpp, which compares it with what the other lanes
// of the wavefront hand in at the same place in the same stretch between two cross-lane operations, and records site and read where
// two lanes differ.  A site is the source line and the number of the macro's expansion in the unit.
#include <stdint.h>
extern "C" uint64_t dsb_uni_check(uint64_t v, int site);
#define DSB_UNI_SITE ((int)((__LINE__ << 10) | (__COUNTER__ & 1023)))
#define DSB_UNI(v) ((decltype(+(v)))dsb_uni_check((uint64_t)(uint32_t)(v), DSB_UNI_SITE))
#define DSB_UNI64(v) ((decltype(+(v)))dsb_uni_check((uint64_t)(v), DSB_UNI_SITE))
