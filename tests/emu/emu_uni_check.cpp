// TEST INFRASTRUCTURE: what DSB_UNI promises, checked on the 64-lane emulation (tests/emu/dsb_uni_check.h, emu_simt.cpp).
//
// The emulation runs a lane alone from one cross-lane operation to the next (a superstep) and lets the next lane run the same
// superstep from the same memory; its rendezvous ends the superstep for all 64 at once (dsb_emu_stats: the count of finished
// supersteps is the same for every lane while it runs superstep k).  So the lanes that pass a DSB_UNI site in superstep k are the
// lanes that are there together on the hardware, and they pass the sites of the superstep in the same order; a lane that is not
// there (a section under `lane < n`, a DSB_SERIAL section) leaves sites out.  The first lane to pass a site writes (site, value)
// to the superstep's list; every later lane finds its next entry of that site from where it stands in the list and compares.
// A value that differs is a finding: the site (source line of dsb_classify_dev.h), the read the harness named, both lanes and values.
// (The emulation's own rendezvous, dsb_emu_exchange, cannot carry the comparison: it waits for all 64 lanes, and DSB_UNI may stand in a
// section that only some of them run.)
// The limit of matching by order: the k-th pass of a lane at a site is compared with the k-th entry of that site the lane has not yet
// gone past.  In wave-uniform code that is the same loop iteration.  A lane that passes a site FEWER times than the first lane did in
// one superstep (a DSB_UNI under a lane-dependent `if` inside a loop without a cross-lane operation) is compared with an earlier
// iteration's entry -- a finding may then name the wrong occurrence, or a real difference in a later one go unseen; and a site that
// the first lanes of a superstep did not pass is only compared among the lanes that come after the one that entered it.  Such
// placements are against the macro's rule anyway (never in per-lane code); the self-test covers the plain cases only.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <map>
#include <string>
#include <vector>

extern "C" int dsb_emu_cur_lane;
extern "C" void dsb_emu_stats(unsigned long *v);
extern "C" void dsb_emu_run(void (*fn)(void *), void *arg);
extern "C" const uint64_t *dsb_emu_exchange(uint64_t v, int site);

namespace {
struct Entry { int site; uint64_t v; int lane; };
struct Finding { int site, read, lane_a, lane_b; uint64_t va, vb; unsigned long count; };
std::vector<Entry> g_list;                 // the sites passed in the current superstep, in the order of the first lane that passed them
unsigned long g_step = ~0ul;               // ... which superstep that is
size_t g_cursor[64]; unsigned long g_lane_step[64];
std::map<int, Finding> g_findings;
unsigned long g_checked;
int g_read = -1;
}

extern "C" uint64_t dsb_uni_check(uint64_t v, int site)
{
	unsigned long st[4]; dsb_emu_stats(st);
	const unsigned long step = st[1]; const int lane = dsb_emu_cur_lane & 63;
	if (step != g_step) { g_list.clear(); g_step = step; }
	if (g_lane_step[lane] != step) { g_cursor[lane] = 0; g_lane_step[lane] = step; }
	g_checked++;
	for (size_t i = g_cursor[lane]; i < g_list.size(); i++) {
		if (g_list[i].site != site || g_list[i].lane == lane) continue;    // (its own entries: the lane was the first at a site it passes again)
		g_cursor[lane] = i + 1;
		if (g_list[i].v != v) {
			auto it = g_findings.find(site);
			if (it != g_findings.end()) it->second.count++;
			else g_findings[site] = Finding{site, g_read, g_list[i].lane, lane, g_list[i].v, v, 1};
		}
		return v;
	}
	// the first lane here.  A lane at the end of the list goes on behind its entry; one that has entries of other lanes still in front of
	// it stays where it is: what it passes next may be one of them
	if (g_cursor[lane] == g_list.size()) g_cursor[lane]++;
	g_list.push_back(Entry{site, v, lane});
	return v;
}
// the read the next findings belong to
extern "C" void dsb_uni_set_read(int r) { g_read = r; }
extern "C" unsigned long dsb_uni_checked(void) { return g_checked; }
// findings since the last call as text, one per line; returns their number
extern "C" int dsb_uni_report(char *out, size_t cap)
{
	size_t o = 0; int n = 0;
	for (auto &kv : g_findings) {
		const Finding &f = kv.second;
		if (out && o < cap) o += (size_t)snprintf(out + o, cap - o, "DSB_UNI at line %d (#%d) read %d: lane %d holds %#llx, lane %d holds %#llx (x%lu)\n", f.site >> 10, f.site & 1023, f.read,
		                                          f.lane_a, (unsigned long long)f.va, f.lane_b, (unsigned long long)f.vb, f.count);
		n++;
	}
	g_findings.clear();
	if (out && cap) out[o < cap ? o : cap - 1] = 0;
	return n;
}
// a tiny kernel for the checker itself: a uniform value, a wave_sync, a value that depends on the lane (site 2 << 10: to be reported),
// a uniform value in a section only three lanes run, and a uniform value all lanes pass after it
extern "C" void dsb_uni_selftest(void)
{
	dsb_emu_run([](void *) {
		const int lane = dsb_emu_cur_lane;
		dsb_uni_check(7, 1 << 10);
		dsb_emu_exchange(0, 1);
		dsb_uni_check((uint64_t)(lane & 1), 2 << 10);
		if (lane >= 5 && lane < 8) dsb_uni_check(5, 3 << 10);
		dsb_uni_check(9, 4 << 10);
	}, nullptr);
}
