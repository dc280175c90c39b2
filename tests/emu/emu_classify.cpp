// TEST INFRASTRUCTURE: runs the DEVICE code of desamba_amd (dsb_classify_dev.h, dsb_probe.h) on the
// host (-DDSB_HOST_EMU) -- as a 1-lane wave (libdsbemu.so: fast, the per-read logic) or as 64 lanes on cooperative
// fibers with a race detector (-DDSB_EMU_LANES=64 -fsanitize=thread + emu_simt.cpp, libdsbemu64.so: every cross-lane operation, every lane's indexing) -- so
// it can be checked against the oracle with `pytest -m "not gpu"`, gdb and sanitizers.  Not linked into libdesamba_amd.so.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "dsb_device.h"
#include "dsb_probe.h"
#include "dsb_seed_scan.h"
#include "dsb_classify_dev.h"
#include "dsb_host.h"
using namespace dsb_g64;

struct EmuRegion { const void *p; size_t n; const char *name; };
struct EmuCtx {
	std::vector<EmuRegion> regions;       // the arrays a lane may touch (64-lane emulation: emu_simt.cpp checks every access against them)
	dsb_index *idx = nullptr;
	DsbDevIndex dx; std::vector<uint8_t> arena; uint32_t max_len; WCtx w; size_t sms_off;
	std::vector<uint8_t> bin; std::vector<uint64_t> pk, bits;
	std::vector<DsbSeed> seedsF, seedsR;
	uint32_t limit_set = 0;
	uint32_t cnt[4];          // work counters of the last read (occ, MEM searches, SA lookups, reference bases)
};

static size_t al(size_t v) { return (v + 255) & ~(size_t)255; }

extern "C" void *emu_new(dsb_index *idx, int min_len, int min_score)
{
	const DsbHostIndex *h = dsb_index_host(idx);
	EmuCtx *e = new EmuCtx(); e->idx = idx;
	DsbDevIndex &dx = e->dx; memset(&dx, 0, sizeof dx);
	dx.ek0 = h->ek0; dx.ek1 = h->ek1; dx.ek_mask = h->ek_mask; dx.ek_len = h->ek_len; dx.single_base_max = h->single_base_max;
	dx.fm = h->fm; dx.fm_sb = h->fm_sb; dx.bwt_len = h->bwt_len; memcpy(dx.rank, h->rank, sizeof dx.rank); dx.dollar_pos = h->dollar_pos; dx.dollar_row = h->dollar_row;
	dx.hash_index = h->hash_c ? nullptr : h->hash_index; dx.hash_c = h->hash_c; dx.sa = (const uint2 *)h->sa; dx.uni = (const uint2 *)h->uni; dx.refpos = h->refpos; dx.refbin = h->refbin; dx.ref_bases = h->n_refbin * 4;
	dx.refinfo = h->refinfo; dx.qmem = h->Q_MEM; dx.qlv = &h->Q_LV[0][0];
	dx.filter_min_length = min_len; dx.filter_min_score = min_score; dx.filter_min_score_LV3 = min_score + 10;
	e->max_len = 0;
	return e;
}
extern "C" void emu_free(void *p) { delete (EmuCtx *)p; }

static void setup_arena(EmuCtx *e, uint32_t L)
{
	if (L <= e->max_len) return;
	e->max_len = L + L / 4 + 1024;
	e->dx.sms_cap = getenv("DSB_EMU_SMS_CAP") ? (uint32_t)atol(getenv("DSB_EMU_SMS_CAP")) : dsb_sms_cap_for(e->max_len);
	size_t o = 0, off[20], len[20]; int k = 0;
	auto add = [&](size_t n) { len[k] = n; off[k++] = o; o += al(n); };
	add(((size_t)(e->max_len >> 1) + 64) * sizeof(DsbSeed));            // 0 seeds
	add((size_t)DSB_ANC_CAP * sizeof(DsbAnchor)); add((size_t)DSB_ANC_CAP * sizeof(DsbAnchor));  // 1,2
	add((size_t)DSB_HIT_CAP * sizeof(DsbChain)); add((size_t)DSB_HIT_CAP * sizeof(DsbChain));    // 3,4
	add((size_t)e->dx.sms_cap * sizeof(DsbSms)); e->sms_off = off[5];      // 5
	add(256);                                                            // 6 (unused)
	add((size_t)(256 + 2 * 400 + 64) * sizeof(DsbScHash));               // 7
	add((size_t)DSB_MEMSLOW_CAP * sizeof(DsbMem));                       // 8
	add((size_t)DSB_SPHASH * 8); add(1024 * sizeof(int));                // 9,10
	add((size_t)2 * DSB_ANC_CAP * 8); add((size_t)2 * DSB_ANC_CAP * 4);  // 11,12
	add(3 * DSB_REFWIN + DSB_REFWIN_FRONT);                                                 // 13
	add((size_t)DSB_WAVE * DSB_LANE_ANC_CAP * sizeof(DsbAnchor)); add((size_t)DSB_WAVE * DSB_SPHASH * 8); add(((size_t)(e->max_len >> 1) + 64) * 4);   // 14,15,16 (per-lane scratch)
	add(((size_t)(e->max_len >> 1) + 64) * 4);                           // 17 island records of fast_classify
	e->arena.assign(o + 256, 0xCD);
	memset(e->arena.data() + off[9], 0, DSB_SPHASH * 8); memset(e->arena.data() + off[15], 0, (size_t)DSB_WAVE * DSB_SPHASH * 8); e->w.sp_gen = 0;
	uint8_t *s = e->arena.data(); WCtx &w = e->w;
	{
		static const char *nm[18] = {"seeds", "anchors", "anchors (copy)", "chains", "chains (copy)", "match nodes", "(unused)", "chain-end hash", "slow-path MEMs", "visited rows", "score_v",
		                            "sort keys", "sort indices", "reference windows", "lane anchors", "lane visited rows", "top islands", "island records"};
		e->regions.clear();
		for (int i = 0; i < k && i < 18; i++) e->regions.push_back(EmuRegion{s + off[i], len[i], nm[i]});
	}
	w.x = &e->dx; w.dbg = nullptr;
	w.seeds = (DsbSeed *)(s + off[0]); w.anc = (DsbAnchor *)(s + off[1]); w.anc_tmp = (DsbAnchor *)(s + off[2]);
	w.hit = (DsbChain *)(s + off[3]); w.hit_tmp = (DsbChain *)(s + off[4]); w.sms = (DsbSms *)(s + off[5]);
	alignas(16) static uint32_t emu_wtab[DSB_WTAB_SLOTS]; w.wtab = emu_wtab;
	w.sc = (DsbScHash *)(s + off[7]); w.mem_slow = (DsbMem *)(s + off[8]); w.spset = (uint64_t *)(s + off[9]); w.score_v = (int *)(s + off[10]);
	w.sortkey = (uint64_t *)(s + off[11]); w.sortidx = (uint32_t *)(s + off[12]);
	w.win_mid = s + off[13] + DSB_REFWIN_FRONT; w.win_right = w.win_mid + DSB_REFWIN; w.win_left = w.win_right + DSB_REFWIN;
	static uint4 emu_ring[DSB_RING]; w.ring = emu_ring; static DpBatch emu_dpb; w.dpb = &emu_dpb;
	static uint32_t emu_red[4]; w.red = emu_red; w.round_info = (uint32_t *)(s + off[17]);
	w.lane_anc = (DsbAnchor *)(s + off[14]); w.lane_spset = (uint64_t *)(s + off[15]); w.top_idx = (uint32_t *)(s + off[16]); w.anc_cap = DSB_ANC_CAP;
	w.heavy_limit = 0;
	w.anc_cap_main = DSB_ANC_CAP; w.hit_cap = DSB_HIT_CAP; w.step_limit = getenv("DSB_EMU_STEP_LIMIT") ? (uint32_t)atol(getenv("DSB_EMU_STEP_LIMIT")) : DSB_STEP_LIMIT;
}

// returns n_hits (or -status when a cap/timeout status was raised); hits as DsbHitOut
extern "C" int emu_classify(void *p, const char *seq, uint32_t L, int hist_max, DsbHitOut *out, int max_out, uint8_t *bitsF_out, uint8_t *bitsR_out)
{
	EmuCtx *e = (EmuCtx *)p; const DsbDevIndex &dx = e->dx;
	setup_arena(e, L);
	// k_encode_bytes
	e->bin.assign(DSB_QPAD_L + 2 * (size_t)L + DSB_QPAD_R, 0);
	uint8_t *F = e->bin.data() + DSB_QPAD_L, *R = F + L;
	for (uint32_t i = 0; i < L; i++) { unsigned char ch = seq[i]; uint32_t c = (ch == 'A' || ch == 'a') ? 0u : (ch == 'G' || ch == 'g') ? 2u : (ch == 'T' || ch == 't') ? 3u : 1u; F[i] = c; R[L - 1 - i] = 3 - c; }
	memset(R + L, DSB_QPAD_R_VAL, DSB_QPAD_R);
	// k_encode_pack
	uint32_t nw = (L + 31) / 32 + 1;
	e->pk.assign(2 * (size_t)nw, 0);
	for (uint32_t t = 0; t < 2 * nw; t++) {
		uint32_t sr = t >= nw, wi = sr ? t - nw : t; const uint8_t *S = sr ? R : F; uint64_t v = 0;
		for (uint32_t b = 0; b < 32; b++) { uint32_t q = wi * 32 + b; v = (v << 2) | (q < L ? S[q] : 0u); }
		e->pk[t] = v;
	}
	// k_seed_probe
	uint32_t n_win = L >= 40 ? L - dx.ek_len + 1 : 0, n_words = (n_win + 63) / 64;
	e->bits.assign(2 * (size_t)n_words + 2, 0);
	uint64_t kmask = dx.ek_len >= 32 ? ~0ULL : ((1ULL << (2 * dx.ek_len)) - 1ULL);
	for (int s = 0; s < 2; s++)
		for (uint32_t q = 0; q < n_win; q++) {
			int t1 = 0;
			int hit = dsb_probe_window(e->pk.data() + (s ? nw : 0), q, dx.ek_len, kmask, dx.single_base_max, dx.ek0, dx.ek1, dx.ek_mask, &t1);
			if (hit) e->bits[(s ? n_words : 0) + (q >> 6)] |= 1ULL << (q & 63);
			uint8_t *bo = s ? bitsR_out : bitsF_out;
			if (bo) bo[q] = (uint8_t)hit;
		}
	WCtx &w = e->w;
	if (e->limit_set) w.step_limit = e->limit_set;
	memset(e->cnt, 0, sizeof e->cnt); w.k.c = e->cnt; w.k.uni = 1;
	w.bin = F; w.L = L; w.status = 0; w.max_read_l = hist_max;
	w.mw = nullptr; w.n_waves = 1;
	w.pre_seeds = nullptr; w.pre_info = nullptr; w.pk[0] = getenv("DSB_EMU_NO_GAP_LANE") ? nullptr : e->pk.data(); w.pk[1] = w.pk[0] ? w.pk[0] + nw : nullptr;
#if DSB_EMU_LANES == 64
	struct Job { WCtx *w; const uint64_t *bF, *bR; } job = {&w, e->bits.data(), e->bits.data() + n_words};
	{	// every array a lane may touch, by name
		const DsbHostIndex *h = dsb_index_host(e->idx);
		dsb_emu_regions_clear();
		for (const EmuRegion &r : e->regions) dsb_emu_region(r.p, r.n, r.name);
		dsb_emu_region(&job, sizeof job, "job"); dsb_emu_region(e, sizeof *e, "context (WCtx, index descriptor, counters)");
		dsb_emu_region(w.wtab, 4 * DSB_WTAB_SLOTS, "LDS window table"); dsb_emu_region(w.ring, sizeof(uint4) * DSB_RING, "LDS ring"); dsb_emu_region(w.dpb, sizeof(DpBatch), "LDS DP batch"); dsb_emu_region(w.red, 16, "LDS red");
		dsb_emu_region(e->bin.data(), e->bin.size(), "byte strands"); dsb_emu_region(e->pk.data(), 8 * e->pk.size(), "packed strands"); dsb_emu_region(e->bits.data(), 8 * e->bits.size(), "hit bits");
		dsb_emu_region(h->ek0, h->ek_size, "filter table 0"); dsb_emu_region(h->ek1, h->ek_size, "filter table 1"); dsb_emu_region(h->fm, h->n_fm * sizeof(DsbFmBlock), "rank lines");
		if (h->fm_sb) dsb_emu_region(h->fm_sb, h->n_fm_sb * 40, "rank superblocks");
		if (h->hash_c) dsb_emu_region(h->hash_c, (size_t)h->n_hash_c * sizeof(DsbHiLine), "13-mer table (compressed)"); else dsb_emu_region(h->hash_index, (((size_t)1 << 26) + 1) * 8, "13-mer table");
		dsb_emu_region(h->sa, h->sa_size * 8, "SA samples"); dsb_emu_region(h->uni, (h->n_uni + 1) * 8, "unitigs"); dsb_emu_region(h->refpos, (h->n_refpos + 1) * 8, "reference positions");
		dsb_emu_region(h->refbin, h->n_refbin + 4096, "reference text"); dsb_emu_region(h->refinfo, h->n_ref * sizeof(DsbRefInfo), "reference info");
		dsb_emu_region(h->Q_MEM, 2000 * sizeof(int), "Q_MEM"); dsb_emu_region(&h->Q_LV[0][0], 400 * sizeof(int), "Q_LV");
	}
	dsb_emu_run([](void *a) { Job *j = (Job *)a; classify_read<false>(*j->w, j->bF, j->bR); }, &job);
#else
	classify_read<false>(w, e->bits.data(), e->bits.data() + n_words);
#endif
	if (w.status) return -(w.status | (w.stage << 8));
	int n = (int)w.n_hit < max_out ? (int)w.n_hit : max_out;
	for (int i = 0; i < n; i++) {
		DsbChain h = w.hit[i]; DsbHitOut o;
		o.ref_ID = h.ref_ID; o.t_st = h.t_st; o.t_ed = h.t_ed; o.q_st = h.q_st; o.q_ed = h.q_ed; o.sum_score = h.sum_score; o.indel = h.indel;
		o.direction = h.direction; o.primary = h.primary; o.pri_index = h.pri_index; o.pad = 0;
		out[i] = o;
	}
	return (int)w.n_hit;
}

extern "C" int emu_seeds(void *p, int strand, DsbSeed *out, int max_out, uint32_t *total)
{
	EmuCtx *e = (EmuCtx *)p; WCtx &w = e->w;
	SDir *sd = (w.sd[0].direction == (uint32_t)strand) ? &w.sd[0] : &w.sd[1];
	int n = (int)sd->l_seed_v < max_out ? (int)sd->l_seed_v : max_out;
	for (int i = 0; i < n; i++) out[i] = sd->seed_v[i];
	if (total) *total = sd->total_score;
	return (int)sd->l_seed_v;
}

#if DSB_EMU_LANES == 64
// the detector on four tiny kernels: 0 clean (a sync between the exchange), 1 conflicting stores, 2 a read of what the neighbour
// writes in the same stretch, 3 a store behind the registered array; -> number of findings, their text in out
extern "C" int dsb_emu_findings(char *out, size_t cap);
extern "C" int emu_selftest(int what, char *out, size_t cap)
{
	static uint32_t shared[128];
	struct J { uint32_t *s; int what; } j = {shared, what};
	dsb_emu_regions_clear(); dsb_emu_region(shared, 64 * 4, "selftest array (64 words)"); dsb_emu_region(&j, sizeof j, "job");
	memset(shared, 0, sizeof shared);
	dsb_emu_findings(nullptr, 0);
	dsb_emu_run([](void *a) {
		J *j = (J *)a; const int lane = DSB_LANE;
		if (j->what == 0) { j->s[lane] = (uint32_t)lane; wave_sync(); j->s[63 - lane] += 1; }
		if (j->what == 1) j->s[0] = (uint32_t)lane;
		if (j->what == 2) { j->s[lane] = 7; j->s[lane] += j->s[(lane + 1) & 63]; }
		if (j->what == 3) j->s[lane + 64] = 1;
	}, &j);
	if (what == 0) for (int i = 0; i < 64; i++) if (shared[i] != (uint32_t)i + 1) return -1;
	return dsb_emu_findings(out, cap);
}
#endif

#ifdef EMU_MAIN
int main(int argc, char **argv)
{
	dsb_index *idx; if (dsb_index_open(argv[1], &idx)) return 1;
	void *e = emu_new(idx, 170, 64);
	FILE *f = fopen(argv[2], "r"); static char line[1 << 20]; long n = 0; int hist = 0; int limit = argc > 3 ? atoi(argv[3]) : 1 << 30;
	DsbHitOut hits[512];
	while (fgets(line, sizeof line, f)) {
		if (n % 4 == 1) {
			size_t l = strlen(line); if (l && line[l - 1] == '\n') line[--l] = 0;
			int nh = emu_classify(e, line, (uint32_t)l, hist, hits, 512, NULL, NULL);
			if ((int)l > hist) hist = (int)l;
			printf("read %ld len %zu nh %d", n / 4, l, nh);
			for (int i = 0; i < nh && i < 3; i++) printf(" [%u %u %u %u %u AS %u d%u p%u/%u]", hits[i].ref_ID, hits[i].t_st, hits[i].t_ed, hits[i].q_st, hits[i].q_ed, hits[i].sum_score, hits[i].direction, hits[i].primary, hits[i].pri_index);
			printf("\n");
			if (n / 4 + 1 >= limit) break;
		}
		n++;
	}
	return 0;
}
#endif

// high-water mark of the match-node arena since the arena was (re)built (its fill pattern is 0xCD)
extern "C" uint32_t emu_sms_peak(void *p)
{
	EmuCtx *e = (EmuCtx *)p; const uint32_t *a = (const uint32_t *)(e->arena.data() + e->sms_off);
	size_t n = (size_t)e->dx.sms_cap * 4;
	while (n && a[n - 1] == 0xCDCDCDCDu) n--;
	return (uint32_t)((n + 3) / 4);
}
// ---- one round of a lane of k_seed_scan, stage by stage: a RESTATEMENT of the per-lane part of the kernel's loop (dsb_gpu.hip), line for line
// but for the names of the word cache.  (As functions of dsb_seed_scan.h that the kernel calls too, the kernel's resource line stayed the
// parent's but its ISA did not, and the benchmark's seed lookup on the strain index came out 0.7 % slower than the parent's own spread allows:
// DESIGN.md.  The device leg of tests/test_stage_seed.py is what covers the kernel's own text.)
// packed words wbase .. wbase + 2 of the forward strand (reverse-strand lanes keep them reverse-complemented); none yet: no index is near wbase
struct DsbScanWords { uint64_t K0, K1, K2; uint32_t wbase; };
DSB_SCAN_FN void dsb_scan_words_init(DsbScanWords &c) { c.K0 = c.K1 = c.K2 = 0; c.wbase = 0xfffffff0u; }
DSB_SCAN_FN uint32_t dsb_scan_lowest(const uint32_t (&want)[DSB_SCAN_W])
{
	uint32_t lo = DSB_SCAN_NONE;
#pragma unroll
	for (int t = 0; t < DSB_SCAN_W; t++) lo = want[t] < lo ? want[t] : lo;
	return lo;
}
// the three packed words that hold the wanted k-mers (lo: the smallest wanted window, not DSB_SCAN_NONE): a sliding window in registers, a
// word is loaded only when the scan has moved past the ones at hand (the texture addresser, not the memory behind it, is what the kernel
// saturates: every lane's load is a request of its own)
DSB_SCAN_FN void dsb_scan_words_fetch(DsbScanWords &c, const uint64_t *P, uint32_t lo, bool rc)
{
	const uint32_t wi = lo >> 5;
	uint64_t n0, n1, n2;
#define DSB_SCAN_WORD(dst, idx) \
	if ((idx) == c.wbase) dst = c.K0; else if ((idx) == c.wbase + 1) dst = c.K1; else if ((idx) == c.wbase + 2) dst = c.K2; \
	else { dst = P[idx]; if (rc) dst = dsb_revcomp_kmer(dst, 32); }
	DSB_SCAN_WORD(n0, wi) DSB_SCAN_WORD(n1, wi + 1) DSB_SCAN_WORD(n2, wi + 2)
#undef DSB_SCAN_WORD
	c.K0 = n0; c.K1 = n1; c.K2 = n2; c.wbase = wi;
}
// k-mer, low-complexity filter and first hash of every wanted window (base: the first window of the word of the smallest).  Forward
// lanes: bases of the block in order K0 K1 K2, window at rel; reverse lanes: the block reverse-complemented is rc(K2) rc(K1) rc(K0), and
// the reverse complement of the k-mer at rel is the k-mer at 96 - rel - k of that block.  p0 counts the windows that pass the filter.
DSB_SCAN_FN void dsb_scan_kmers(const DsbScanWords &c, const uint32_t (&want)[DSB_SCAN_W], uint32_t base, bool rc, int k, uint64_t kmask, int sbm, uint64_t ek_mask,
                                uint64_t (&km)[DSB_SCAN_W], uint64_t (&h1)[DSB_SCAN_W], bool (&ok)[DSB_SCAN_W], uint32_t &p0)
{
	const uint64_t B0 = rc ? c.K2 : c.K0, B1 = c.K1, B2 = rc ? c.K0 : c.K2;
#pragma unroll
	for (int t = 0; t < DSB_SCAN_W; t++) {
		ok[t] = want[t] != DSB_SCAN_NONE; km[t] = 0; h1[t] = 0;
		if (ok[t]) {
			uint32_t rel = want[t] - base;                                // < 64: the window starts in the first or second word
			if (rc) rel = 96u - rel - (uint32_t)k;                        // 12 .. 80
			const uint64_t a = rel < 32 ? B0 : rel < 64 ? B1 : B2, b = rel < 32 ? B1 : B2; const uint32_t sh = (rel & 31u) * 2;
			const uint64_t hi = sh ? ((a << sh) | (b >> (64 - sh))) : a;
			const uint64_t v = (hi >> (64 - 2 * k)) & kmask;
			ok[t] = dsb_kmer_ok(v, k, sbm); km[t] = v;
			if (ok[t]) { p0++; h1[t] = dsb_ph1(v) & ek_mask; }
		}
	}
}
// table 0 (get_exist_kmer, src/cly.c:956-972); returns whether any window of the lane goes on to table 1
DSB_SCAN_FN bool dsb_scan_table0(const uint8_t *ek0, const uint64_t (&h1)[DSB_SCAN_W], bool (&ok)[DSB_SCAN_W])
{
	uint8_t t0[DSB_SCAN_W];
#pragma unroll
	for (int t = 0; t < DSB_SCAN_W; t++) { t0[t] = 0; if (ok[t]) t0[t] = ek0[h1[t] >> 3]; }
	bool any1 = false;
#pragma unroll
	for (int t = 0; t < DSB_SCAN_W; t++) { ok[t] = ok[t] && ((t0[t] >> (7 - (h1[t] & 7))) & 1); any1 |= ok[t]; }
	return any1;
}
// table 1 in two steps, its loads first: p1 counts the probes made
DSB_SCAN_FN void dsb_scan_table1_load(const uint8_t *ek1, uint64_t ek_mask, const uint64_t (&km)[DSB_SCAN_W], const bool (&ok)[DSB_SCAN_W],
                                      uint8_t (&t1)[DSB_SCAN_W], uint64_t (&h2)[DSB_SCAN_W], uint32_t &p1)
{
#pragma unroll
	for (int t = 0; t < DSB_SCAN_W; t++) { t1[t] = 0; h2[t] = 0; if (ok[t]) { h2[t] = dsb_ph2(km[t]) & ek_mask; t1[t] = ek1[h2[t] >> 3]; p1++; } }
}
// bit t of the result = window want[t] hit
DSB_SCAN_FN uint32_t dsb_scan_table1_bits(const bool (&ok)[DSB_SCAN_W], const uint8_t (&t1)[DSB_SCAN_W], const uint64_t (&h2)[DSB_SCAN_W])
{
	uint32_t bits = 0;
#pragma unroll
	for (int t = 0; t < DSB_SCAN_W; t++) if (ok[t] && ((t1[t] >> (7 - (h2[t] & 7))) & 1)) bits |= 1u << t;
	return bits;
}

// ---- the seed lookup on its own (tests/test_stage_seed.py).  One lane of k_seed_scan: the state machine of dsb_seed_scan.h and the round
// functions above in the kernel's order, without the wavefront votes (a lane whose neighbours go on to table 1 runs the table-1 step with
// nothing to ask, which changes nothing).  P: the packed words of the forward strand, followed by the reverse strand's as on the device.
// cnt: [0] windows that passed the low-complexity filter (the kernel's first counter), [1] windows asked for, [2] table-1 probes (the
// second counter), [3] rounds, [4] packed words loaded from memory
struct ScanLane { std::vector<DsbSeed> sv; uint32_t ns = 0, total = 0, cnt[5] = {0, 0, 0, 0, 0}; };
static void scan_lane(const uint64_t *P, uint32_t n, int k, int sbm, const uint8_t *ek0, const uint8_t *ek1, uint64_t ek_mask, const uint8_t *summ, int summ_shift,
                      bool rc, DsbScanLook look, ScanLane &o)
{
	const uint64_t kmask = k >= 32 ? ~0ULL : ((1ULL << (2 * k)) - 1ULL);
	std::vector<DsbSeed> &sv = o.sv;
	auto store = [&](uint32_t idx, uint32_t off, uint32_t len) { if (sv.size() <= idx) sv.resize(idx + 1); sv[idx].offset = off; sv[idx].len = (uint16_t)len; sv[idx].top = 0; };
	auto mark = [&](uint32_t idx) { sv[idx].top = 1; };
	DsbScan s; dsb_scan_init(s, n, look);
	uint32_t p0 = 0, p1 = 0;
	DsbScanWords kw; dsb_scan_words_init(kw);
	while (s.mode != DSB_SCAN_DONE) {
		uint32_t want[DSB_SCAN_W]; dsb_scan_want(s, want);
		const uint32_t lo = dsb_scan_lowest(want);
		if (lo != DSB_SCAN_NONE) {
			const uint32_t wi = lo >> 5;
			for (uint32_t q = wi; q < wi + 3; q++) if (q - kw.wbase > 2u) o.cnt[4]++;
			dsb_scan_words_fetch(kw, P, lo, rc);
		}
		for (int t = 0; t < DSB_SCAN_W; t++) if (want[t] != DSB_SCAN_NONE) o.cnt[1]++;
		uint64_t km[DSB_SCAN_W], h1[DSB_SCAN_W]; bool ok[DSB_SCAN_W];
		dsb_scan_kmers(kw, want, lo & ~31u, rc, k, kmask, sbm, ek_mask, km, h1, ok, p0);
		if (summ) {          // (the kernel's own four lines)
			uint8_t sb[DSB_SCAN_W];
			for (int t = 0; t < DSB_SCAN_W; t++) { sb[t] = 0xff; if (ok[t]) sb[t] = summ[(h1[t] >> summ_shift) >> 3]; }
			for (int t = 0; t < DSB_SCAN_W; t++) ok[t] = ok[t] && ((sb[t] >> ((h1[t] >> summ_shift) & 7)) & 1);
		}
		const bool any1 = dsb_scan_table0(ek0, h1, ok);
		uint32_t bits = 0;
		if (any1) { uint8_t t1[DSB_SCAN_W]; uint64_t h2[DSB_SCAN_W]; dsb_scan_table1_load(ek1, ek_mask, km, ok, t1, h2, p1); bits = dsb_scan_table1_bits(ok, t1, h2); }
		dsb_scan_consume(s, bits, rc, store, mark);
		o.cnt[3]++;
	}
	dsb_scan_finish(s, mark);
	o.ns = s.ns; o.total = s.total; o.cnt[0] = p0; o.cnt[2] = p1;
}
static DsbScanLook look_of(const uint8_t *look, uint64_t table_bytes)
{
	DsbScanLook k = dsb_scan_look_for(table_bytes);
	if (look) { k.after_seed = look[0]; k.back_fwd = look[1]; k.fwd_n = look[2]; k.stride_n = look[3]; }
	return k;
}
static int scan_lane_out(const ScanLane &o, DsbSeed *out, int max_out, uint32_t *total, uint32_t *cnt)
{
	const int m = (int)o.ns < max_out ? (int)o.ns : max_out;
	for (int i = 0; i < m; i++) out[i] = o.sv[i];
	if (total) *total = o.total;
	if (cnt) memcpy(cnt, o.cnt, sizeof o.cnt);
	return (int)o.ns;
}
// the strands of the last read on the index of the context: the seed list of one strand (same layout as emu_seeds) and the counters of
// scan_lane; look: after_seed, back_fwd, fwd_n, stride_n (null: what dsb_scan_look_for gives the index), summ: a summary of table 0 (or null)
extern "C" int emu_scan_seeds(void *p, int strand, DsbSeed *out, int max_out, uint32_t *total, uint32_t *cnt, const uint8_t *look, const uint8_t *summ, int summ_shift)
{
	EmuCtx *e = (EmuCtx *)p; const DsbDevIndex &dx = e->dx; const WCtx &w = e->w;
	const uint32_t L = w.L, n = L >= 40 ? L - dx.ek_len + 1 : 0;
	ScanLane o;
	scan_lane(e->pk.data(), n, dx.ek_len, dx.single_base_max, dx.ek0, dx.ek1, dx.ek_mask, summ, summ_shift, strand == 0, look_of(look, (dx.ek_mask + 1) / 8), o);
	return scan_lane_out(o, out, max_out, total, cnt);
}
// the same on a caller's packed read (pk: 2 x ((L + 31) / 32 + 1) words, forward strand first) and a caller's filter tables
extern "C" int emu_stage_scan_read(const uint64_t *pk, uint32_t L, int k, int sbm, const uint8_t *ek0, const uint8_t *ek1, uint64_t ek_mask, const uint8_t *summ, int summ_shift,
                                   int strand, const uint8_t *look, DsbSeed *out, int max_out, uint32_t *total, uint32_t *cnt)
{
	if (L < 40 || k < 1 || k > 20 || !look) return -1;
	ScanLane o;
	scan_lane(pk, L - (uint32_t)k + 1, k, sbm, ek0, ek1, ek_mask, summ, summ_shift, strand == 0, look_of(look, 0), o);
	return scan_lane_out(o, out, max_out, total, cnt);
}
// the state machine alone on one hit byte per window of a strand (strand 1 forward, 0 reverse; the reverse strand is scanned through the
// mirrored index, as the kernel does)
extern "C" int emu_stage_scan_bytes(const uint8_t *hit, uint32_t n, int strand, const uint8_t *look, DsbSeed *out, int max_out, uint32_t *total, uint32_t *cnt)
{
	if (!look) return -1;
	const bool rc = strand == 0;
	ScanLane o; std::vector<DsbSeed> &sv = o.sv;
	auto store = [&](uint32_t idx, uint32_t off, uint32_t len) { if (sv.size() <= idx) sv.resize(idx + 1); sv[idx].offset = off; sv[idx].len = (uint16_t)len; sv[idx].top = 0; };
	auto mark = [&](uint32_t idx) { sv[idx].top = 1; };
	DsbScan s; dsb_scan_init(s, n, look_of(look, 0));
	while (s.mode != DSB_SCAN_DONE) {
		uint32_t want[DSB_SCAN_W]; dsb_scan_want(s, want); uint32_t bits = 0;
		for (int t = 0; t < DSB_SCAN_W; t++) {
			if (want[t] == DSB_SCAN_NONE) continue;
			if (want[t] >= n) return -2;
			o.cnt[1]++;
			if (hit[rc ? n - 1 - want[t] : want[t]]) bits |= 1u << t;
		}
		dsb_scan_consume(s, bits, rc, store, mark);
		o.cnt[3]++;
	}
	dsb_scan_finish(s, mark);
	o.ns = s.ns; o.total = s.total;
	return scan_lane_out(o, out, max_out, total, cnt);
}
// every window of one packed strand through dsb_probe_window, as k_seed_probe asks (P: (L + 31) / 32 + 1 words); went_t1: table-1 probes made
extern "C" void emu_stage_probe(const uint64_t *P, uint32_t n, int k, int sbm, const uint8_t *ek0, const uint8_t *ek1, uint64_t ek_mask, const uint8_t *summ, int summ_shift,
                                uint8_t *out, uint32_t *went_t1)
{
	const uint64_t kmask = k >= 32 ? ~0ULL : ((1ULL << (2 * k)) - 1ULL);
	uint32_t t1n = 0;
	for (uint32_t q = 0; q < n; q++) { int t1 = 0; out[q] = (uint8_t)dsb_probe_window(P, q, k, kmask, sbm, ek0, ek1, ek_mask, &t1, summ, summ_shift); t1n += (uint32_t)t1; }
	if (went_t1) *went_t1 = t1n;
}
#if DSB_EMU_LANES != 64
// seed_vector_scan on a caller's hit words (bit w & 63 of word w >> 6; the bits behind n are 0, as k_seed_probe leaves them, and one
// zero word follows, as seed_vector stages them); direction 1 forward, 0 reverse.  One lane runs it on the device as well.
extern "C" int emu_stage_vector_scan(const uint64_t *words, uint32_t n, int direction, DsbSeed *out, int max_out, uint32_t *total)
{
	std::vector<DsbSeed> sv((size_t)(n >> 1) + 64); uint32_t ns = 0, tot = 0;
	memset(sv.data(), 0, sv.size() * sizeof(DsbSeed));
	seed_vector_scan<const uint64_t *>(words, n, sv.data(), direction ? D_FORWARD : D_REVERSE, &ns, &tot);
	const int m = (int)ns < max_out ? (int)ns : max_out;
	for (int i = 0; i < m; i++) out[i] = sv[i];
	if (total) *total = tot;
	return (int)ns;
}
#endif
// loop budget of the following reads (DSB_STEP_LIMIT by default); steps the last read charged
// a-9 on its own: the device's register-packed lv_extd on two strings that arrive with 8 bytes in front of them (as its callers' local
// arrays hold them); the end marks go where the callers put them
extern "C" int32_t emu_lv_extd(const uint8_t *ref_padded, int32_t ref_length, const uint8_t *query_padded, int32_t query_length)
{
	uint8_t r[8 + 32], q[8 + 32];
	if (ref_length < 0 || ref_length > 12 || query_length != ref_length) return -1;
	memcpy(r, ref_padded, (size_t)(8 + ref_length)); memcpy(q, query_padded, (size_t)(8 + query_length));
	r[8 + ref_length] = '#'; q[8 + query_length] = '$';
	return lv_extd(r + 8, ref_length, q + 8, query_length);
}
// a-11 on its own: the device's sc_hash_idx / combine_test / combine_chain on chains given as rows of 9 u32 (layout: oracle/oracle.h
// ora_combine_stage); test_out[i] = what combine_test said right before combine_chain was asked
extern "C" void emu_combine_stage(uint32_t *chains, uint32_t n, const int32_t *queries, uint32_t n_q, int32_t *out, int32_t *test_out)
{
	std::vector<DsbChain> H(n + 1); std::vector<DsbScHash> sc(256 + 2 * (size_t)n + 8);
	memset(H.data(), 0, H.size() * sizeof(DsbChain)); memset(sc.data(), 0, sc.size() * sizeof(DsbScHash));
	for (uint32_t i = 0; i < n; i++) {
		const uint32_t *r = chains + 9 * i;
		H[i].ref_ID = r[0]; H[i].direction = (uint8_t)r[1]; H[i].sum_score = r[2]; H[i].anchor_number = r[3]; H[i].indel = r[4];
		H[i].t_st = r[5]; H[i].t_ed = r[6]; H[i].q_st = r[7]; H[i].q_ed = r[8];
	}
	sc_hash_idx(sc.data(), H.data(), n);
	for (uint32_t i = 0; i < n_q; i++) {
		DsbChain *combined = nullptr;
		const int32_t *q = queries + 4 * i;
		test_out[i] = combine_test(H.data(), q[0], sc.data(), q[1], q[2] != 0, q[3]) ? 1 : 0;
		out[i] = combine_chain(H.data(), q[0], sc.data(), q[1], q[2] != 0, q[3], &combined) ? (int32_t)(combined - H.data()) : -1;
	}
	for (uint32_t i = 0; i < n; i++) {
		uint32_t *r = chains + 9 * i;
		r[0] = H[i].ref_ID; r[1] = H[i].direction; r[2] = H[i].sum_score; r[3] = H[i].anchor_number; r[4] = H[i].indel;
		r[5] = H[i].t_st; r[6] = H[i].t_ed; r[7] = H[i].q_st; r[8] = H[i].q_ed;
	}
}
extern "C" void emu_set_step_limit(void *p, uint32_t v) { ((EmuCtx *)p)->w.step_limit = v; ((EmuCtx *)p)->limit_set = v; }
extern "C" void emu_steps(void *p, uint32_t out[2]) { out[0] = ((EmuCtx *)p)->w.steps; out[1] = ((EmuCtx *)p)->w.lsteps; }
// work counters of the last read: occ, MEM searches, SA lookups, reference bases fetched
extern "C" void emu_counters(void *p, uint32_t out[4]) { memcpy(out, ((EmuCtx *)p)->cnt, 16); }
// cly_r.anchor_v.n when classify_seq returned (printed by the DES writers)
extern "C" uint32_t emu_n_anc(void *p) { return ((EmuCtx *)p)->w.n_anc; }

// ---- stage a-12 form by form (tests/stage/dsb_stage_forms.h, tests/test_stage_sdp.py): sdp_match as wtab_build + sdp_match_t,
// wtab_build_pk + sdp_match_t, sdp_match_inv, the dispatcher, sdp_match_lds; gap_lane; sdp_middle_M2.  The context is the one
// classify_kernel_body sets up, on host memory; no index directory is involved.
#include "../stage/dsb_stage_forms.h"
struct StageHost {
	alignas(16) uint32_t wtab[DSB_WTAB_SLOTS]; uint4 ring[DSB_RING]; uint32_t red[4], cnt[4]; DsbDevIndex sx; WCtx w; DsbRefInfo ri; DpBatch dpb;
	std::vector<uint8_t> slice;
};
static StageHost *stage_host()
{
	static StageHost *h = nullptr;
	if (!h) { h = new StageHost(); h->slice.assign(STAGE_SLICE, 0xCD); }
	memset(&h->sx, 0, sizeof h->sx); memset(&h->w, 0, sizeof h->w); memset(h->cnt, 0, sizeof h->cnt);
	h->ri.seq_l = ~0ULL; h->ri.seq_offset = 0; h->w.dpb = &h->dpb;
	return h;
}
struct StageJob {
	StageHost *h; int what, form; StageSdp *sc; StageChain *cc; StageDp *dc; const uint32_t *sizes; StageExt *ec; DsbChain *chains; const int32_t *rows5; DsbScHash *scs; const DsbRefInfo *ris; const uint8_t *bin; const uint64_t *pk; const uint8_t *aux; DsbSms *nodes; uint4 *mirror; DsbGap *G; const int32_t *anchors;
};
static void stage_lane(void *p)
{
	StageJob *j = (StageJob *)p; StageHost *h = j->h;
	stage_ctx(h->w, &h->sx, h->slice.data(), h->wtab, h->ring, h->red, h->cnt, &h->ri);
	if (j->what == 0) stage_sdp(h->w, &h->sx, j->form, j->sc, j->bin, j->pk, j->aux, j->nodes, j->mirror);
	else if (j->what == 1) stage_gap_lane(h->w, &h->sx, j->cc, j->bin, j->pk, j->aux, j->G);
	else if (j->what == 2) stage_middle(h->w, &h->sx, j->cc, j->bin, j->pk, j->aux, j->anchors);
	else if (j->what == 3) stage_dp(h->w, &h->sx, j->dc, j->nodes, j->sizes);
	else stage_ext(h->w, &h->sx, j->ec, j->bin, j->pk, j->aux, j->chains, j->rows5, j->nodes, j->scs, j->ris);
}
static void stage_run(StageJob &j)
{
#if DSB_EMU_LANES == 64
	dsb_emu_run(stage_lane, &j);
#else
	stage_lane(&j);
#endif
}
static void stage_regions(StageJob &j, const void *cases, size_t case_bytes, size_t bin_bytes, size_t pk_words, size_t aux_bytes)
{
#if DSB_EMU_LANES == 64
	StageHost *h = j.h;
	dsb_emu_regions_clear();
	dsb_emu_region(&j, sizeof j, "job"); dsb_emu_region(&h->slice, sizeof h->slice, "slice handle"); dsb_emu_region(h->wtab, sizeof h->wtab, "LDS window table"); dsb_emu_region(h->ring, sizeof h->ring, "LDS ring");
	dsb_emu_region(h->red, sizeof h->red, "LDS red"); dsb_emu_region(h->cnt, sizeof h->cnt, "LDS counters"); dsb_emu_region(&h->sx, sizeof h->sx, "index descriptor");
	dsb_emu_region(&h->w, sizeof h->w, "context"); dsb_emu_region(&h->ri, sizeof h->ri, "reference info"); dsb_emu_region(&h->dpb, sizeof h->dpb, "LDS DP batch");
	dsb_emu_region(h->slice.data() + STAGE_OFF_SORTKEY, 16384, "sort keys"); dsb_emu_region(h->slice.data() + STAGE_OFF_SORTIDX, 4096, "sort indices");
	dsb_emu_region(h->slice.data() + STAGE_OFF_ANC, 16384, "anchors"); dsb_emu_region(h->slice.data() + STAGE_OFF_ANC_TMP, 16384, "anchors (copy)");
	dsb_emu_region(h->slice.data() + STAGE_OFF_WIN, 6656, "reference windows"); dsb_emu_region(h->slice.data() + STAGE_OFF_SMS, STAGE_CHAIN_SMS * 16, "match nodes");
	dsb_emu_region(cases, case_bytes, "cases"); dsb_emu_region(j.bin, bin_bytes, "byte strands"); dsb_emu_region(j.pk, 8 * pk_words, "packed strands");
	dsb_emu_region(j.aux, aux_bytes, j.what == 0 ? "window bytes" : "reference text");
#else
	(void)j; (void)cases; (void)case_bytes; (void)bin_bytes; (void)pk_words; (void)aux_bytes;
#endif
}
extern "C" uint32_t emu_stage_sizes(uint32_t *out)
{
	out[0] = sizeof(StageSdp); out[1] = sizeof(StageChain); out[2] = sizeof(DsbGap); out[3] = DSB_WTAB_SLOTS; out[4] = DSB_WTAB_MAXQ; out[5] = DSB_INV_PAIRS; out[6] = DSB_INV_MINQ; out[7] = DSB_INV_MAXPOS;
	out[8] = DSB_SDP_CAND; out[9] = DSB_SDP_KEEP; out[10] = DSB_GL_QW; out[11] = DSB_GL_NODES; out[12] = DSB_GL_MAXT; out[13] = DSB_INV_WORDS; out[14] = DSB_EMU_LANES; out[15] = STAGE_MAX_ANC;
	return 16;
}
extern "C" int emu_stage_sdp(int form, StageSdp *cases, uint32_t n, const uint8_t *bin, size_t bin_bytes, const uint64_t *pk, size_t pk_words, const uint8_t *win, size_t win_bytes,
                             DsbSms *nodes, size_t node_entries, uint4 *mirror)
{
	StageJob j; memset(&j, 0, sizeof j); j.h = stage_host(); j.what = 0; j.form = form; j.bin = bin; j.pk = pk; j.aux = win; j.nodes = nodes;
	stage_regions(j, cases, (size_t)n * sizeof(StageSdp), bin_bytes, pk_words, win_bytes);
#if DSB_EMU_LANES == 64
	dsb_emu_region(nodes, node_entries * sizeof(DsbSms), "node lists"); dsb_emu_region(mirror, (size_t)n * 64 * sizeof(uint4), "node mirrors");
#else
	(void)node_entries;
#endif
	for (uint32_t k = 0; k < n; k++) { j.sc = cases + k; j.mirror = mirror + 64 * (size_t)k; stage_run(j); }
	return 0;
}
extern "C" int emu_stage_gap_lane(StageChain *cases, uint32_t n, const uint8_t *bin, size_t bin_bytes, const uint64_t *pk, size_t pk_words, const uint8_t *ref, size_t ref_bytes, DsbGap *G, size_t n_gaps)
{
	StageJob j; memset(&j, 0, sizeof j); j.h = stage_host(); j.what = 1; j.bin = bin; j.pk = pk; j.aux = ref; j.G = G;
	stage_regions(j, cases, (size_t)n * sizeof(StageChain), bin_bytes, pk_words, ref_bytes);
#if DSB_EMU_LANES == 64
	dsb_emu_region(G, n_gaps * sizeof(DsbGap), "gaps");
#else
	(void)n_gaps;
#endif
	for (uint32_t k = 0; k < n; k++) { j.cc = cases + k; stage_run(j); }
	return 0;
}
extern "C" int emu_stage_middle(StageChain *cases, uint32_t n, const uint8_t *bin, size_t bin_bytes, const uint64_t *pk, size_t pk_words, const uint8_t *ref, size_t ref_bytes, const int32_t *anchors, size_t n_rows)
{
	StageJob j; memset(&j, 0, sizeof j); j.h = stage_host(); j.what = 2; j.bin = bin; j.pk = pk; j.aux = ref; j.anchors = anchors;
	stage_regions(j, cases, (size_t)n * sizeof(StageChain), bin_bytes, pk_words, ref_bytes);
#if DSB_EMU_LANES == 64
	dsb_emu_region(anchors, n_rows * 16, "anchor rows");
#else
	(void)n_rows;
#endif
	for (uint32_t k = 0; k < n; k++) { j.cc = cases + k; stage_run(j); }
	return 0;
}

// the sparse DP on bare node lists (tests/test_stage_dp.py): forms (a) .. (c); form (d), sdp_batch_old_mw on several wavefronts, runs on the device only
extern "C" int emu_stage_dp(StageDp *cases, uint32_t n, DsbSms *nodes, size_t node_entries, const uint32_t *sizes, size_t n_sizes)
{
	if (stage_dp_check(cases, n, node_entries, n_sizes)) return __LINE__;
	for (uint32_t k = 0; k < n; k++) if (cases[k].form == DP_MW) return __LINE__;
	StageJob j; memset(&j, 0, sizeof j); j.h = stage_host(); j.what = 3; j.nodes = nodes; j.sizes = sizes;
	stage_regions(j, cases, (size_t)n * sizeof(StageDp), 0, 0, 0);
#if DSB_EMU_LANES == 64
	dsb_emu_region(nodes, node_entries * sizeof(DsbSms), "node lists"); dsb_emu_region(sizes, n_sizes * 4, "block sizes");
#endif
	for (uint32_t k = 0; k < n; k++) { j.dc = cases + k; stage_run(j); }
	return 0;
}
extern "C" uint32_t emu_stage_sizes_dp(uint32_t *out)
{
	out[0] = sizeof(StageDp); out[1] = STAGE_DP_GUARD; out[2] = DSB_RING; out[3] = DSB_DPB; out[4] = DSB_DP_UNROLL; out[5] = DSB_EMU_LANES; out[6] = DSB_MW_MAXW; out[7] = DSB_ST_HEAVY;
	return 8;
}

// one sdp_right_M2 / sdp_left_M2 per case, block-wise or node by node (tests/test_stage_ext.py)
extern "C" int emu_stage_ext(StageExt *cases, uint32_t n, const uint8_t *bin, size_t bin_bytes, const uint64_t *pk, size_t pk_words, const uint8_t *ref, size_t ref_bytes,
                             DsbChain *chains, size_t n_chains, const int32_t *anchors, size_t n_rows, DsbSms *nodes, size_t node_entries, DsbScHash *scs, size_t n_sc,
                             const DsbRefInfo *ris, size_t n_ri)
{
	if (stage_ext_check(cases, n, n_chains, n_rows, anchors, chains, node_entries, n_sc, n_ri)) return __LINE__;
	StageJob j; memset(&j, 0, sizeof j); j.h = stage_host(); j.what = 4; j.bin = bin; j.pk = pk; j.aux = ref; j.chains = chains; j.rows5 = anchors; j.nodes = nodes; j.scs = scs; j.ris = ris;
	stage_regions(j, cases, (size_t)n * sizeof(StageExt), bin_bytes, pk_words, ref_bytes);
#if DSB_EMU_LANES == 64
	dsb_emu_region(chains, n_chains * sizeof(DsbChain), "chains"); dsb_emu_region(anchors, n_rows * 20, "anchor rows"); dsb_emu_region(nodes, node_entries * sizeof(DsbSms), "node lists");
	dsb_emu_region(scs, n_sc * sizeof(DsbScHash), "chain hash"); dsb_emu_region(ris, n_ri * sizeof(DsbRefInfo), "reference info");
#endif
	for (uint32_t k = 0; k < n; k++) { j.ec = cases + k; stage_run(j); }
	return 0;
}
extern "C" uint32_t emu_stage_sizes_ext(uint32_t *out) { out[0] = sizeof(StageExt); out[1] = sizeof(DsbChain); out[2] = sizeof(DsbScHash); out[3] = sizeof(DsbRefInfo); return 4; }

// ---- the chain stages form by form (tests/stage/dsb_stage_forms.h, tests/test_stage_chain.py, tests/test_stage_finish.py): resolve_tree with the
// sort, the DP and the selection forced; the cut and the tail of delete_small_score_rst, detect_primary; glibc_sort_chains
struct Stage2Job { StageHost *h; uint8_t *slice; StageRes *rc; StageFin *fc; const uint32_t *rows; uint32_t *order; int32_t *pre; DsbChain *hits, *raw; };
static void stage2_lane(void *p)
{
	Stage2Job *j = (Stage2Job *)p; StageHost *h = j->h;
	stage_ctx(h->w, &h->sx, j->slice, h->wtab, h->ring, h->red, h->cnt, &h->ri);
	if (j->rc) stage_resolve(h->w, j->rc, j->rows, j->order, j->pre, j->hits, j->raw, j->slice);
	else stage_finish(h->w, &h->sx, j->fc, j->hits, j->raw, j->slice);
}
static std::vector<uint8_t> g_stage2_slice;      // (at file scope: a function's static would bring a guard variable and, in the 64-lane build, an atomic hook)
static std::vector<uint8_t> &stage2_slice()
{
	if (g_stage2_slice.empty()) g_stage2_slice.assign(STAGE2_SLICE, 0xCD);
	return g_stage2_slice;
}
static void stage2_run(Stage2Job &j)
{
#if DSB_EMU_LANES == 64
	dsb_emu_run(stage2_lane, &j);
#else
	stage2_lane(&j);
#endif
}
static void stage2_regions(Stage2Job &j, const void *cases, size_t case_bytes)
{
#if DSB_EMU_LANES == 64
	StageHost *h = j.h; uint8_t *s = j.slice;
	dsb_emu_regions_clear();
	dsb_emu_region(&j, sizeof j, "job"); dsb_emu_region(h->wtab, sizeof h->wtab, "LDS window table"); dsb_emu_region(h->ring, sizeof h->ring, "LDS ring");
	dsb_emu_region(h->red, sizeof h->red, "LDS red"); dsb_emu_region(h->cnt, sizeof h->cnt, "LDS counters"); dsb_emu_region(&h->sx, sizeof h->sx, "index descriptor");
	dsb_emu_region(&h->w, sizeof h->w, "context"); dsb_emu_region(&h->ri, sizeof h->ri, "reference info"); dsb_emu_region(&h->dpb, sizeof h->dpb, "LDS DP batch");
	dsb_emu_region(s + STAGE2_OFF_ANC, STAGE2_MAX_ANC * 40u, "anchors"); dsb_emu_region(s + STAGE2_OFF_ANC_TMP, STAGE2_MAX_ANC * 40u, "anchors (copy)");
	dsb_emu_region(s + STAGE2_OFF_SORTKEY, 2u * STAGE2_MAX_ANC * 8u, "sort keys"); dsb_emu_region(s + STAGE2_OFF_SORTIDX, 2u * STAGE2_MAX_ANC * 4u, "sort indices");
	dsb_emu_region(s + STAGE2_OFF_SCOREV, 4096, "score_v"); dsb_emu_region(s + STAGE2_OFF_WIN, 4096, "reference window"); dsb_emu_region(s + STAGE2_OFF_HIT_TMP, STAGE2_MAX_HIT * 48u, "chains (copy)");
	dsb_emu_region(cases, case_bytes, "cases");
#else
	(void)j; (void)cases; (void)case_bytes;
#endif
}
extern "C" uint32_t emu_stage_sizes2(uint32_t *out)
{
	out[0] = sizeof(StageRes); out[1] = sizeof(StageFin); out[2] = sizeof(DsbChain); out[3] = DSB_WTAB_SLOTS; out[4] = DSB_RANKSORT_MAX; out[5] = DSB_CHAINDP_LDS; out[6] = STAGE2_MAX_ANC; out[7] = STAGE2_MAX_HIT;
	out[8] = STAGE2_GUARD; out[9] = DSB_EMU_LANES;
	return 10;
}
extern "C" int emu_stage_resolve(StageRes *cases, uint32_t n, const uint32_t *rows, size_t n_rows, uint32_t *order, int32_t *pre, DsbChain *hits, size_t n_hits, DsbChain *raw, size_t n_raw)
{
	if (stage_resolve_check(cases, n, rows, n_rows, n_hits, n_raw)) return __LINE__;
	Stage2Job j; memset(&j, 0, sizeof j); j.h = stage_host(); j.slice = stage2_slice().data(); j.rows = rows; j.order = order; j.pre = pre; j.hits = hits; j.raw = raw;
	stage2_regions(j, cases, (size_t)n * sizeof(StageRes));
#if DSB_EMU_LANES == 64
	dsb_emu_region(rows, n_rows * 32, "anchor rows"); dsb_emu_region(order, n_rows * 4, "anchor order"); dsb_emu_region(pre, n_rows * 4, "anchor links");
	dsb_emu_region(hits, n_hits * sizeof(DsbChain), "chains"); dsb_emu_region(raw, n_raw * sizeof(DsbChain), "chains before the selection");
#endif
	for (uint32_t k = 0; k < n; k++) { j.rc = cases + k; stage2_run(j); }
	return 0;
}
extern "C" int emu_stage_finish(StageFin *cases, uint32_t n, DsbChain *chains, DsbChain *tail, size_t n_chains)
{
	if (stage_finish_check(cases, n, n_chains)) return __LINE__;
	Stage2Job j; memset(&j, 0, sizeof j); j.h = stage_host(); j.slice = stage2_slice().data(); j.hits = chains; j.raw = tail;
	stage2_regions(j, cases, (size_t)n * sizeof(StageFin));
#if DSB_EMU_LANES == 64
	dsb_emu_region(chains, n_chains * sizeof(DsbChain), "chains"); dsb_emu_region(tail, n_chains * sizeof(DsbChain), "chains behind the tail");
#endif
	for (uint32_t k = 0; k < n; k++) { j.fc = cases + k; stage2_run(j); }
	return 0;
}

// ---- the anchor stage form by form (tests/stage/dsb_stage_forms.h, tests/test_stage_anchor.py): the FM search, fast_island, fast_classify, fast_classify_lane and
// slow_classify on a loaded index; the descriptor is the one emu_new builds, on the host view of the index
struct Stage3Index { dsb_index *idx; DsbDevIndex dx; };
extern "C" void *emu_stage_anchor_index(dsb_index *idx)
{
	const DsbHostIndex *h = dsb_index_host(idx);
	Stage3Index *s = new Stage3Index(); s->idx = idx;
	DsbDevIndex &dx = s->dx; memset(&dx, 0, sizeof dx);
	dx.ek0 = h->ek0; dx.ek1 = h->ek1; dx.ek_mask = h->ek_mask; dx.ek_len = h->ek_len; dx.single_base_max = h->single_base_max;
	dx.fm = h->fm; dx.fm_sb = h->fm_sb; dx.bwt_len = h->bwt_len; memcpy(dx.rank, h->rank, sizeof dx.rank); dx.dollar_pos = h->dollar_pos; dx.dollar_row = h->dollar_row;
	dx.hash_index = h->hash_c ? nullptr : h->hash_index; dx.hash_c = h->hash_c; dx.sa = (const uint2 *)h->sa; dx.uni = (const uint2 *)h->uni; dx.refpos = h->refpos; dx.refbin = h->refbin; dx.ref_bases = h->n_refbin * 4;
	dx.refinfo = h->refinfo; dx.qmem = h->Q_MEM; dx.qlv = &h->Q_LV[0][0];
	return s;
}
extern "C" void emu_stage_anchor_index_free(void *p) { delete (Stage3Index *)p; }
// what the index was opened as: [0] the 13-mer table is the compressed one, [1] the rank lines have superblocks, [2] the filter's k-mer length
extern "C" void emu_stage_anchor_index_info(void *p, uint32_t *out) { const DsbDevIndex &dx = ((Stage3Index *)p)->dx; out[0] = dx.hash_c != nullptr; out[1] = dx.fm_sb != nullptr; out[2] = (uint32_t)dx.ek_len; }
struct Stage3Job { StageHost *h; uint8_t *slice; const DsbDevIndex *dx; StageAnc *c, *cases; uint32_t k0, n; const uint8_t *bin; DsbSeed *seeds; DsbAnchor *anchors; const int32_t *calls; int64_t *mems; };
static void stage3_lane(void *p)
{
	Stage3Job *j = (Stage3Job *)p; StageHost *h = j->h;
	stage_ctx(h->w, &h->sx, j->slice, h->wtab, h->ring, h->red, h->cnt, &h->ri);
	if (j->c) stage_anchor(h->w, &h->sx, j->dx, j->c, j->bin, j->seeds, j->anchors, j->calls, j->mems, j->slice);
	else stage_anchor_lane(h->w, &h->sx, j->dx, j->cases, j->k0, j->n, j->bin, j->seeds, j->anchors, j->slice);
}
static std::vector<uint8_t> g_stage3_slice;
extern "C" uint32_t emu_stage_sizes3(uint32_t *out)
{
	out[0] = sizeof(StageAnc); out[1] = sizeof(DsbAnchor); out[2] = sizeof(DsbSeed); out[3] = DSB_LANE_ANC_CAP; out[4] = DSB_LANE_STEPS; out[5] = STAGE3_GUARD; out[6] = STAGE3_MEM; out[7] = DSB_EMU_LANES;
	out[8] = DSB_SPSET_CAP; out[9] = STAGE3_MAX_SEEDS;
	return 10;
}
extern "C" int emu_stage_anchor(void *index, StageAnc *cases, uint32_t n, const uint8_t *bin, size_t bin_bytes, DsbSeed *seeds, size_t n_seeds, DsbAnchor *anchors, size_t n_anchors,
                                const int32_t *calls, size_t n_calls, int64_t *mems, size_t n_mems)
{
	Stage3Index *si = (Stage3Index *)index;
	if (stage_anchor_check(cases, n, bin_bytes, n_seeds, n_anchors, calls, n_calls, n_mems, seeds, si->dx.ek_len)) return __LINE__;
	if (!n) return 0;
	for (uint32_t k = 0; k < n; k++) if ((cases[k].form == ANC_LANE) != (cases[0].form == ANC_LANE)) return __LINE__;
	if (g_stage3_slice.empty()) g_stage3_slice.assign(STAGE3_SLICE, 0);
	Stage3Job j; memset(&j, 0, sizeof j); j.h = stage_host(); j.slice = g_stage3_slice.data(); j.dx = &si->dx; j.cases = cases; j.n = n; j.bin = bin; j.seeds = seeds; j.anchors = anchors; j.calls = calls; j.mems = mems;
#if DSB_EMU_LANES == 64
	{
		StageHost *h = j.h; uint8_t *s = j.slice; const DsbHostIndex *x = dsb_index_host(si->idx);
		dsb_emu_regions_clear();
		// (the detector looks an address up in this list front to back: what the walks read most comes first)
		dsb_emu_region(x->fm, x->n_fm * sizeof(DsbFmBlock), "rank lines");
		if (x->fm_sb) dsb_emu_region(x->fm_sb, x->n_fm_sb * 40, "rank superblocks");
		if (x->hash_c) dsb_emu_region(x->hash_c, (size_t)x->n_hash_c * sizeof(DsbHiLine), "13-mer table (compressed)"); else dsb_emu_region(x->hash_index, (((size_t)1 << 26) + 1) * 8, "13-mer table");
		dsb_emu_region(x->sa, x->sa_size * 8, "SA samples"); dsb_emu_region(x->uni, (x->n_uni + 1) * 8, "unitigs"); dsb_emu_region(x->refpos, (x->n_refpos + 1) * 8, "reference positions");
		dsb_emu_region(x->refbin, x->n_refbin + 4096, "reference text"); dsb_emu_region(x->refinfo, x->n_ref * sizeof(DsbRefInfo), "reference info (index)");
		dsb_emu_region(x->Q_MEM, 2000 * sizeof(int), "Q_MEM"); dsb_emu_region(&x->Q_LV[0][0], 400 * sizeof(int), "Q_LV");
		dsb_emu_region(&j, sizeof j, "job"); dsb_emu_region(h->wtab, sizeof h->wtab, "LDS window table"); dsb_emu_region(h->ring, sizeof h->ring, "LDS ring");
		dsb_emu_region(h->red, sizeof h->red, "LDS red"); dsb_emu_region(h->cnt, sizeof h->cnt, "LDS counters"); dsb_emu_region(&h->sx, sizeof h->sx, "index descriptor");
		dsb_emu_region(&h->w, sizeof h->w, "context"); dsb_emu_region(&h->ri, sizeof h->ri, "reference info"); dsb_emu_region(&h->dpb, sizeof h->dpb, "LDS DP batch");
		dsb_emu_region(&si->dx, sizeof si->dx, "index descriptor (source)");
		dsb_emu_region(s + STAGE3_OFF_SPSET, DSB_SPHASH * 8u, "visited rows"); dsb_emu_region(s + STAGE3_OFF_LANE_SP, 64u * DSB_SPHASH * 8u, "lane visited rows");
		dsb_emu_region(s + STAGE3_OFF_LANE_ANC, 64u * DSB_LANE_ANC_CAP * 40u, "lane anchors"); dsb_emu_region(s + STAGE3_OFF_TOP, STAGE3_MAX_SEEDS * 4u, "top islands");
		dsb_emu_region(s + STAGE3_OFF_ROUND, STAGE3_MAX_SEEDS * 4u, "island records"); dsb_emu_region(s + STAGE3_OFF_ORD, STAGE3_MAX_SEEDS * 4u, "island order");
		dsb_emu_region(s + STAGE3_OFF_MEM, DSB_MEMSLOW_CAP * 32u, "slow-path MEMs");
		dsb_emu_region(cases, (size_t)n * sizeof(StageAnc), "cases"); dsb_emu_region(bin, bin_bytes, "byte strands"); dsb_emu_region(seeds, n_seeds * sizeof(DsbSeed), "seeds");
		dsb_emu_region(anchors, n_anchors * sizeof(DsbAnchor), "anchors"); dsb_emu_region(calls, n_calls * 16, "search calls"); dsb_emu_region(mems, n_mems * STAGE3_MEM * 8, "search results");
	}
#endif
	auto run = [&]() {
#if DSB_EMU_LANES == 64
		dsb_emu_run(stage3_lane, &j);
#else
		stage3_lane(&j);
#endif
	};
	if (cases[0].form == ANC_LANE) for (uint32_t k = 0; k < n; k += DSB_WAVE) { j.c = nullptr; j.k0 = k; run(); }
	else for (uint32_t k = 0; k < n; k++) { j.c = cases + k; run(); }
	return 0;
}
