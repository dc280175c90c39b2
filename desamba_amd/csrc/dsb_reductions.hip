// The run reductions of classify (dsb_reductions.h): per-read taxa, per-reference coverage with its per-window profile and per-reference
// abundance by EM with each read's assignment by its posterior, per-read LCA classification -- their kernels, the launches after a batch's last classify launch (reductions_run), the
// host side of each, and their merges over the contexts of a dsb_multi.
#include <algorithm>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include "dsb_ctx.h"
#include "dsb_sam_fields.h"
#include "dsb_taxonomy.h"

// One lane per read, after the batch's last classify work: the taxon of the read's own records as `deSAMBA analysis`
// reads them back from the SAM (dsb_taxonomy.cpp, ana_get_tid src/analysis.c:1271-1330).  The records are the ones
// dsb_format_sam prints -- the primary, the supplementary ones, the secondary ones up to max_sec -- taken where the classify
// kernels left them (DsbReadOut / DsbHitOut); MAPQ and the CIGAR's length come from dsb_sam_fields.h, as the writer's do.
// Each parent walk stops after `bound` steps (the deepest chain of the taxonomy + 2: the loader rejects cycles); a read the
// host must walk itself is flagged DSB_TAXON_HOST: a first record with score 0 or a taxid above max_tid (the read ends
// there and its other records become reads of their own), a reference whose name does not come back from the SAM as it
// is, or a walk that ran out of steps.
__global__ void __launch_bounds__(256) k_read_taxon(const DsbReadOut *__restrict__ rout, const DsbHitOut *__restrict__ hout, const DsbCounters *__restrict__ counters,
                                                    uint32_t cap_hout, const DsbReadDesc *__restrict__ rd, uint32_t n, const uint32_t *__restrict__ parent,
                                                    const uint32_t *__restrict__ ref_tid, uint32_t n_ref, uint32_t max_tid, uint32_t bound, int max_sec, dsb_read_taxon *__restrict__ out)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const uint32_t nh = dsb_hits_out(counters->hits, cap_hout);
	const DsbReadOut r = rout[i];
	dsb_read_taxon t; t.taxid = 0; t.score = 0; t.len = 0; t.mapq = 0; t.flags = 0; t.pad = 0;
	const uint32_t nrec = dsb_hits_cut(r.first, r.n, nh) ? 0u : r.n;
	if (nrec) {
		const dsb_hit *h = reinterpret_cast<const dsb_hit *>(hout + r.first);
		const uint32_t read_l = rd[i].len;
		const uint32_t t0 = h[0].ref_ID < n_ref ? ref_tid[h[0].ref_ID] : DSB_TID_NONE;
		t.flags = DSB_TAXON_CLASSIFIED;
		t.score = h[0].sum_score; t.len = dsb_sam_cigar_len(h, read_l, false); t.mapq = (uint8_t)dsb_sam_mapq_pri(h, nrec);
		if (t0 == DSB_TID_NONE || t0 > max_tid || t.score == 0) { t.flags |= DSB_TAXON_HOST; t.taxid = t0 <= max_tid ? t0 : 0; }
		else {
			uint32_t tid = t0;
			for (int pass = 0; pass <= 1 && !(t.flags & DSB_TAXON_HOST); pass++)
				for (uint32_t k = 1; k < nrec; k++) {
					const dsb_hit *c = h + k;
					if (!dsb_sam_shown(c, pass, max_sec)) continue;
					const uint32_t rt = c->ref_ID < n_ref ? ref_tid[c->ref_ID] : DSB_TID_NONE;
					if (rt == DSB_TID_NONE) { t.flags |= DSB_TAXON_HOST; break; }
					if (c->sum_score != t.score || rt > max_tid) continue;
					uint32_t p = rt, steps = 0;
					for (; steps < bound; steps++) {                                // is rt at or below the taxon held?
						if (p == tid) { tid = rt; break; }
						if (p < 1 || p == DSB_TID_NONE || p > max_tid) break;
						p = parent[p];
					}
					if (steps == bound) { t.flags |= DSB_TAXON_HOST; break; }
				}
			t.taxid = tid;
		}
	}
	out[i] = t;
}

// Per-reference coverage (dsb_ctx_enable_coverage).  One wavefront per read, after the batch's last classify work: each
// record printed without FLAG 0x100 (dsb_sam_counted) adds to its reference's counters (lane 0) and sets the bits of its interval
// [min(t_st, LN), min(t_ed, LN)), the lanes striding over its words.  The bits are set by agent-scope atomic ORs, never by plain
// stores: two records may share a word, and their workgroups may sit on XCDs whose L2s are not coherent with each other.  A
// reference's bits start at word word_off[ref]; bits at LN and beyond are never set.
__global__ void __launch_bounds__(256) k_ref_cover(const DsbReadOut *__restrict__ rout, const DsbHitOut *__restrict__ hout, const DsbCounters *__restrict__ counters,
                                                   uint32_t cap_hout, uint32_t n, const uint64_t *__restrict__ ref_len, const uint64_t *__restrict__ word_off,
                                                   uint32_t n_ref, uint64_t *bits, dsb_ref_coverage *cov)
{
	const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (i >= n) return;
	const uint32_t nh = dsb_hits_out(counters->hits, cap_hout);
	const DsbReadOut r = rout[i];
	const uint32_t nrec = dsb_hits_cut(r.first, r.n, nh) ? 0u : r.n;
	if (!nrec) return;
	const dsb_hit *h = reinterpret_cast<const dsb_hit *>(hout + r.first);
	const int mq_pri = dsb_sam_mapq_pri(h, nrec);
	for (uint32_t k = 0; k < nrec; k++) {
		const dsb_hit *c = h + k;
		if (!dsb_sam_counted(c, k) || c->ref_ID >= n_ref) continue;
		const uint64_t ln = ref_len[c->ref_ID];
		const uint64_t s = c->t_st < ln ? c->t_st : ln, e = c->t_ed < ln ? c->t_ed : ln;
		if (lane == 0) {
			dsb_ref_coverage *o = cov + c->ref_ID;
			__hip_atomic_fetch_add(&o->numreads, (uint64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			if (e > s) __hip_atomic_fetch_add(&o->aligned_bases, e - s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			const int mq = k ? dsb_sam_mapq_sup(mq_pri) : mq_pri;
			if (mq) __hip_atomic_fetch_add(&o->mapq_sum, (uint64_t)mq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
		if (e <= s) continue;
		uint64_t *w = bits + word_off[c->ref_ID];
		for (uint64_t q = (s >> 6) + lane; q <= ((e - 1) >> 6); q += 64) {
			const uint64_t lo = q * 64 < s ? s - q * 64 : 0, hi = q * 64 + 64 > e ? e - q * 64 : 64;   // bits [lo, hi) of word q
			const uint64_t m = (hi == 64 ? ~0ull : (1ull << hi) - 1) & (~0ull << lo);
			__hip_atomic_fetch_or(w + q, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
	}
}

// End of a run: covbases, a segmented popcount over words [w0, w0 + nw) of the bitmap (bits[q - w0] holds word q), balanced by words
// rather than by reference.  Each wavefront takes DSB_COVER_CHUNK words, finds the reference of its first word by binary search in
// the word offsets (empty references skipped: the last r with word_off[r] <= a) and adds one partial sum per reference it spans.
#define DSB_COVER_CHUNK 1024
__global__ void __launch_bounds__(256) k_cover_count(const uint64_t *__restrict__ bits, uint64_t w0, uint64_t nw, const uint64_t *__restrict__ word_off,
                                                     uint32_t n_ref, dsb_ref_coverage *cov)
{
	const uint64_t a = w0 + ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * DSB_COVER_CHUNK, end = w0 + nw;
	const uint32_t lane = threadIdx.x & 63;
	if (a >= end) return;
	const uint64_t b = a + DSB_COVER_CHUNK < end ? a + DSB_COVER_CHUNK : end;
	uint32_t lo = 0, hi = n_ref;                           // word_off[lo] <= a < word_off[hi] (= the bitmap's size for hi = n_ref)
	while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (word_off[mid] <= a) lo = mid; else hi = mid; }
	for (uint32_t r = lo;; r++) {
		const uint64_t s = word_off[r] > a ? word_off[r] : a, e = word_off[r + 1] < b ? word_off[r + 1] : b;
		uint32_t sum = 0;                                  // (at most 64 bits x DSB_COVER_CHUNK words)
		for (uint64_t q = s + lane; q < e; q += 64) sum += (uint32_t)__popcll(bits[q - w0]);
		for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o, 64);
		if (lane == 0 && sum) __hip_atomic_fetch_add(&cov[r].covbases, (uint64_t)sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (e >= b) break;
	}
}

// before a count: covbases = 0 (the other three counters stay)
__global__ void __launch_bounds__(256) k_cover_clear(dsb_ref_coverage *cov, uint32_t n_ref)
{
	const uint32_t r = blockIdx.x * 256 + threadIdx.x;
	if (r < n_ref) cov[r].covbases = 0;
}

// dsb_multi_coverage: dst |= src over nw words (the contexts' bitmaps merged before the count)
__global__ void __launch_bounds__(256) k_cover_or(uint64_t *__restrict__ dst, const uint64_t *__restrict__ src, uint64_t nw)
{
	for (uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x; q < nw; q += (uint64_t)gridDim.x * 256) dst[q] |= src[q];
}

// ---- per-window coverage (dsb_ctx_enable_coverage_windows) ----
// One wavefront per read, behind k_ref_cover on the same stream, over the same records with the same guards and the same clipped
// interval [s, e).  Window j of a reference is [jW, min((j + 1)W, LN)); its counters are win[2 (first[ref] + j)] (starts) and the
// word after it (aligned_bases).  The lanes stride over the windows s / W .. (e - 1) / W of a record: each adds the length of its
// overlap, and the lane that holds window s / W adds the record's start.  Agent-scope no-return atomic adds throughout, for the reason
// k_ref_cover gives: records of different workgroups share windows.
__global__ void __launch_bounds__(256) k_ref_windows(const DsbReadOut *__restrict__ rout, const DsbHitOut *__restrict__ hout, const DsbCounters *__restrict__ counters,
                                                     uint32_t cap_hout, uint32_t n, const uint64_t *__restrict__ ref_len, const uint64_t *__restrict__ first,
                                                     uint32_t n_ref, uint32_t W, uint64_t *win)
{
	const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (i >= n) return;
	const uint32_t nh = dsb_hits_out(counters->hits, cap_hout);
	const DsbReadOut r = rout[i];
	const uint32_t nrec = dsb_hits_cut(r.first, r.n, nh) ? 0u : r.n;
	if (!nrec) return;
	const dsb_hit *h = reinterpret_cast<const dsb_hit *>(hout + r.first);
	for (uint32_t k = 0; k < nrec; k++) {
		const dsb_hit *c = h + k;
		if (!dsb_sam_counted(c, k) || c->ref_ID >= n_ref) continue;
		const uint64_t ln = ref_len[c->ref_ID];
		const uint64_t s = c->t_st < ln ? c->t_st : ln, e = c->t_ed < ln ? c->t_ed : ln;
		if (e <= s) continue;
		uint64_t *w = win + 2 * first[c->ref_ID];
		const uint64_t j0 = s / W, j1 = (e - 1) / W;               // (e <= LN: j1 is a window of the reference)
		for (uint64_t j = j0 + lane; j <= j1; j += 64) {
			const uint64_t lo = j * W > s ? j * W : s, hi = (j + 1) * W < e ? (j + 1) * W : e;
			__hip_atomic_fetch_add(w + 2 * j + 1, hi - lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			if (j == j0) __hip_atomic_fetch_add(w + 2 * j, (uint64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
	}
}

// the set bits of bitmap word q of a reference (its bases [64 q, 64 q + 64)) that lie in the bases [y0, y1); the word must meet them
__device__ inline uint32_t window_bits(uint64_t word, uint64_t q, uint64_t y0, uint64_t y1)
{
	const uint64_t lo = q * 64 < y0 ? y0 - q * 64 : 0, hi = q * 64 + 64 > y1 ? y1 - q * 64 : 64;
	return (uint32_t)__popcll(word & (hi == 64 ? ~0ull : (1ull << hi) - 1) & (~0ull << lo));
}

// A fetch: the covbases of every window, from words [w0, w0 + nw) of the bitmap (bits[q - w0] holds word q), balanced by words as
// k_cover_count is and with its walk over the references of a chunk.  The chunk's words of reference r are the bases [x0, x1) of r
// (x1 clipped at LN), which meet the windows x0 / W .. (x1 - 1) / W; each of them gets the popcount of its bases INSIDE the chunk, so a
// window cut by the chunk's ends -- a window of more than DSB_COVER_CHUNK words, or one across a chunk boundary of the merge of
// dsb_multi_coverage_windows -- gets one partial sum per chunk, and a word that straddles windows is counted under a mask in each.
// From DSB_WINDOW_WAVE bases (64 words) on, the wavefront takes the windows one after the other, the lanes striding over the
// window's words, and lane 0 adds the reduced sum; below it each lane takes a window and walks its words (at most 65) alone.
// Either way one atomic add per wavefront and window.
#define DSB_WINDOW_WAVE 4096
__global__ void __launch_bounds__(256) k_window_count(const uint64_t *__restrict__ bits, uint64_t w0, uint64_t nw, const uint64_t *__restrict__ word_off,
                                                      const uint64_t *__restrict__ ref_len, const uint64_t *__restrict__ first, uint32_t n_ref, uint32_t W,
                                                      uint64_t *wcov)
{
	const uint64_t a = w0 + ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * DSB_COVER_CHUNK, end = w0 + nw;
	const uint32_t lane = threadIdx.x & 63;
	if (a >= end) return;
	const uint64_t b = a + DSB_COVER_CHUNK < end ? a + DSB_COVER_CHUNK : end;
	uint32_t lo = 0, hi = n_ref;                           // word_off[lo] <= a < word_off[hi], as k_cover_count
	while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (word_off[mid] <= a) lo = mid; else hi = mid; }
	for (uint32_t r = lo;; r++) {
		const uint64_t off = word_off[r], s = off > a ? off : a, e = word_off[r + 1] < b ? word_off[r + 1] : b;
		if (e > s) {
			const uint64_t ln = ref_len[r], x0 = (s - off) * 64, x1 = (e - off) * 64 < ln ? (e - off) * 64 : ln;   // (word e - 1 is one of r's: x1 > x0)
			const uint64_t at = off - w0;                      // word q of r is bits[at + q] (modulo 2^64 where r began before w0: only q >= s - off is read)
			uint64_t *o = wcov + first[r];
			const uint64_t j0 = x0 / W, j1 = (x1 - 1) / W;
			if (W >= DSB_WINDOW_WAVE) {
				for (uint64_t j = j0; j <= j1; j++) {
					const uint64_t y0 = j * W > x0 ? j * W : x0, y1 = (j + 1) * W < x1 ? (j + 1) * W : x1;
					uint32_t sum = 0;                          // (at most 64 bits x DSB_COVER_CHUNK words)
					for (uint64_t q = (y0 >> 6) + lane; q <= ((y1 - 1) >> 6); q += 64) sum += window_bits(bits[at + q], q, y0, y1);
					for (int t = 32; t; t >>= 1) sum += __shfl_xor(sum, t, 64);
					if (lane == 0 && sum) __hip_atomic_fetch_add(o + j, (uint64_t)sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				}
			} else {
				for (uint64_t j = j0 + lane; j <= j1; j += 64) {
					const uint64_t y0 = j * W > x0 ? j * W : x0, y1 = (j + 1) * W < x1 ? (j + 1) * W : x1;
					uint32_t sum = 0;
					for (uint64_t q = y0 >> 6; q <= ((y1 - 1) >> 6); q++) sum += window_bits(bits[at + q], q, y0, y1);
					if (sum) __hip_atomic_fetch_add(o + j, (uint64_t)sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				}
			}
		}
		if (e >= b) break;
	}
}

// before a count: the covbases slots = 0 (starts and aligned_bases stay)
__global__ void __launch_bounds__(256) k_window_clear(uint64_t *wcov, uint64_t n_win)
{
	for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < n_win; j += (uint64_t)gridDim.x * 256) wcov[j] = 0;
}

// ---- per-reference abundance by EM (dsb_ctx_enable_abundance) ----
// A read's candidate set in the run-wide store: its references (ascending ref_ID) are elems[off .. off + len); hash is
// dsb_em_mix over them, never 0.  An unclassified read has an empty record (len 0, hash 0).  Batch b's reads own records
// [base_s, base_s + n) in input order and its elements lie at base_e + (the read's first hit in the hit buffer), so no two
// reads share room and no atomics place them; the gaps (hits that are not candidates) cost 4 bytes per hit.
struct DsbEmSet { uint64_t hash; uint32_t off, len; };
// the store's counters: [0] records, [1] elements (gaps included), [2] nonzero = a set found no room (nothing written)
#define DSB_EM_CNT 4
__device__ __host__ inline uint64_t dsb_em_mix(uint64_t h, uint32_t r)
{
	h ^= (uint64_t)r + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2);
	h ^= h >> 31; h *= 0xbf58476d1ce4e5b9ull; h ^= h >> 29;
	return h;
}
#define DSB_EM_HASH0 0x2545f4914f6cdd1dull

__device__ inline uint32_t wave_min_u32(uint32_t v) { for (int o = 32; o; o >>= 1) { const uint32_t t = __shfl_xor(v, o, 64); v = t < v ? t : v; } return v; }
__device__ inline uint32_t wave_max_u32(uint32_t v) { for (int o = 32; o; o >>= 1) { const uint32_t t = __shfl_xor(v, o, 64); v = t > v ? t : v; } return v; }

// One wavefront per read, after the batch's last classify work (the hits dsb_batch_fetch hands out: dsb_hits_out, dsb_hits_cut).
// S_max = the largest AS over the read's hits on references < n_ref; the candidate set is the distinct ref_IDs of the hits with
// AS * 1000 >= S_max * min_permille (a reference's best hit passes exactly when one of its hits does).  The set is formed in
// ascending order by repeated selection: each round the lanes find the smallest qualifying ref_ID above the last one taken
// (|C| + 1 rounds over the hits).  Lane j keeps element j for the first 64; a longer set is selected a second time as it is written.
// The host reserved n records and cap_hout elements behind (base_s, base_e); thread 0 of the grid moves the counters past them.
// hash_mask keeps the low DSB_EM_HASH_BITS of the hash (all 64 by default; a hash of 0 becomes 1 either way).
__global__ void __launch_bounds__(256) k_em_collect(const DsbReadOut *__restrict__ rout, const DsbHitOut *__restrict__ hout, const DsbCounters *__restrict__ counters,
                                                    uint32_t cap_hout, uint32_t n, uint32_t n_ref, uint32_t min_permille, DsbEmSet *__restrict__ sets,
                                                    uint32_t *__restrict__ elems, unsigned long long *em_cnt, uint64_t base_s, uint64_t base_e,
                                                    uint64_t cap_sets, uint64_t cap_elems, uint64_t hash_mask)
{
	const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	const uint32_t nh = dsb_hits_out(counters->hits, cap_hout);
	if (blockIdx.x == 0 && threadIdx.x == 0) { em_cnt[0] = base_s + n; em_cnt[1] = base_e + nh; }
	if (i >= n) return;
	const DsbReadOut r = rout[i];
	const uint32_t nrec = dsb_hits_cut(r.first, r.n, nh) ? 0u : r.n;
	const uint64_t s = base_s + i, e = base_e + (nrec ? r.first : 0u);
	if (s >= cap_sets) { if (lane == 0) atomicOr(em_cnt + 2, 1ull); return; }
	const DsbHitOut *h = hout + r.first;
	uint32_t smax = 0; bool valid = false;
	for (uint32_t q = lane; q < nrec; q += 64) if (h[q].ref_ID < n_ref) { valid = true; smax = h[q].sum_score > smax ? h[q].sum_score : smax; }
	if (!__ballot(valid)) {                                        // unclassified (or only hits on references beyond the index)
		if (lane == 0) { DsbEmSet o; o.hash = 0; o.off = (uint32_t)e; o.len = 0; sets[s] = o; }
		return;
	}
	smax = wave_max_u32(smax);
	const uint64_t thr = (uint64_t)smax * min_permille;
	uint32_t k = 0, mine = 0; int64_t last = -1; uint64_t hash = DSB_EM_HASH0;
	for (;;) {
		uint32_t best = 0xffffffffu;
		for (uint32_t q = lane; q < nrec; q += 64) {
			const uint32_t ref = h[q].ref_ID;
			if (ref < n_ref && (int64_t)ref > last && ref < best && (uint64_t)h[q].sum_score * 1000u >= thr) best = ref;
		}
		best = wave_min_u32(best);
		if (best == 0xffffffffu) break;
		if (k == lane) mine = best;
		hash = dsb_em_mix(hash, best); last = best; k++;
	}
	if (e + k > cap_elems) { if (lane == 0) atomicOr(em_cnt + 2, 1ull); return; }
	hash &= hash_mask;                                            // (DSB_EM_HASH_BITS: collisions on purpose)
	if (lane == 0) { DsbEmSet o; o.hash = hash ? hash : 1; o.off = (uint32_t)e; o.len = k; sets[s] = o; }
	if (k <= 64) { if (lane < k) elems[e + lane] = mine; return; }
	last = -1;
	for (uint32_t j = 0; j < k; j++) {
		uint32_t best = 0xffffffffu;
		for (uint32_t q = lane; q < nrec; q += 64) {
			const uint32_t ref = h[q].ref_ID;
			if (ref < n_ref && (int64_t)ref > last && ref < best && (uint64_t)h[q].sum_score * 1000u >= thr) best = ref;
		}
		best = wave_min_u32(best);
		if (lane == 0) elems[e + j] = best;
		last = best;
	}
}

// class build: the (hash, set index) keys of the store
__global__ void __launch_bounds__(256) k_em_keys(const DsbEmSet *__restrict__ sets, uint32_t n, uint64_t *__restrict__ key, uint32_t *__restrict__ val)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i < n) { key[i] = sets[i].hash; val[i] = i; }
}

__device__ inline bool em_same_set(const DsbEmSet &a, const DsbEmSet &b, const uint32_t *elems)
{
	if (a.len != b.len) return false;
	for (uint32_t j = 0; j < a.len; j++) if (elems[a.off + j] != elems[b.off + j]) return false;
	return true;
}

// after the sort by hash: head[i] = 1 where a class starts (the empty records, hash 0, come first and start none).  Neighbours of one hash are compared element by element; two different
// sets of one hash set *collide (the host then orders each run of one hash by the sets themselves and marks again).
__global__ void __launch_bounds__(256) k_em_mark(const DsbEmSet *__restrict__ sets, const uint32_t *__restrict__ elems, const uint32_t *__restrict__ order,
                                                 uint32_t n, uint32_t *__restrict__ head, unsigned int *collide)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	uint32_t hd = sets[order[i]].len != 0;                        // (empty records: hash 0, sorted in front of every class)
	if (i && hd) {
		const DsbEmSet a = sets[order[i - 1]], b = sets[order[i]];
		if (a.hash == b.hash) {
			hd = em_same_set(a, b, elems) ? 0u : 1u;
			if (hd) atomicOr(collide, 1u);
		}
	}
	head[i] = hd;
}

// classes from the inclusive scan of head (cls[i] = class of sorted position i, plus one): the first position of each class and the
// length of its set
__global__ void __launch_bounds__(256) k_em_classes(const DsbEmSet *__restrict__ sets, const uint32_t *__restrict__ order, const uint32_t *__restrict__ head,
                                                    const uint32_t *__restrict__ cls, uint32_t n, uint32_t *__restrict__ start, uint32_t *__restrict__ len)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n || !head[i]) return;
	const uint32_t k = cls[i] - 1;
	start[k] = i;
	len[k] = sets[order[i]].len;
}

// the class elements in class order (cref[coff[k] ..) = the set of class k, ascending) and the class of each (for the transposed CSR)
__global__ void __launch_bounds__(256) k_em_fill(const DsbEmSet *__restrict__ sets, const uint32_t *__restrict__ elems, const uint32_t *__restrict__ order,
                                                 const uint32_t *__restrict__ start, const uint32_t *__restrict__ coff, uint32_t K, uint32_t *__restrict__ cref,
                                                 uint32_t *__restrict__ ccls)
{
	const uint32_t k = blockIdx.x * 256 + threadIdx.x;
	if (k >= K) return;
	const DsbEmSet s = sets[order[start[k]]];
	for (uint32_t j = 0; j < s.len; j++) { cref[coff[k] + j] = elems[s.off + j]; ccls[coff[k] + j] = k; }
}

// per reference: the first entry of its classes in the (ref, class)-sorted pairs (lower bound; roff[n_ref] = the pair count)
__global__ void __launch_bounds__(256) k_em_rowoff(const uint32_t *__restrict__ sref, uint32_t m, uint32_t n_ref, uint32_t *__restrict__ roff)
{
	const uint32_t r = blockIdx.x * 256 + threadIdx.x;
	if (r > n_ref) return;
	uint32_t lo = 0, hi = m;
	while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (sref[mid] < r) lo = mid + 1; else hi = mid; }
	roff[r] = lo;
}

// per reference: numreads, uniqreads, and the starting share (1 / R for a reference in some class, else 0)
__global__ void __launch_bounds__(256) k_em_init(const uint32_t *__restrict__ roff, const uint32_t *__restrict__ scls, const uint32_t *__restrict__ start,
                                                 const uint32_t *__restrict__ clen, uint32_t n_ref, double a0, double *__restrict__ a,
                                                 unsigned long long *__restrict__ numreads, unsigned long long *__restrict__ uniqreads)
{
	const uint32_t r = blockIdx.x * 256 + threadIdx.x;
	if (r >= n_ref) return;
	unsigned long long nr = 0, ur = 0;
	for (uint32_t q = roff[r]; q < roff[r + 1]; q++) {
		const uint32_t k = scls[q], c = start[k + 1] - start[k];
		nr += c;
		if (clen[k] == 1) ur += c;
	}
	numreads[r] = nr; uniqreads[r] = ur;
	a[r] = roff[r + 1] > roff[r] ? a0 : 0.0;
}

// EM state on the device: chg[it & 1] = max_r N |a'_r - a_r| of iteration it (as the bits of a non-negative double: their
// unsigned order is the doubles' order); done / iters: the iteration after which the criterion held
struct DsbEmState { unsigned long long chg[2]; unsigned int done, iters; };

// iteration it, first half: per class k, denom = sum over its set (ascending ref_ID) of a_s / L_s, coef = c_k / denom (0 for a
// denominator that underflowed to 0).  Every thread sees the same state: once iteration it - 1 met the criterion, all return.
__global__ void __launch_bounds__(256) k_em_class(const uint32_t *__restrict__ cref, const uint32_t *__restrict__ coff, const uint32_t *__restrict__ start,
                                                  uint32_t K, const double *__restrict__ a, const double *__restrict__ L, double tol, uint32_t it,
                                                  DsbEmState *st, double *__restrict__ coef)
{
	if (st->done) return;
	const uint32_t k = blockIdx.x * 256 + threadIdx.x;
	if (it > 0 && __longlong_as_double((long long)st->chg[(it - 1) & 1]) < tol) {
		if (k == 0) { st->done = 1; st->iters = it; }
		return;
	}
	if (k == 0) st->chg[it & 1] = 0;
	if (k >= K) return;
	double d = 0.0;
	for (uint32_t q = coff[k]; q < coff[k + 1]; q++) { const uint32_t s = cref[q]; d += a[s] / L[s]; }
	coef[k] = d > 0.0 ? (double)(start[k + 1] - start[k]) / d : 0.0;
}

// second half: one wavefront per reference.  t = sum of coef over the reference's classes in class order -- lane j takes the
// classes j, j + 64, ... in order, then a fixed butterfly over the 64 partial sums -- and a'_r = (a_r / L_r) t / N.
__global__ void __launch_bounds__(256) k_em_ref(const uint32_t *__restrict__ roff, const uint32_t *__restrict__ scls, const double *__restrict__ coef,
                                                uint32_t n_ref, const double *__restrict__ a, const double *__restrict__ L, double N, uint32_t it,
                                                DsbEmState *st, double *__restrict__ an)
{
	if (st->done) return;
	const uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (r >= n_ref) return;
	const uint32_t q0 = roff[r], q1 = roff[r + 1];
	if (q0 == q1) { if (lane == 0) an[r] = 0.0; return; }
	double t = 0.0;
	for (uint32_t q = q0 + lane; q < q1; q += 64) t += coef[scls[q]];
	for (int o = 32; o; o >>= 1) t += __shfl_xor(t, o, 64);
	if (lane) return;
	const double v = (a[r] / L[r]) * t / N;
	an[r] = v;
	const double d = fabs(v - a[r]) * N;
	atomicMax(&st->chg[it & 1], (unsigned long long)__double_as_longlong(d));
}

// dsb_multi_abundance: the offsets of a context's sets, moved behind the elements of the contexts before it
__global__ void __launch_bounds__(256) k_em_rebase(DsbEmSet *sets, uint32_t n, uint32_t base)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i < n) sets[i].off += base;
}

// ---- per-read assignment by the EM posterior (dsb_*_abundance_assign) ----
// After the solve, one thread per class k (k_em_class's launch shape, and its walk: the class's references in ascending ref_ID):
// w_s = a_s / L_s from the final shares, d = their sum in that order (k_em_class's d_k), the reference with the largest w -- the
// strict comparison leaves equal weights to the smallest ref_ID -- and posterior = w_ref / d (d == 0, every share underflowed: the
// first reference and 0).  Every read of the class gets this record.
__global__ void __launch_bounds__(256) k_em_assign_class(const uint32_t *__restrict__ cref, const uint32_t *__restrict__ coff, uint32_t K,
                                                         const double *__restrict__ a, const double *__restrict__ L, dsb_read_assign *__restrict__ crec)
{
	const uint32_t k = blockIdx.x * 256 + threadIdx.x;
	if (k >= K) return;
	const uint32_t q0 = coff[k], q1 = coff[k + 1];
	double d = 0.0, best = -1.0; uint32_t ref = DSB_ASSIGN_NONE;
	for (uint32_t q = q0; q < q1; q++) {
		const uint32_t s = cref[q];
		const double w = a[s] / L[s];
		d += w;
		if (w > best) { best = w; ref = s; }
	}
	dsb_read_assign o; o.ref_ID = ref; o.n_cand = q1 - q0; o.posterior = d > 0.0 ? best / d : 0.0;
	crec[k] = o;
}

// One lane per store record: sorted position p holds record order[p], of class cls[p] - 1; the empty records (unclassified reads)
// are sorted in front of every class, cls 0 (p < start[0]), and get the "none" record.  order is a permutation: plain stores.
__global__ void __launch_bounds__(256) k_em_assign_read(const uint32_t *__restrict__ order, const uint32_t *__restrict__ cls, uint32_t n,
                                                        const dsb_read_assign *__restrict__ crec, dsb_read_assign *__restrict__ out)
{
	const uint32_t p = blockIdx.x * 256 + threadIdx.x;
	if (p >= n) return;
	const uint32_t k = cls[p];
	dsb_read_assign o; o.ref_ID = DSB_ASSIGN_NONE; o.n_cand = 0; o.posterior = 0.0;
	if (k) o = crec[k - 1];
	out[order[p]] = o;
}

// ---- per-read LCA classification (dsb_ctx_enable_lca) ----
// The lowest common ancestor of two rooted taxids, 0 standing for "nothing yet" (the neutral value: taxid 0 is never rooted).  The
// deeper node is lifted to the other's depth, then both are lifted until they meet -- at taxid 1 at the latest, since both chains
// reach it.  *d follows the result's depth.  Every walk stops after `bound` steps (max_depth + 2, as k_read_taxon's).
__device__ inline uint32_t lca_join(uint32_t a, uint32_t da, uint32_t b, uint32_t db, const uint32_t *__restrict__ parent, uint32_t bound, uint32_t *d)
{
	if (!a) { *d = db; return b; }
	if (!b) { *d = da; return a; }
	for (uint32_t s = 0; da > db && s < bound; s++) { a = parent[a]; da--; }
	for (uint32_t s = 0; db > da && s < bound; s++) { b = parent[b]; db--; }
	for (uint32_t s = 0; a != b && da && s < bound; s++) { a = parent[a]; b = parent[b]; da--; }
	*d = da;
	return a;
}

// One wavefront per read, after the batch's last classify work (the hits dsb_batch_fetch hands out: dsb_hits_out, dsb_hits_cut), for
// the reason k_em_collect gives: a strain-dense read has hundreds of hits.  Pass 1: S_max by wave-max over the hits on references
// < n_ref.  Pass 2: lane j takes the hits j, j + 64, ...; a passing hit (AS * 1000 >= S_max * min_permille) whose reference's taxid is
// rooted (depth table) is folded into the lane's LCA; n_pass is the sum of the rounds' ballots.  Then a 6-step xor butterfly with
// lca_join as the operator -- it is associative, commutative and idempotent, so every lane ends with the LCA of all.  AMBIGUOUS: a
// lane saw two taxids, or a ballot finds a lane whose first taxid is not the first lane's.  Lane 0 writes the record.
__global__ void __launch_bounds__(256) k_read_lca(const DsbReadOut *__restrict__ rout, const DsbHitOut *__restrict__ hout, const DsbCounters *__restrict__ counters,
                                                  uint32_t cap_hout, uint32_t n, const uint32_t *__restrict__ parent, const uint16_t *__restrict__ depth,
                                                  const uint32_t *__restrict__ ref_tid, uint32_t n_ref, uint32_t max_tid, uint32_t bound, uint32_t min_permille,
                                                  dsb_read_lca *__restrict__ out)
{
	const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (i >= n) return;
	const uint32_t nh = dsb_hits_out(counters->hits, cap_hout);
	const DsbReadOut r = rout[i];
	const uint32_t nrec = dsb_hits_cut(r.first, r.n, nh) ? 0u : r.n;
	const DsbHitOut *h = hout + r.first;
	dsb_read_lca o; o.taxid = 0; o.score = 0; o.n_pass = 0; o.depth = 0; o.flags = 0; o.pad = 0;
	uint32_t smax = 0; bool valid = false;
	for (uint32_t q = lane; q < nrec; q += 64) if (h[q].ref_ID < n_ref) { valid = true; smax = h[q].sum_score > smax ? h[q].sum_score : smax; }
	if (!__ballot(valid)) { if (lane == 0) out[i] = o; return; }   // unclassified (or only hits on references beyond the index)
	smax = wave_max_u32(smax);
	const uint64_t thr = (uint64_t)smax * min_permille;
	uint32_t mine = 0, mine_d = 0, first = 0, n_pass = 0; bool two = false;
	for (uint32_t q0 = 0; q0 < nrec; q0 += 64) {
		const uint32_t q = q0 + lane;
		const bool pass = q < nrec && h[q].ref_ID < n_ref && (uint64_t)h[q].sum_score * 1000u >= thr;
		n_pass += (uint32_t)__popcll(__ballot(pass));
		if (!pass) continue;
		const uint32_t t = ref_tid[h[q].ref_ID];
		if (t < 1 || t > max_tid) continue;                       // (DSB_TID_NONE included)
		const uint32_t d = depth[t];
		if (d == DSB_DEPTH_UNROOTED) continue;
		if (!first) first = t; else if (t != first) two = true;
		mine = lca_join(mine, mine_d, t, d, parent, bound, &mine_d);
	}
	const uint64_t have = __ballot(first != 0);
	bool amb = false;
	if (have) {
		const uint32_t lead = __shfl(first, __ffsll((unsigned long long)have) - 1, 64);
		amb = __ballot(two || (first != 0 && first != lead)) != 0;
	}
	for (int s = 32; s; s >>= 1) {
		const uint32_t t = __shfl_xor(mine, s, 64), d = __shfl_xor(mine_d, s, 64);
		mine = lca_join(mine, mine_d, t, d, parent, bound, &mine_d);
	}
	if (lane) return;
	o.taxid = mine; o.score = smax; o.n_pass = n_pass; o.depth = (uint16_t)(mine ? mine_d : 0);
	o.flags = (uint8_t)(DSB_LCA_CLASSIFIED | (mine ? 0 : DSB_LCA_NO_TAXON) | (amb ? DSB_LCA_AMBIGUOUS : 0));
	out[i] = o;
}

// One lane per read, behind k_read_lca on the same stream: the run's direct counts and summary.  Most reads of a sample share a
// few taxa, and one atomic per read on a hot line is what k_em_collect's first version paid for: equal taxids are
// grouped inside the wavefront first -- the taxid of the first lane still waiting, a ballot of the lanes that hold it, one atomicAdd
// of the group's size by that lane -- so a wavefront issues one add per distinct taxid.  The summary the same way: one add per
// counter and wavefront.  Integer adds only: the sums do not depend on the order.  sum: [0] reads, [1] classified (taxid != 0),
// [2] NO_TAXON, [3] AMBIGUOUS.
__global__ void __launch_bounds__(256) k_lca_count(const dsb_read_lca *__restrict__ rec, uint32_t n, uint32_t max_tid, unsigned long long *direct,
                                                   unsigned long long *sum)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
	const bool live = i < n;
	dsb_read_lca r; r.taxid = 0; r.flags = 0;
	if (live) r = rec[i];
	const uint32_t tid = r.taxid <= max_tid ? r.taxid : 0;         // (k_read_lca writes no taxid above max_tid)
	uint64_t left = __ballot(live && tid != 0);
	const unsigned long long n_cls = (unsigned long long)__popcll(left);
	while (left) {
		const int src = __ffsll((unsigned long long)left) - 1;
		const uint32_t t = __shfl(tid, src, 64);
		const uint64_t m = __ballot(live && tid == t);
		if ((int)lane == src) atomicAdd(direct + t, (unsigned long long)__popcll(m));
		left &= ~m;
	}
	const unsigned long long n_live = (unsigned long long)__popcll(__ballot(live));
	const unsigned long long n_not = (unsigned long long)__popcll(__ballot(live && (r.flags & DSB_LCA_NO_TAXON)));
	const unsigned long long n_amb = (unsigned long long)__popcll(__ballot(live && (r.flags & DSB_LCA_AMBIGUOUS)));
	if (lane == 0) {
		if (n_live) atomicAdd(sum + 0, n_live);
		if (n_cls) atomicAdd(sum + 1, n_cls);
		if (n_not) atomicAdd(sum + 2, n_not);
		if (n_amb) atomicAdd(sum + 3, n_amb);
	}
}

// The roll-up of dsb_ctx_lca_counts, reading direct only.  cnt: [0] listed taxids, [1] nodes with clade > 0.
// k_lca_list: the taxids with direct > 0 (in any order: only integer sums follow)
__global__ void __launch_bounds__(256) k_lca_list(const unsigned long long *__restrict__ direct, uint32_t max_tid, uint32_t *__restrict__ list, unsigned int *cnt)
{
	const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (t >= 1 && t <= max_tid && direct[t]) list[atomicAdd(cnt, 1u)] = (uint32_t)t;
}

// one lane per listed taxid: its count is added to clade[] of every node from it to taxid 1 (few nodes times depth: contention does
// not matter here); the lane that finds a node at 0 lists it (a count is never 0, so exactly one does).  Listed taxids are rooted.
__global__ void __launch_bounds__(256) k_lca_rollup(const unsigned long long *__restrict__ direct, const uint32_t *__restrict__ list, uint32_t n_list,
                                                    const uint32_t *__restrict__ parent, uint32_t max_tid, uint32_t bound, unsigned long long *clade,
                                                    uint32_t *__restrict__ nodes, uint32_t cap_nodes, unsigned int *cnt)
{
	const uint32_t k = blockIdx.x * 256 + threadIdx.x;
	if (k >= n_list) return;
	const unsigned long long c = direct[list[k]];
	uint32_t p = list[k];
	for (uint32_t s = 0; s < bound && p >= 1 && p <= max_tid; s++) {
		if (atomicAdd(clade + p, c) == 0) { const uint32_t at = atomicAdd(cnt + 1, 1u); if (at < cap_nodes) nodes[at] = p; }
		if (p == 1) break;
		p = parent[p];
	}
}

// the rows of the nodes (sorted by taxid before this)
__global__ void __launch_bounds__(256) k_lca_rows(const uint32_t *__restrict__ nodes, uint32_t n, const unsigned long long *__restrict__ clade,
                                                  const unsigned long long *__restrict__ direct, dsb_taxon_count *__restrict__ rows)
{
	const uint32_t k = blockIdx.x * 256 + threadIdx.x;
	if (k >= n) return;
	dsb_taxon_count o; o.taxid = nodes[k]; o.pad = 0; o.clade_reads = clade[o.taxid]; o.direct_reads = direct[o.taxid];
	rows[k] = o;
}

// dsb_multi_lca_counts: dst += src over n counters
__global__ void __launch_bounds__(256) k_lca_add(unsigned long long *__restrict__ dst, const unsigned long long *__restrict__ src, uint64_t n)
{
	for (uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (uint64_t)gridDim.x * 256) dst[q] += src[q];
}

// ================================== host side ====================================================
// temporary device buffers of one call (em_solve, the merges of a dsb_multi), freed together when it returns
struct DevScratch {
	std::vector<void *> p;
	~DevScratch() { for (void *q : p) hipFree(q); }
	template <class T> T *get(size_t n)
	{
		void *q = nullptr;
		if (hipMalloc(&q, (n ? n : 1) * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
		p.push_back(q); return (T *)q;
	}
};

// ---- taxonomy ----
static void lca_free(dsb_ctx *c);
extern "C" int dsb_ctx_set_taxonomy(dsb_ctx *c, const dsb_taxonomy *tx)
{
	if (!c) return DSB_EINVAL;
	if (tx && !tx->acyclic) return DSB_EINVAL;                 // (dsb_taxonomy_load_any: the device's walks need the bound)
	HIPCHK(hipSetDevice(c->device));
	HIPCHK(hipStreamSynchronize(c->stream));
	lca_free(c);                                               // (LCA reads this taxonomy's tables: a ctx whose LCA is on leaves it here)
	hipFree(c->taxa.d_parent); hipFree(c->taxa.d_ref_tid); c->taxa.d_parent = c->taxa.d_ref_tid = nullptr;
	c->taxa.tx = nullptr; c->taxa.run = c->taxa.done = false;
	if (!tx) { hipFree(c->taxa.d_taxa); c->taxa.d_taxa = nullptr; c->taxa.cap_taxa = 0; return DSB_OK; }
	const size_t n_ref = (size_t)dsb_index_n_ref(c->idx);
	std::vector<uint32_t> rt(n_ref ? n_ref : 1);
	for (size_t r = 0; r < n_ref; r++) rt[r] = dsb_ref_taxid(dsb_index_ref_name(c->idx, (uint32_t)r));
	if (hipMalloc((void **)&c->taxa.d_parent, ((size_t)tx->max_tid + 1) * 4) != hipSuccess || hipMalloc((void **)&c->taxa.d_ref_tid, rt.size() * 4) != hipSuccess) {
		hipFree(c->taxa.d_parent); c->taxa.d_parent = nullptr; return DSB_ENOMEM;
	}
	HIPCHK(hipMemcpy(c->taxa.d_parent, tx->parent, ((size_t)tx->max_tid + 1) * 4, hipMemcpyHostToDevice));
	HIPCHK(hipMemcpy(c->taxa.d_ref_tid, rt.data(), rt.size() * 4, hipMemcpyHostToDevice));
	// the per-read records for the batches the ctx was sized for now, not inside a batch (grow() waits for the device)
	if (grow(&c->taxa.d_taxa, &c->taxa.cap_taxa, std::max(c->cap_rout, (size_t)c->opts.max_batch_reads))) return DSB_ENOMEM;
	c->taxa.tx = tx;
	return DSB_OK;
}

extern "C" int dsb_batch_taxa(dsb_ctx *c, const dsb_read_taxon **out)
{
	if (!c || !out || !c->taxa.tx || !c->taxa.run) return DSB_EINVAL;
	if (!c->taxa.done) { dsb_result r; int rc = dsb_batch_fetch(c, &r); if (rc && rc != DSB_ECAP) return rc; }
	*out = c->taxa.h_taxa.data();
	return DSB_OK;
}

// ---- per-reference coverage ----
static void windows_free(dsb_ctx *c)
{
	hipFree(c->cover.d_first); hipFree(c->cover.d_win); hipFree(c->cover.d_wcov);
	c->cover.d_first = c->cover.d_win = c->cover.d_wcov = nullptr; c->cover.win = 0; c->cover.n_win = 0;
}
static void cover_free(dsb_ctx *c)
{
	windows_free(c);
	hipFree(c->cover.d_bits); hipFree(c->cover.d_off); hipFree(c->cover.d_len); hipFree(c->cover.d_cov);
	c->cover = DsbCover();
}

extern "C" int dsb_ctx_reset_coverage(dsb_ctx *c)
{
	if (!c || !c->cover.d_cov) return DSB_EINVAL;
	HIPCHK(hipSetDevice(c->device));
	const size_t n_ref = (size_t)dsb_index_n_ref(c->idx);
	HIPCHK(hipMemsetAsync(c->cover.d_bits, 0, (c->cover.words ? c->cover.words : 1) * 8, c->stream));
	HIPCHK(hipMemsetAsync(c->cover.d_cov, 0, (n_ref ? n_ref : 1) * sizeof(dsb_ref_coverage), c->stream));
	if (c->cover.win) {                                        // (one state: the windows describe the reads the bitmap does)
		HIPCHK(hipMemsetAsync(c->cover.d_win, 0, (c->cover.n_win ? c->cover.n_win : 1) * 16, c->stream));
		HIPCHK(hipMemsetAsync(c->cover.d_wcov, 0, (c->cover.n_win ? c->cover.n_win : 1) * 8, c->stream));
	}
	HIPCHK(hipStreamSynchronize(c->stream));
	return DSB_OK;
}

extern "C" int dsb_ctx_enable_coverage(dsb_ctx *c, int on)
{
	if (!c) return DSB_EINVAL;
	HIPCHK(hipSetDevice(c->device));
	HIPCHK(hipStreamSynchronize(c->stream));
	if (on && c->cover.d_cov) return dsb_ctx_reset_coverage(c);
	cover_free(c);
	if (!on) return DSB_OK;
	const size_t n_ref = (size_t)dsb_index_n_ref(c->idx);
	std::vector<uint64_t> off(n_ref + 1, 0), len(n_ref ? n_ref : 1, 0);
	for (size_t r = 0; r < n_ref; r++) { len[r] = dsb_index_ref_len(c->idx, (uint32_t)r); off[r + 1] = off[r] + (len[r] + 63) / 64; }
	const uint64_t nw = off[n_ref];
	if (hipMalloc((void **)&c->cover.d_bits, (nw ? nw : 1) * 8) != hipSuccess || hipMalloc((void **)&c->cover.d_off, off.size() * 8) != hipSuccess ||
	    hipMalloc((void **)&c->cover.d_len, len.size() * 8) != hipSuccess || hipMalloc((void **)&c->cover.d_cov, (n_ref ? n_ref : 1) * sizeof(dsb_ref_coverage)) != hipSuccess) {
		cover_free(c); (void)hipGetLastError(); return DSB_ENOMEM;
	}
	c->cover.words = nw;
	HIPCHK(hipMemcpy(c->cover.d_off, off.data(), off.size() * 8, hipMemcpyHostToDevice));
	HIPCHK(hipMemcpy(c->cover.d_len, len.data(), len.size() * 8, hipMemcpyHostToDevice));
	return dsb_ctx_reset_coverage(c);
}

// covbases of words [w0, w0 + nw) of the bitmap, held in bits[0 .. nw), added to c's counters
static void cover_count(dsb_ctx *c, const uint64_t *bits, uint64_t w0, uint64_t nw, hipStream_t st)
{
	if (!nw) return;
	const uint64_t waves = (nw + DSB_COVER_CHUNK - 1) / DSB_COVER_CHUNK;
	hipLaunchKernelGGL(k_cover_count, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, bits, w0, nw, (const uint64_t *)c->cover.d_off,
	                   (uint32_t)dsb_index_n_ref(c->idx), c->cover.d_cov);
}

extern "C" int dsb_ctx_coverage(dsb_ctx *c, dsb_ref_coverage *out)
{
	if (!c || !out || !c->cover.d_cov) return DSB_EINVAL;
	HIPCHK(hipSetDevice(c->device));
	const uint32_t n_ref = (uint32_t)dsb_index_n_ref(c->idx);
	if (!n_ref) return DSB_OK;
	// on the ctx's stream: after the batches it has run (k_ref_cover leaves covbases alone, so a batch behind it changes nothing here)
	hipLaunchKernelGGL(k_cover_clear, dim3((n_ref + 255) / 256), dim3(256), 0, c->stream, c->cover.d_cov, n_ref);
	cover_count(c, c->cover.d_bits, 0, c->cover.words, c->stream);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(out, c->cover.d_cov, n_ref * sizeof(dsb_ref_coverage), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return DSB_OK;
}

// ---- per-window coverage ----
extern "C" uint64_t dsb_coverage_n_windows(const dsb_index *idx, uint32_t window)
{
	if (!idx || !window) return 0;
	const uint64_t n_ref = dsb_index_n_ref(idx);
	uint64_t n = 0;
	for (uint64_t r = 0; r < n_ref; r++) { const uint64_t ln = dsb_index_ref_len(idx, (uint32_t)r); n += ln / window + (ln % window != 0); }
	return n;
}

extern "C" int dsb_ctx_enable_coverage_windows(dsb_ctx *c, uint32_t window)
{
	if (!c) return DSB_EINVAL;
	HIPCHK(hipSetDevice(c->device));
	HIPCHK(hipStreamSynchronize(c->stream));
	windows_free(c);
	if (!window) return DSB_OK;
	if (!c->cover.d_cov) return DSB_EINVAL;
	const size_t n_ref = (size_t)dsb_index_n_ref(c->idx);
	std::vector<uint64_t> first(n_ref + 1, 0);
	for (size_t r = 0; r < n_ref; r++) { const uint64_t ln = dsb_index_ref_len(c->idx, (uint32_t)r); first[r + 1] = first[r] + ln / window + (ln % window != 0); }
	const uint64_t nw = first[n_ref];
	if (nw > (uint64_t)1 << 58) return DSB_ENOMEM;             // (24 bytes each)
	if (hipMalloc((void **)&c->cover.d_first, first.size() * 8) != hipSuccess || hipMalloc((void **)&c->cover.d_win, (size_t)(nw ? nw : 1) * 16) != hipSuccess ||
	    hipMalloc((void **)&c->cover.d_wcov, (size_t)(nw ? nw : 1) * 8) != hipSuccess) {
		windows_free(c); (void)hipGetLastError(); return DSB_ENOMEM;
	}
	c->cover.win = window; c->cover.n_win = nw;
	HIPCHK(hipMemcpy(c->cover.d_first, first.data(), first.size() * 8, hipMemcpyHostToDevice));
	return dsb_ctx_reset_coverage(c);                          // bitmap, counters and windows: the same reads from here on
}

// covbases of the windows met by words [w0, w0 + nw) of the bitmap, held in bits[0 .. nw), added to c's covbases slots
static void window_count(dsb_ctx *c, const uint64_t *bits, uint64_t w0, uint64_t nw, hipStream_t st)
{
	if (!nw) return;
	const uint64_t waves = (nw + DSB_COVER_CHUNK - 1) / DSB_COVER_CHUNK;
	hipLaunchKernelGGL(k_window_count, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, bits, w0, nw, (const uint64_t *)c->cover.d_off, (const uint64_t *)c->cover.d_len,
	                   (const uint64_t *)c->cover.d_first, (uint32_t)dsb_index_n_ref(c->idx), c->cover.win, c->cover.d_wcov);
}
static void window_clear(dsb_ctx *c, hipStream_t st)
{
	if (!c->cover.n_win) return;
	hipLaunchKernelGGL(k_window_clear, dim3((unsigned)std::min<uint64_t>((c->cover.n_win + 255) / 256, 8192)), dim3(256), 0, st, c->cover.d_wcov, c->cover.n_win);
}

// the n windows to the host: {starts, aligned_bases} from sa (on the current device) and covbases from wcov, a piece at a time through two
// staging vectors, all on stream st
static int windows_deliver(hipStream_t st, const uint64_t *sa, const uint64_t *wcov, uint64_t n, dsb_cov_window *out)
{
	const uint64_t piece = (uint64_t)1 << 20;
	std::vector<uint64_t> h_sa((size_t)std::min(n, piece) * 2), h_cb((size_t)std::min(n, piece));
	for (uint64_t j0 = 0; j0 < n; j0 += piece) {
		const uint64_t k = n - j0 < piece ? n - j0 : piece;
		HIPCHK(hipMemcpyAsync(h_sa.data(), sa + 2 * j0, k * 16, hipMemcpyDeviceToHost, st));
		HIPCHK(hipMemcpyAsync(h_cb.data(), wcov + j0, k * 8, hipMemcpyDeviceToHost, st));
		HIPCHK(hipStreamSynchronize(st));
		for (uint64_t j = 0; j < k; j++) { dsb_cov_window &o = out[j0 + j]; o.starts = h_sa[2 * j]; o.aligned_bases = h_sa[2 * j + 1]; o.covbases = h_cb[j]; }
	}
	return DSB_OK;
}

extern "C" int dsb_ctx_coverage_windows(dsb_ctx *c, dsb_cov_window *out, size_t cap, size_t *n)
{
	if (!c || !n || !c->cover.win) return DSB_EINVAL;
	*n = (size_t)c->cover.n_win;
	if (!out) return DSB_OK;                                   // (count only)
	if (cap < *n) return DSB_ECAP;
	HIPCHK(hipSetDevice(c->device));
	// on the ctx's stream, as dsb_ctx_coverage: k_ref_windows leaves the covbases slots alone, so a batch behind this changes nothing here
	window_clear(c, c->stream);
	window_count(c, c->cover.d_bits, 0, c->cover.words, c->stream);
	HIPCHK(hipGetLastError());
	return windows_deliver(c->stream, c->cover.d_win, c->cover.d_wcov, c->cover.n_win, out);
}

extern "C" long dsb_coverage_windows_format(const dsb_index *x, const dsb_ref_coverage *cov, const dsb_cov_window *win, uint32_t window, char *buf, size_t cap)
{
	if (!x || !cov || !win || !window || (!buf && cap)) return -1;
	size_t o = 0; int w;
#define EMIT(...) do { w = snprintf(buf + o, cap > o ? cap - o : 0, __VA_ARGS__); if (w < 0 || (size_t)w >= (cap > o ? cap - o : 0)) return -1; o += (size_t)w; } while (0)
	EMIT("#rname\tstart\tend\tnumreads\tcovbases\tcoverage\tmeandepth\n");
	const uint64_t n_ref = dsb_index_n_ref(x);
	uint64_t first = 0;
	for (uint64_t r = 0; r < n_ref; r++) {
		const uint64_t ln = dsb_index_ref_len(x, (uint32_t)r), nw = ln / window + (ln % window != 0);
		if (cov[r].numreads)
			for (uint64_t j = 0; j < nw; j++) {
				const dsb_cov_window &c = win[first + j];
				const uint64_t s = j * window, e = s + window < ln ? s + window : ln;
				EMIT("%s\t%llu\t%llu\t%llu\t%llu\t%g\t%g\n", dsb_index_ref_name(x, (uint32_t)r), (unsigned long long)s, (unsigned long long)e, (unsigned long long)c.starts,
				     (unsigned long long)c.covbases, 100.0 * (double)c.covbases / (double)(e - s), (double)c.aligned_bases / (double)(e - s));
			}
		first += nw;
	}
#undef EMIT
	return (long)o;
}

// ---- per-reference abundance ----
static void em_free(dsb_ctx *c)
{
	hipFree(c->em.d_sets); hipFree(c->em.d_elems); hipFree(c->em.d_cnt);
	c->em = DsbEmStore();
}

// a store array grown to hold `need` entries (at least twice what it held), its first `used` entries kept
template <class T> static int em_grow(T **p, size_t *cap, size_t used, size_t need)
{
	if (need <= *cap) return DSB_OK;
	const size_t nc = std::max(need, 2 * *cap);
	T *q = nullptr;
	if (hipMalloc((void **)&q, nc * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); return DSB_ENOMEM; }
	if (used && hipMemcpy(q, *p, used * sizeof(T), hipMemcpyDeviceToDevice) != hipSuccess) { hipFree(q); return DSB_ENODEV; }
	hipFree(*p); *p = q; *cap = nc;
	return DSB_OK;
}

// room for n_sets more sets and n_elems more elements.  The device must be done with the store (no k_em_collect pending).
static int em_reserve(dsb_ctx *c, size_t n_sets, size_t n_elems)
{
	unsigned long long cnt[DSB_EM_CNT];
	HIPCHK(hipMemcpy(cnt, c->em.d_cnt, sizeof cnt, hipMemcpyDeviceToHost));
	if (cnt[2]) return DSB_ENOMEM;                             // (a set found no room: cannot happen after a reservation)
	const size_t need_s = (size_t)cnt[0] + n_sets, need_e = (size_t)cnt[1] + n_elems;
	if (need_s > 0xffffffffu || need_e > 0xffffffffu) return DSB_ENOMEM;   // (record indices and element offsets are 32-bit)
	int rc = em_grow(&c->em.d_sets, &c->em.cap_sets, (size_t)cnt[0], need_s);
	if (!rc) rc = em_grow(&c->em.d_elems, &c->em.cap_elems, (size_t)cnt[1], need_e);
	c->em.used_sets = (size_t)cnt[0]; c->em.used_elems = (size_t)cnt[1];
	return rc;
}

extern "C" int dsb_ctx_reset_abundance(dsb_ctx *c)
{
	if (!c || !c->em.d_cnt) return DSB_EINVAL;
	HIPCHK(hipSetDevice(c->device));
	HIPCHK(hipMemsetAsync(c->em.d_cnt, 0, DSB_EM_CNT * sizeof(unsigned long long), c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	c->em.reads = 0; c->em.log.clear();
	return DSB_OK;
}

extern "C" int dsb_ctx_enable_abundance(dsb_ctx *c, int on, uint32_t min_permille)
{
	if (!c || (on && (min_permille < 1 || min_permille > 1000))) return DSB_EINVAL;
	HIPCHK(hipSetDevice(c->device));
	HIPCHK(hipStreamSynchronize(c->stream));
	if (on && c->em.d_cnt) { c->em.permille = min_permille; return dsb_ctx_reset_abundance(c); }
	em_free(c);
	if (!on) return DSB_OK;
	if (hipMalloc((void **)&c->em.d_cnt, DSB_EM_CNT * sizeof(unsigned long long)) != hipSuccess) { (void)hipGetLastError(); c->em.d_cnt = nullptr; return DSB_ENOMEM; }
	c->em.permille = min_permille;
	return dsb_ctx_reset_abundance(c);
}

#define EMCK(e) do { if ((e) != hipSuccess) { (void)hipGetLastError(); return DSB_ENODEV; } } while (0)
#define EM_ITER_BLOCK 16

static int em_opts(const dsb_em_opts *o, dsb_em_opts *v)
{
	v->max_iter = 10000; v->reserved = 0; v->tol = 0.01;
	if (!o) return DSB_OK;
	if (o->max_iter < 1 || !(o->tol >= 0.0)) return DSB_EINVAL;
	*v = *o; v->reserved = 0;
	return DSB_OK;
}

// The classes of n records (elements in elems[0 .. n_elems); the empty records of unclassified reads take no part) and the EM over them, on the current device, on stream st.
//   classes: radix sort of (hash, set index); k_em_mark compares neighbours of one hash element by element (a collision: the host
//            orders each run of one hash by the sets themselves); an inclusive scan of the class heads numbers the classes.
//   CSR:     the (ref, class) pairs of every class's set, written in class order and radix-sorted by ref -- stably, so each
//            reference's classes stay in class order; the row offsets by binary search.
//   EM:      k_em_class + k_em_ref per iteration, EM_ITER_BLOCK iterations per host round trip; the device's done word makes the
//            result the state after the first iteration that met tol, whatever the block.
//   assign:  with d_assign (n records, in store order) the two kernels of DESIGN 2.10.1 behind the last iteration, *assigned = they ran
//            (they do not when no read is classified: every record is then "none", which the caller writes itself)
static int em_solve(hipStream_t st, const dsb_index *idx, const DsbEmSet *sets, const uint32_t *elems, uint32_t n, uint32_t n_elems, uint64_t reads,
                    uint32_t permille, const dsb_em_opts &o, dsb_ref_abundance *out, dsb_abundance_summary *sum, dsb_read_assign *d_assign = nullptr,
                    bool *assigned = nullptr)
{
	if (assigned) *assigned = false;
	const uint32_t n_ref = (uint32_t)dsb_index_n_ref(idx);
	memset(out, 0, (size_t)n_ref * sizeof *out); memset(sum, 0, sizeof *sum);
	sum->reads = reads; sum->min_permille = permille; sum->converged = 1;
	if (!n || !n_ref) return DSB_OK;
	DevScratch T;
	uint64_t *key = T.get<uint64_t>(n), *key_s = T.get<uint64_t>(n);
	uint32_t *val = T.get<uint32_t>(n), *order = T.get<uint32_t>(n), *head = T.get<uint32_t>(n), *cls = T.get<uint32_t>(n);
	unsigned int *flag = T.get<unsigned int>(1);
	if (!key || !key_s || !val || !order || !head || !cls || !flag) return DSB_ENOMEM;
	const dim3 gn((n + 255) / 256), b256(256);
	hipLaunchKernelGGL(k_em_keys, gn, b256, 0, st, sets, n, key, val);
	size_t tb = 0;
	EMCK(rocprim::radix_sort_pairs(nullptr, tb, key, key_s, val, order, n, 0, 64, st));
	void *tmp = T.get<uint8_t>(tb);
	if (!tmp) return DSB_ENOMEM;
	EMCK(rocprim::radix_sort_pairs(tmp, tb, key, key_s, val, order, n, 0, 64, st));
	EMCK(hipMemsetAsync(flag, 0, 4, st));
	hipLaunchKernelGGL(k_em_mark, gn, b256, 0, st, sets, elems, (const uint32_t *)order, n, head, flag);
	unsigned int collide = 0;
	EMCK(hipMemcpyAsync(&collide, flag, 4, hipMemcpyDeviceToHost, st));
	EMCK(hipStreamSynchronize(st));
	if (collide) {
		// different sets of one 64-bit hash (rare): order by (hash, length, elements) on the host, then mark again
		std::vector<DsbEmSet> hs(n); std::vector<uint32_t> ho(n), he(n_elems ? n_elems : 1);
		EMCK(hipMemcpy(hs.data(), sets, (size_t)n * sizeof(DsbEmSet), hipMemcpyDeviceToHost));
		EMCK(hipMemcpy(he.data(), elems, (size_t)n_elems * 4, hipMemcpyDeviceToHost));
		for (uint32_t i = 0; i < n; i++) ho[i] = i;
		std::sort(ho.begin(), ho.end(), [&](uint32_t x, uint32_t y) {
			const DsbEmSet &a = hs[x], &b = hs[y];
			if (a.hash != b.hash) return a.hash < b.hash;
			if (a.len != b.len) return a.len < b.len;
			return std::lexicographical_compare(he.begin() + a.off, he.begin() + a.off + a.len, he.begin() + b.off, he.begin() + b.off + b.len);
		});
		EMCK(hipMemcpy(order, ho.data(), (size_t)n * 4, hipMemcpyHostToDevice));
		EMCK(hipMemsetAsync(flag, 0, 4, st));
		hipLaunchKernelGGL(k_em_mark, gn, b256, 0, st, sets, elems, (const uint32_t *)order, n, head, flag);
	}
	EMCK(rocprim::inclusive_scan(nullptr, tb, head, cls, n, rocprim::plus<uint32_t>(), st));
	if (!(tmp = T.get<uint8_t>(tb))) return DSB_ENOMEM;
	EMCK(rocprim::inclusive_scan(tmp, tb, head, cls, n, rocprim::plus<uint32_t>(), st));
	uint32_t K = 0;
	EMCK(hipMemcpyAsync(&K, cls + (n - 1), 4, hipMemcpyDeviceToHost, st));
	EMCK(hipStreamSynchronize(st));
	if (!K) return DSB_OK;                                     // (no read classified)
	uint32_t *start = T.get<uint32_t>((size_t)K + 1), *clen = T.get<uint32_t>((size_t)K + 1), *coff = T.get<uint32_t>((size_t)K + 1);
	if (!start || !clen || !coff) return DSB_ENOMEM;
	EMCK(hipMemsetAsync(clen + K, 0, 4, st));
	EMCK(hipMemcpyAsync(start + K, &n, 4, hipMemcpyHostToDevice, st));
	hipLaunchKernelGGL(k_em_classes, gn, b256, 0, st, sets, (const uint32_t *)order, (const uint32_t *)head, (const uint32_t *)cls, n, start, clen);
	EMCK(rocprim::exclusive_scan(nullptr, tb, clen, coff, 0u, (size_t)K + 1, rocprim::plus<uint32_t>(), st));
	if (!(tmp = T.get<uint8_t>(tb))) return DSB_ENOMEM;
	EMCK(rocprim::exclusive_scan(tmp, tb, clen, coff, 0u, (size_t)K + 1, rocprim::plus<uint32_t>(), st));
	uint32_t M = 0, start0 = 0;                                 // (the records before start[0] are the empty ones)
	EMCK(hipMemcpyAsync(&M, coff + K, 4, hipMemcpyDeviceToHost, st));
	EMCK(hipMemcpyAsync(&start0, start, 4, hipMemcpyDeviceToHost, st));
	EMCK(hipStreamSynchronize(st));
	sum->classified = n - start0;
	uint32_t *cref = T.get<uint32_t>(M), *ccls = T.get<uint32_t>(M), *sref = T.get<uint32_t>(M), *scls = T.get<uint32_t>(M), *roff = T.get<uint32_t>((size_t)n_ref + 1);
	if (!cref || !ccls || !sref || !scls || !roff) return DSB_ENOMEM;
	const dim3 gk((K + 255) / 256), gr((n_ref + 256) / 256), gw((n_ref + 3) / 4);
	hipLaunchKernelGGL(k_em_fill, gk, b256, 0, st, sets, elems, (const uint32_t *)order, (const uint32_t *)start, (const uint32_t *)coff, K, cref, ccls);
	unsigned bits = 1;
	while (bits < 32 && (1ull << bits) < n_ref) bits++;
	EMCK(rocprim::radix_sort_pairs(nullptr, tb, cref, sref, ccls, scls, M, 0, bits, st));
	if (!(tmp = T.get<uint8_t>(tb))) return DSB_ENOMEM;
	EMCK(rocprim::radix_sort_pairs(tmp, tb, cref, sref, ccls, scls, M, 0, bits, st));
	hipLaunchKernelGGL(k_em_rowoff, gr, b256, 0, st, (const uint32_t *)sref, M, n_ref, roff);
	std::vector<uint32_t> hroff((size_t)n_ref + 1);
	EMCK(hipMemcpyAsync(hroff.data(), roff, hroff.size() * 4, hipMemcpyDeviceToHost, st));
	EMCK(hipStreamSynchronize(st));
	uint32_t R = 0;
	for (uint32_t r = 0; r < n_ref; r++) R += hroff[r + 1] > hroff[r];
	std::vector<double> hL(n_ref);
	for (uint32_t r = 0; r < n_ref; r++) { const uint64_t l = dsb_index_ref_len(idx, r); hL[r] = l ? (double)l : 1.0; }
	double *L = T.get<double>(n_ref), *a[2] = {T.get<double>(n_ref), T.get<double>(n_ref)}, *coef = T.get<double>(K);
	unsigned long long *nr = T.get<unsigned long long>(n_ref), *ur = T.get<unsigned long long>(n_ref);
	DsbEmState *est = T.get<DsbEmState>(1);
	if (!L || !a[0] || !a[1] || !coef || !nr || !ur || !est) return DSB_ENOMEM;
	EMCK(hipMemcpyAsync(L, hL.data(), (size_t)n_ref * 8, hipMemcpyHostToDevice, st));
	EMCK(hipMemsetAsync(est, 0, sizeof(DsbEmState), st));
	hipLaunchKernelGGL(k_em_init, gr, b256, 0, st, (const uint32_t *)roff, (const uint32_t *)scls, (const uint32_t *)start, (const uint32_t *)clen, n_ref,
	                   1.0 / (double)R, a[0], nr, ur);
	const double N = (double)(n - start0);
	DsbEmState hs; memset(&hs, 0, sizeof hs);
	for (uint32_t it = 0; it < o.max_iter;) {
		const uint32_t end = o.max_iter - it < EM_ITER_BLOCK ? o.max_iter : it + EM_ITER_BLOCK;
		for (; it < end; it++) {
			hipLaunchKernelGGL(k_em_class, gk, b256, 0, st, (const uint32_t *)cref, (const uint32_t *)coff, (const uint32_t *)start, K, (const double *)a[it & 1],
			                   (const double *)L, o.tol, it, est, coef);
			hipLaunchKernelGGL(k_em_ref, gw, b256, 0, st, (const uint32_t *)roff, (const uint32_t *)scls, (const double *)coef, n_ref, (const double *)a[it & 1],
			                   (const double *)L, N, it, est, a[(it + 1) & 1]);
		}
		EMCK(hipGetLastError());
		EMCK(hipMemcpyAsync(&hs, est, sizeof hs, hipMemcpyDeviceToHost, st));
		EMCK(hipStreamSynchronize(st));
		if (hs.done) break;
	}
	const uint32_t iters = hs.done ? hs.iters : o.max_iter;
	if (d_assign) {
		// the per-read records, from the shares the table below is made of (a[iters & 1]); done by the wait that follows
		dsb_read_assign *crec = T.get<dsb_read_assign>(K);
		if (!crec) return DSB_ENOMEM;
		hipLaunchKernelGGL(k_em_assign_class, gk, b256, 0, st, (const uint32_t *)cref, (const uint32_t *)coff, K, (const double *)a[iters & 1], (const double *)L, crec);
		hipLaunchKernelGGL(k_em_assign_read, gn, b256, 0, st, (const uint32_t *)order, (const uint32_t *)cls, n, (const dsb_read_assign *)crec, d_assign);
		EMCK(hipGetLastError());
		if (assigned) *assigned = true;
	}
	double chg = 0.0;
	memcpy(&chg, &hs.chg[(iters - 1) & 1], 8);
	std::vector<double> ha(n_ref); std::vector<unsigned long long> hnr(n_ref), hur(n_ref);
	EMCK(hipMemcpyAsync(ha.data(), a[iters & 1], (size_t)n_ref * 8, hipMemcpyDeviceToHost, st));
	EMCK(hipMemcpyAsync(hnr.data(), nr, (size_t)n_ref * 8, hipMemcpyDeviceToHost, st));
	EMCK(hipMemcpyAsync(hur.data(), ur, (size_t)n_ref * 8, hipMemcpyDeviceToHost, st));
	EMCK(hipStreamSynchronize(st));
	double W = 0.0;                                            // (in ref_ID order)
	for (uint32_t r = 0; r < n_ref; r++) W += ha[r] / hL[r];
	for (uint32_t r = 0; r < n_ref; r++) {
		dsb_ref_abundance &x = out[r];
		x.numreads = hnr[r]; x.uniqreads = hur[r];
		x.est_reads = N * ha[r]; x.read_share = ha[r];
		x.copy_share = W > 0.0 ? (ha[r] / hL[r]) / W : 0.0;
	}
	sum->classes = K; sum->iterations = iters; sum->max_change = chg;
	sum->converged = hs.done || chg < o.tol;
	return DSB_OK;
}

// the store's counters, read on the ctx's stream (after the batches it holds)
static int em_counts(dsb_ctx *c, unsigned long long cnt[DSB_EM_CNT])
{
	HIPCHK(hipMemcpyAsync(cnt, c->em.d_cnt, DSB_EM_CNT * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return cnt[2] ? DSB_ENOMEM : DSB_OK;
}

extern "C" int dsb_ctx_abundance(dsb_ctx *c, const dsb_em_opts *opts, dsb_ref_abundance *out, dsb_abundance_summary *summary)
{
	dsb_em_opts o;
	if (!c || !out || !summary || !c->em.d_cnt || em_opts(opts, &o)) return DSB_EINVAL;
	HIPCHK(hipSetDevice(c->device));
	unsigned long long cnt[DSB_EM_CNT];
	int rc = em_counts(c, cnt);
	if (rc) return rc;
	return em_solve(c->stream, c->idx, c->em.d_sets, c->em.d_elems, (uint32_t)cnt[0], (uint32_t)cnt[1], c->em.reads, c->em.permille, o, out, summary);
}

// ---- per-read assignment: the ordinal log and the delivery in input order ----
extern "C" int dsb_ctx_set_batch_ordinal(dsb_ctx *c, uint64_t first)
{
	if (!c) return DSB_EINVAL;
	InSlot &s = c->in[c->cur];
	s.ord_set = true; s.ord_first = first;
	return DSB_OK;
}

// a context's log and where its records start in the store that was solved (dsb_multi: the contexts' stores one after the other)
struct EmPiece { const std::vector<DsbEmLog> *log; uint64_t off; };

// 1 + the largest ordinal logged, or 0
static uint64_t assign_count(const std::vector<EmPiece> &pc)
{
	uint64_t n = 0;
	for (const EmPiece &p : pc) for (const DsbEmLog &e : *p.log) if (e.n) n = std::max(n, e.first + e.n);
	return n;
}

// reads[0 .. n_out) = "none", then each logged batch's records, a contiguous run of the store (d_assign, n_store records; nullptr:
// no read was classified), to reads[first ..): one copy per batch, 16 bytes per read
static int assign_deliver(hipStream_t st, const dsb_read_assign *d_assign, uint64_t n_store, const std::vector<EmPiece> &pc, dsb_read_assign *reads, uint64_t n_out)
{
	dsb_read_assign none; none.ref_ID = DSB_ASSIGN_NONE; none.n_cand = 0; none.posterior = 0.0;
	std::fill(reads, reads + n_out, none);
	if (!d_assign) return DSB_OK;
	for (const EmPiece &p : pc)
		for (const DsbEmLog &e : *p.log) {
			if (!e.n) continue;
			if (p.off + e.base + e.n > n_store || e.first + e.n > n_out) return DSB_ENODEV;     // (cannot happen: the log follows k_em_collect)
			EMCK(hipMemcpyAsync(reads + e.first, d_assign + p.off + e.base, e.n * sizeof(dsb_read_assign), hipMemcpyDeviceToHost, st));
		}
	EMCK(hipStreamSynchronize(st));
	return DSB_OK;
}

extern "C" int dsb_ctx_abundance_assign(dsb_ctx *c, const dsb_em_opts *opts, dsb_ref_abundance *out, dsb_abundance_summary *summary, dsb_read_assign *reads,
                                        size_t cap, size_t *n)
{
	dsb_em_opts o;
	if (!c || !n || !c->em.d_cnt || em_opts(opts, &o)) return DSB_EINVAL;
	const std::vector<EmPiece> pc = {{&c->em.log, 0}};
	*n = (size_t)assign_count(pc);
	if (!reads) return DSB_OK;                                 // (count only)
	if (!out || !summary) return DSB_EINVAL;
	if (cap < *n) return DSB_ECAP;
	HIPCHK(hipSetDevice(c->device));
	unsigned long long cnt[DSB_EM_CNT];
	int rc = em_counts(c, cnt);
	if (rc) return rc;
	DevScratch T;
	dsb_read_assign *d_assign = T.get<dsb_read_assign>((size_t)cnt[0]);
	if (!d_assign) return DSB_ENOMEM;
	bool ran = false;
	rc = em_solve(c->stream, c->idx, c->em.d_sets, c->em.d_elems, (uint32_t)cnt[0], (uint32_t)cnt[1], c->em.reads, c->em.permille, o, out, summary, d_assign, &ran);
	if (rc) return rc;
	return assign_deliver(c->stream, ran ? d_assign : nullptr, cnt[0], pc, reads, *n);
}

// ---- per-read LCA classification ----
#define DSB_LCA_SUM 4
static void lca_free(dsb_ctx *c)
{
	hipFree(c->lca.d_depth); hipFree(c->lca.d_direct); hipFree(c->lca.d_clade); hipFree(c->lca.d_sum); hipFree(c->lca.d_rec);
	c->lca = DsbLca();
}

extern "C" int dsb_ctx_reset_lca(dsb_ctx *c)
{
	if (!c || !c->lca.d_direct) return DSB_EINVAL;
	HIPCHK(hipSetDevice(c->device));
	HIPCHK(hipMemsetAsync(c->lca.d_direct, 0, ((size_t)c->taxa.tx->max_tid + 1) * 8, c->stream));
	HIPCHK(hipMemsetAsync(c->lca.d_sum, 0, DSB_LCA_SUM * 8, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return DSB_OK;
}

extern "C" int dsb_ctx_enable_lca(dsb_ctx *c, int on, uint32_t min_permille)
{
	if (!c || (on && (min_permille < 1 || min_permille > 1000))) return DSB_EINVAL;
	const dsb_taxonomy *tx = c->taxa.tx;
	if (on && (!tx || !tx->depth || tx->max_depth + 2 >= DSB_DEPTH_UNROOTED)) return DSB_EINVAL;
	HIPCHK(hipSetDevice(c->device));
	HIPCHK(hipStreamSynchronize(c->stream));
	if (on && c->lca.d_direct) { c->lca.permille = min_permille; return dsb_ctx_reset_lca(c); }
	lca_free(c);
	if (!on) return DSB_OK;
	const size_t nt = (size_t)tx->max_tid + 1;
	if (hipMalloc((void **)&c->lca.d_depth, nt * 2) != hipSuccess || hipMalloc((void **)&c->lca.d_direct, nt * 8) != hipSuccess ||
	    hipMalloc((void **)&c->lca.d_clade, nt * 8) != hipSuccess || hipMalloc((void **)&c->lca.d_sum, DSB_LCA_SUM * 8) != hipSuccess ||
	    grow(&c->lca.d_rec, &c->lca.cap_rec, std::max(c->cap_rout, (size_t)c->opts.max_batch_reads))) {
		lca_free(c); (void)hipGetLastError(); return DSB_ENOMEM;
	}
	HIPCHK(hipMemcpy(c->lca.d_depth, tx->depth, nt * 2, hipMemcpyHostToDevice));
	c->lca.permille = min_permille;
	return dsb_ctx_reset_lca(c);
}

extern "C" int dsb_batch_lca(dsb_ctx *c, const dsb_read_lca **out)
{
	if (!c || !out || !c->lca.d_direct || !c->lca.run) return DSB_EINVAL;
	if (!c->lca.done) { dsb_result r; int rc = dsb_batch_fetch(c, &r); if (rc && rc != DSB_ECAP) return rc; }
	*out = c->lca.h_rec.data();
	return DSB_OK;
}

// The roll-up over a direct table on c's device, on stream st (after the batches it counted), reading it only: the taxids with
// direct > 0 are listed, each adds its count along its chain to taxid 1 into c's clade table (zeroed first), the nodes that got a
// count are sorted by taxid and their (taxid, clade, direct) rows are copied: the tables themselves never cross PCIe.
static int lca_rollup(dsb_ctx *c, const unsigned long long *direct, hipStream_t st, dsb_taxon_count *out, size_t cap, size_t *n)
{
	const dsb_taxonomy *tx = c->taxa.tx;
	const uint32_t max_tid = tx->max_tid, bound = tx->max_depth + 2;
	DevScratch T;
	uint32_t *list = T.get<uint32_t>((size_t)max_tid + 1);
	unsigned int *cnt = T.get<unsigned int>(2);
	if (!list || !cnt) return DSB_ENOMEM;
	EMCK(hipMemsetAsync(cnt, 0, 8, st));
	EMCK(hipMemsetAsync(c->lca.d_clade, 0, ((size_t)max_tid + 1) * 8, st));
	hipLaunchKernelGGL(k_lca_list, dim3((unsigned)(((size_t)max_tid + 256) / 256)), dim3(256), 0, st, direct, max_tid, list, cnt);
	unsigned int h[2] = {0, 0};
	EMCK(hipMemcpyAsync(h, cnt, 4, hipMemcpyDeviceToHost, st));
	EMCK(hipStreamSynchronize(st));
	*n = 0;
	if (!h[0]) return DSB_OK;
	const size_t cap_nodes = std::min((size_t)h[0] * ((size_t)tx->max_depth + 1), (size_t)max_tid);
	uint32_t *nodes = T.get<uint32_t>(cap_nodes), *sorted = T.get<uint32_t>(cap_nodes);
	if (!nodes || !sorted) return DSB_ENOMEM;
	hipLaunchKernelGGL(k_lca_rollup, dim3((h[0] + 255) / 256), dim3(256), 0, st, direct, (const uint32_t *)list, (uint32_t)h[0], (const uint32_t *)c->taxa.d_parent,
	                   max_tid, bound, c->lca.d_clade, nodes, (uint32_t)cap_nodes, cnt);
	EMCK(hipGetLastError());
	EMCK(hipMemcpyAsync(h, cnt, 8, hipMemcpyDeviceToHost, st));
	EMCK(hipStreamSynchronize(st));
	if (h[1] > cap_nodes) return DSB_ENODEV;                   // (cannot happen: a node is listed once)
	const uint32_t nn = h[1];
	size_t tb = 0;
	EMCK(rocprim::radix_sort_keys(nullptr, tb, nodes, sorted, nn, 0, 32, st));
	void *tmp = T.get<uint8_t>(tb);
	dsb_taxon_count *rows = T.get<dsb_taxon_count>(nn);
	if (!tmp || !rows) return DSB_ENOMEM;
	EMCK(rocprim::radix_sort_keys(tmp, tb, nodes, sorted, nn, 0, 32, st));
	hipLaunchKernelGGL(k_lca_rows, dim3((nn + 255) / 256), dim3(256), 0, st, (const uint32_t *)sorted, nn, (const unsigned long long *)c->lca.d_clade, direct, rows);
	EMCK(hipGetLastError());
	*n = nn;
	const size_t take = out ? std::min(cap, (size_t)nn) : 0;
	if (take) EMCK(hipMemcpyAsync(out, rows, take * sizeof(dsb_taxon_count), hipMemcpyDeviceToHost, st));
	EMCK(hipStreamSynchronize(st));
	return out && cap < nn ? DSB_ECAP : DSB_OK;
}

// the summary counters of a context, read on its stream
static int lca_sums(dsb_ctx *c, unsigned long long s[DSB_LCA_SUM])
{
	HIPCHK(hipSetDevice(c->device));
	HIPCHK(hipMemcpyAsync(s, c->lca.d_sum, DSB_LCA_SUM * 8, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return DSB_OK;
}

extern "C" int dsb_ctx_lca_counts(dsb_ctx *c, dsb_taxon_count *out, size_t cap, size_t *n, dsb_lca_summary *summary)
{
	if (!c || !n || !c->lca.d_direct) return DSB_EINVAL;
	unsigned long long s[DSB_LCA_SUM];
	if (int rc = lca_sums(c, s)) return rc;
	if (summary) { summary->reads = s[0]; summary->classified = s[1]; summary->no_taxon = s[2]; summary->ambiguous = s[3]; summary->min_permille = c->lca.permille; summary->reserved = 0; }
	return lca_rollup(c, c->lca.d_direct, c->stream, out, cap, n);
}

// ---- the seam with the classify driver (dsb_gpu.hip) ----
// the hit buffer's arguments of the per-read kernels: k_read_taxon, k_ref_cover, k_ref_windows, k_em_collect and k_read_lca
#define DSB_BATCH_HITS(b) (b).rout, (b).hout, (b).counters, (uint32_t)(b).cap_hout

int reductions_run(dsb_ctx *c, const DsbBatchView &b)
{
	const uint32_t n_ref = (uint32_t)dsb_index_n_ref(c->idx);
	if (c->taxa.tx) {
		// the per-read taxa: after every classify launch of the batch (the second runs and the run after a regrown hit buffer included)
		if (grow(&c->taxa.d_taxa, &c->taxa.cap_taxa, b.n)) return DSB_ENOMEM;
		const uint32_t bound = c->taxa.tx->max_depth + 2;
		hipLaunchKernelGGL(k_read_taxon, dim3((b.n + 255) / 256), dim3(256), 0, b.st, DSB_BATCH_HITS(b), b.rd, b.n, (const uint32_t *)c->taxa.d_parent,
		                   (const uint32_t *)c->taxa.d_ref_tid, n_ref, c->taxa.tx->max_tid, bound, c->opts.max_sec_N, c->taxa.d_taxa);
		c->taxa.run = true;
	}
	if (c->cover.d_cov) {
		// the per-reference coverage, after the same launches, whether or not a taxonomy is attached
		hipLaunchKernelGGL(k_ref_cover, dim3((b.n + 3) / 4), dim3(256), 0, b.st, DSB_BATCH_HITS(b), b.n, (const uint64_t *)c->cover.d_len, (const uint64_t *)c->cover.d_off,
		                   n_ref, c->cover.d_bits, c->cover.d_cov);
		// and, when windows are on, the per-window starts and aligned bases of the same records
		if (c->cover.win)
			hipLaunchKernelGGL(k_ref_windows, dim3((b.n + 3) / 4), dim3(256), 0, b.st, DSB_BATCH_HITS(b), b.n, (const uint64_t *)c->cover.d_len, (const uint64_t *)c->cover.d_first,
			                   n_ref, c->cover.win, c->cover.d_win);
	}
	if (c->em.d_cnt) {
		// the candidate sets of the batch's reads, after the same launches.  Room for n records and for every hit the buffer can
		// hold (a read's set lies in the room of its hits) is made first: the store's counters are read here, where the stream
		// has already run everything before this batch's second run (ev[3]) and nothing of this batch touched them.
		if (int rc = em_reserve(c, b.n, b.cap_hout)) return rc;
		// the ordinal log of DESIGN 2.10.1: where the batch's records lie in the store and which reads of the input they are
		c->em.log.push_back({(uint64_t)c->em.used_sets, b.ord_set ? b.ord_first : c->em.reads, (uint64_t)b.n});
		c->em.reads += b.n;
		hipLaunchKernelGGL(k_em_collect, dim3((b.n + 3) / 4), dim3(256), 0, b.st, DSB_BATCH_HITS(b), b.n, n_ref, c->em.permille,
		                   c->em.d_sets, c->em.d_elems, c->em.d_cnt, (uint64_t)c->em.used_sets, (uint64_t)c->em.used_elems, (uint64_t)c->em.cap_sets,
		                   (uint64_t)c->em.cap_elems, (uint64_t)c->knobs.em_hash_mask);
	}
	if (c->lca.d_direct) {
		// the per-read LCA records of the batch and, behind them, the run's counts: after the same launches, never in a graph
		if (grow(&c->lca.d_rec, &c->lca.cap_rec, b.n)) return DSB_ENOMEM;
		const dsb_taxonomy *tx = c->taxa.tx;
		hipLaunchKernelGGL(k_read_lca, dim3((b.n + 3) / 4), dim3(256), 0, b.st, DSB_BATCH_HITS(b), b.n, (const uint32_t *)c->taxa.d_parent, (const uint16_t *)c->lca.d_depth,
		                   (const uint32_t *)c->taxa.d_ref_tid, n_ref, tx->max_tid, tx->max_depth + 2, c->lca.permille, c->lca.d_rec);
		hipLaunchKernelGGL(k_lca_count, dim3((b.n + 255) / 256), dim3(256), 0, b.st, (const dsb_read_lca *)c->lca.d_rec, b.n, tx->max_tid, c->lca.d_direct, c->lca.d_sum);
		c->lca.run = true;
	}
	if (c->ident.d_tab) return identity_run(c, b);             // per-hit edit distance and the per-reference identity table (dsb_identity.hip)
	return DSB_OK;
}

int reductions_fetch(dsb_ctx *c, size_t n, bool queued)
{
	c->taxa.done = false;
	if (c->taxa.run) { c->taxa.h_taxa.resize(n); if (n) HIPCHK(hipMemcpyAsync(c->taxa.h_taxa.data(), c->taxa.d_taxa, n * sizeof(dsb_read_taxon), hipMemcpyDeviceToHost, c->stream)); }
	c->lca.done = false;
	if (c->lca.run) { c->lca.h_rec.resize(n); if (n) HIPCHK(hipMemcpyAsync(c->lca.h_rec.data(), c->lca.d_rec, n * sizeof(dsb_read_lca), hipMemcpyDeviceToHost, c->stream)); }
	c->ident.done = false;
	if (c->ident.run) { if (int rc = identity_fetch_queue(c, c->h_hout.size())) return rc; }    // (queued is set whenever the batch has hits)
	if (queued || ((c->taxa.run || c->lca.run) && n)) HIPCHK(hipStreamSynchronize(c->stream));
	c->lca.done = c->lca.run; c->ident.done = c->ident.run;
	if (!c->taxa.run) return DSB_OK;
	// the reads the device left to the host get their taxon here (rare: see k_read_taxon)
	const dsb_hit *H = reinterpret_cast<const dsb_hit *>(c->h_hout.data());
	const InSlot &s = c->in[c->cur];
	for (size_t i = 0; i < n; i++)
		if (c->taxa.h_taxa[i].flags & DSB_TAXON_HOST)
			c->taxa.h_taxa[i].taxid = dsb_read_taxid_host(c->taxa.tx, c->idx, s.h_rd[i].len, H + c->res_reads[i].first, c->res_reads[i].n, c->opts.max_sec_N);
	c->taxa.done = true;
	return DSB_OK;
}

void reductions_release(dsb_ctx *c)
{
	hipFree(c->taxa.d_parent); hipFree(c->taxa.d_ref_tid); hipFree(c->taxa.d_taxa); cover_free(c); em_free(c); lca_free(c); identity_release(c);
}

// ---- several contexts (dsb_multi) ----
// enable(c, true) on every context; if one fails, enable(c, false) on all of them and its error is returned
template <class F> static int multi_enable(dsb_multi *m, F enable)
{
	for (dsb_ctx *c : m->ctx) { int rc = enable(c, true); if (rc) { for (dsb_ctx *d : m->ctx) enable(d, false); return rc; } }
	return DSB_OK;
}

// bytes from device `dev` to device `dev0`, on stream st of dev0: a copy within the device, or a peer copy
static hipError_t copy_to(void *dst, int dev0, const void *src, int dev, size_t bytes, hipStream_t st)
{
	return dev == dev0 ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st) : hipMemcpyPeerAsync(dst, dev0, src, dev, bytes, st);
}

extern "C" int dsb_multi_set_taxonomy(dsb_multi *m, const dsb_taxonomy *tx)
{
	if (!m) return DSB_EINVAL;
	m->tx = nullptr; m->taxa_ok = false;
	m->lca_on = m->lca_ok = false;                              // (dsb_ctx_set_taxonomy turns each context's LCA off)
	int rc = multi_enable(m, [&](dsb_ctx *c, bool on) { return dsb_ctx_set_taxonomy(c, on ? tx : nullptr); });
	if (rc) return rc;
	m->tx = tx;
	return DSB_OK;
}
extern "C" int dsb_multi_taxa(dsb_multi *m, const dsb_read_taxon **out)
{
	if (!m || !out || !m->tx || !m->taxa_ok) return DSB_EINVAL;
	*out = m->taxa.data();
	return DSB_OK;
}

extern "C" int dsb_multi_enable_coverage(dsb_multi *m, int on)
{
	if (!m) return DSB_EINVAL;
	return multi_enable(m, [&](dsb_ctx *c, bool en) { return dsb_ctx_enable_coverage(c, en ? on : 0); });
}

// The contexts' bitmaps ORed chunk by chunk into a buffer on the first context's device -- read in place where a context shares
// that device, copied over (copy_to) where it does not -- and each chunk counted there, on the first context's stream: per reference
// into its covbases counters (refs), per window into its covbases slots (wins), both cleared first.  The contexts' own bitmaps are left
// as they are; the caller has waited for every context's stream, and waits for the first one's before T, which holds the buffers, goes.
static int multi_cover_count(dsb_multi *m, DevScratch &T, bool refs, bool wins)
{
	dsb_ctx *c0 = m->ctx[0];
	const uint32_t n_ref = (uint32_t)dsb_index_n_ref(m->idx);
	bool remote = false;
	for (dsb_ctx *c : m->ctx) remote |= c->device != c0->device;
	const uint64_t nw = c0->cover.words, chunk = nw < (4ull << 20) ? nw : (4ull << 20);   // (32 MiB of words per chunk)
	uint64_t *acc = nw ? T.get<uint64_t>(chunk) : nullptr, *buf = nw && remote ? T.get<uint64_t>(chunk) : nullptr;
	if (nw && (!acc || (remote && !buf))) return DSB_ENOMEM;
	const hipStream_t st = c0->stream;
	if (refs) hipLaunchKernelGGL(k_cover_clear, dim3((n_ref + 255) / 256), dim3(256), 0, st, c0->cover.d_cov, n_ref);
	if (wins) window_clear(c0, st);
	int rc = DSB_OK;
	for (uint64_t w0 = 0; w0 < nw && !rc; w0 += chunk) {
		const uint64_t k = nw - w0 < chunk ? nw - w0 : chunk;
		const unsigned grid = (unsigned)std::min<uint64_t>((k + 255) / 256, 8192);
		if (copy_to(acc, c0->device, c0->cover.d_bits + w0, c0->device, k * 8, st) != hipSuccess) rc = DSB_ENODEV;
		for (size_t i = 1; i < m->ctx.size() && !rc; i++) {
			const dsb_ctx *c = m->ctx[i];
			const uint64_t *src = c->cover.d_bits + w0;
			if (c->device != c0->device) {
				if (copy_to(buf, c0->device, src, c->device, k * 8, st) != hipSuccess) { rc = DSB_ENODEV; break; }
				src = buf;
			}
			hipLaunchKernelGGL(k_cover_or, dim3(grid), dim3(256), 0, st, acc, src, k);
		}
		if (!rc && refs) cover_count(c0, acc, w0, k, st);
		if (!rc && wins) window_count(c0, acc, w0, k, st);    // (a window cut by the chunk's end gets its other part from the next chunk)
	}
	if (!rc && hipGetLastError() != hipSuccess) rc = DSB_ENODEV;
	return rc;
}

// The contexts' coverage merged: the counters are added on the host; covbases is counted from the merged bitmap (multi_cover_count).
extern "C" int dsb_multi_coverage(dsb_multi *m, dsb_ref_coverage *out)
{
	if (!m || !out || m->ctx.empty()) return DSB_EINVAL;
	for (dsb_ctx *c : m->ctx) if (!c->cover.d_cov) return DSB_EINVAL;
	dsb_ctx *c0 = m->ctx[0];
	if (m->ctx.size() == 1) return dsb_ctx_coverage(c0, out);
	const uint32_t n_ref = (uint32_t)dsb_index_n_ref(m->idx);
	if (!n_ref) return DSB_OK;
	memset(out, 0, n_ref * sizeof *out);
	std::vector<dsb_ref_coverage> part(n_ref);
	for (dsb_ctx *c : m->ctx) {
		HIPCHK(hipSetDevice(c->device));
		HIPCHK(hipStreamSynchronize(c->stream));
		HIPCHK(hipMemcpy(part.data(), c->cover.d_cov, n_ref * sizeof(dsb_ref_coverage), hipMemcpyDeviceToHost));
		for (uint32_t r = 0; r < n_ref; r++) { out[r].numreads += part[r].numreads; out[r].aligned_bases += part[r].aligned_bases; out[r].mapq_sum += part[r].mapq_sum; }
	}
	HIPCHK(hipSetDevice(c0->device));
	const hipStream_t st = c0->stream;
	DevScratch T;
	int rc = multi_cover_count(m, T, true, false);
	if (!rc && hipMemcpyAsync(part.data(), c0->cover.d_cov, n_ref * sizeof(dsb_ref_coverage), hipMemcpyDeviceToHost, st) != hipSuccess) rc = DSB_ENODEV;
	if (hipStreamSynchronize(st) != hipSuccess) rc = DSB_ENODEV;
	if (rc) return rc;
	for (uint32_t r = 0; r < n_ref; r++) out[r].covbases = part[r].covbases;
	return DSB_OK;
}

extern "C" int dsb_multi_enable_coverage_windows(dsb_multi *m, uint32_t window)
{
	if (!m) return DSB_EINVAL;
	return multi_enable(m, [&](dsb_ctx *c, bool en) { return dsb_ctx_enable_coverage_windows(c, en ? window : 0); });
}

// The contexts' windows merged: starts and aligned_bases are added into a table on the first context's device (k_lca_add is the u64
// vector add; a context on another device is copied over first), covbases is counted per window from the merged bitmap
// (multi_cover_count) into the first context's slots.  Integer sums and a union: what one context would have counted.
extern "C" int dsb_multi_coverage_windows(dsb_multi *m, dsb_cov_window *out, size_t cap, size_t *n)
{
	if (!m || !n || m->ctx.empty()) return DSB_EINVAL;
	dsb_ctx *c0 = m->ctx[0];
	for (dsb_ctx *c : m->ctx) if (!c->cover.win || c->cover.win != c0->cover.win) return DSB_EINVAL;
	if (m->ctx.size() == 1) return dsb_ctx_coverage_windows(c0, out, cap, n);
	const uint64_t nwin = c0->cover.n_win;
	*n = (size_t)nwin;
	if (!out) return DSB_OK;                                   // (count only)
	if (cap < *n) return DSB_ECAP;
	if (!nwin) return DSB_OK;
	bool remote = false;
	for (dsb_ctx *c : m->ctx) {
		HIPCHK(hipSetDevice(c->device));
		HIPCHK(hipStreamSynchronize(c->stream));                // (the context's counters and bitmap are final)
		remote |= c->device != c0->device;
	}
	HIPCHK(hipSetDevice(c0->device));
	const hipStream_t st = c0->stream;
	DevScratch T;
	uint64_t *acc = T.get<uint64_t>(2 * nwin), *buf = remote ? T.get<uint64_t>(2 * nwin) : nullptr;
	if (!acc || (remote && !buf)) return DSB_ENOMEM;
	int rc = copy_to(acc, c0->device, c0->cover.d_win, c0->device, nwin * 16, st) == hipSuccess ? DSB_OK : DSB_ENODEV;
	const unsigned grid = (unsigned)std::min<uint64_t>((2 * nwin + 255) / 256, 8192);
	for (size_t i = 1; i < m->ctx.size() && !rc; i++) {
		const dsb_ctx *c = m->ctx[i];
		const uint64_t *src = c->cover.d_win;
		if (c->device != c0->device) {
			if (copy_to(buf, c0->device, src, c->device, nwin * 16, st) != hipSuccess) { rc = DSB_ENODEV; break; }
			src = buf;
		}
		hipLaunchKernelGGL(k_lca_add, dim3(grid), dim3(256), 0, st, (unsigned long long *)acc, (const unsigned long long *)src, 2 * nwin);
	}
	if (!rc) rc = multi_cover_count(m, T, false, true);
	if (!rc) rc = windows_deliver(st, acc, c0->cover.d_wcov, nwin, out);
	if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = DSB_ENODEV;
	return rc;
}
extern "C" int dsb_multi_enable_abundance(dsb_multi *m, int on, uint32_t min_permille)
{
	if (!m) return DSB_EINVAL;
	return multi_enable(m, [&](dsb_ctx *c, bool en) { return dsb_ctx_enable_abundance(c, en ? on : 0, en ? min_permille : 0); });
}

// The contexts' stores one after the other on the first context's device (copy_to), each context's element offsets moved
// behind the elements before it, then the solve of one context.  The classes, their order and every sum depend only on the
// multiset of sets, so the result is bitwise that of one context.
// reads: nullptr (dsb_multi_abundance), or the n_out per-read records of dsb_multi_abundance_assign
static int multi_solve(dsb_multi *m, const dsb_em_opts &o, dsb_ref_abundance *out, dsb_abundance_summary *summary, dsb_read_assign *reads, uint64_t n_out)
{
	dsb_ctx *c0 = m->ctx[0];
	std::vector<unsigned long long> ns(m->ctx.size()), ne(m->ctx.size());
	uint64_t S = 0, E = 0, n_reads = 0;
	for (size_t i = 0; i < m->ctx.size(); i++) {
		dsb_ctx *c = m->ctx[i];
		HIPCHK(hipSetDevice(c->device));
		unsigned long long cnt[DSB_EM_CNT];
		int rc = em_counts(c, cnt);
		if (rc) return rc;
		ns[i] = cnt[0]; ne[i] = cnt[1]; S += cnt[0]; E += cnt[1]; n_reads += c->em.reads;
	}
	if (S > 0xffffffffu || E > 0xffffffffu) return DSB_ENOMEM;
	HIPCHK(hipSetDevice(c0->device));
	const hipStream_t st = c0->stream;
	DevScratch T;
	DsbEmSet *sets = T.get<DsbEmSet>(S); uint32_t *elems = T.get<uint32_t>(E);
	if (!sets || !elems) return DSB_ENOMEM;
	uint64_t s0 = 0, e0 = 0;
	for (size_t i = 0; i < m->ctx.size(); i++) {
		const dsb_ctx *c = m->ctx[i];
		if (ns[i]) {
			EMCK(copy_to(sets + s0, c0->device, c->em.d_sets, c->device, ns[i] * sizeof(DsbEmSet), st));
			if (ne[i]) EMCK(copy_to(elems + e0, c0->device, c->em.d_elems, c->device, ne[i] * 4, st));
			if (e0) hipLaunchKernelGGL(k_em_rebase, dim3((unsigned)((ns[i] + 255) / 256)), dim3(256), 0, st, sets + s0, (uint32_t)ns[i], (uint32_t)e0);
		}
		s0 += ns[i]; e0 += ne[i];
	}
	EMCK(hipGetLastError());
	if (!reads) return em_solve(st, m->idx, sets, elems, (uint32_t)S, (uint32_t)E, n_reads, c0->em.permille, o, out, summary);
	dsb_read_assign *d_assign = T.get<dsb_read_assign>(S);
	if (!d_assign) return DSB_ENOMEM;
	bool ran = false;
	int rc = em_solve(st, m->idx, sets, elems, (uint32_t)S, (uint32_t)E, n_reads, c0->em.permille, o, out, summary, d_assign, &ran);
	if (rc) return rc;
	std::vector<EmPiece> pc;
	s0 = 0;
	for (size_t i = 0; i < m->ctx.size(); i++) { pc.push_back({&m->ctx[i]->em.log, s0}); s0 += ns[i]; }
	return assign_deliver(st, ran ? d_assign : nullptr, S, pc, reads, n_out);
}

extern "C" int dsb_multi_abundance(dsb_multi *m, const dsb_em_opts *opts, dsb_ref_abundance *out, dsb_abundance_summary *summary)
{
	dsb_em_opts o;
	if (!m || !out || !summary || m->ctx.empty() || em_opts(opts, &o)) return DSB_EINVAL;
	dsb_ctx *c0 = m->ctx[0];
	for (dsb_ctx *c : m->ctx) if (!c->em.d_cnt || c->em.permille != c0->em.permille) return DSB_EINVAL;
	if (m->ctx.size() == 1) return dsb_ctx_abundance(c0, opts, out, summary);
	return multi_solve(m, o, out, summary, nullptr, 0);
}

extern "C" int dsb_multi_abundance_assign(dsb_multi *m, const dsb_em_opts *opts, dsb_ref_abundance *out, dsb_abundance_summary *summary, dsb_read_assign *reads,
                                          size_t cap, size_t *n)
{
	dsb_em_opts o;
	if (!m || !n || m->ctx.empty() || em_opts(opts, &o)) return DSB_EINVAL;
	dsb_ctx *c0 = m->ctx[0];
	for (dsb_ctx *c : m->ctx) if (!c->em.d_cnt || c->em.permille != c0->em.permille) return DSB_EINVAL;
	if (m->ctx.size() == 1) return dsb_ctx_abundance_assign(c0, opts, out, summary, reads, cap, n);
	std::vector<EmPiece> pc;
	for (dsb_ctx *c : m->ctx) pc.push_back({&c->em.log, 0});
	*n = (size_t)assign_count(pc);
	if (!reads) return DSB_OK;                                 // (count only)
	if (!out || !summary) return DSB_EINVAL;
	if (cap < *n) return DSB_ECAP;
	return multi_solve(m, o, out, summary, reads, *n);
}

extern "C" int dsb_multi_enable_lca(dsb_multi *m, int on, uint32_t min_permille)
{
	if (!m) return DSB_EINVAL;
	m->lca_on = m->lca_ok = false;
	int rc = multi_enable(m, [&](dsb_ctx *c, bool en) { return dsb_ctx_enable_lca(c, en ? on : 0, en ? min_permille : 0); });
	if (rc) return rc;
	m->lca_on = on != 0;
	return DSB_OK;
}
extern "C" int dsb_multi_lca(dsb_multi *m, const dsb_read_lca **out)
{
	if (!m || !out || !m->lca_on || !m->lca_ok) return DSB_EINVAL;
	*out = m->lca.data();
	return DSB_OK;
}

// The contexts' direct tables added into a table on the first context's device -- copied over (copy_to) where a context sits on
// another device -- then the roll-up of one context over the sum; the summary counters are added on the host.  The contexts' own
// tables are left as they are.  Integer sums: what one context would have counted.
extern "C" int dsb_multi_lca_counts(dsb_multi *m, dsb_taxon_count *out, size_t cap, size_t *n, dsb_lca_summary *summary)
{
	if (!m || !n || m->ctx.empty()) return DSB_EINVAL;
	dsb_ctx *c0 = m->ctx[0];
	for (dsb_ctx *c : m->ctx) if (!c->lca.d_direct || c->lca.permille != c0->lca.permille || c->taxa.tx != c0->taxa.tx) return DSB_EINVAL;
	if (m->ctx.size() == 1) return dsb_ctx_lca_counts(c0, out, cap, n, summary);
	unsigned long long tot[DSB_LCA_SUM] = {0, 0, 0, 0};
	bool remote = false;
	for (dsb_ctx *c : m->ctx) {
		unsigned long long s[DSB_LCA_SUM];
		if (int rc = lca_sums(c, s)) return rc;                // (waits for the context's stream: its table is final)
		for (int k = 0; k < DSB_LCA_SUM; k++) tot[k] += s[k];
		remote |= c->device != c0->device;
	}
	if (summary) { summary->reads = tot[0]; summary->classified = tot[1]; summary->no_taxon = tot[2]; summary->ambiguous = tot[3]; summary->min_permille = c0->lca.permille; summary->reserved = 0; }
	HIPCHK(hipSetDevice(c0->device));
	const size_t nt = (size_t)c0->taxa.tx->max_tid + 1;
	const hipStream_t st = c0->stream;
	DevScratch T;
	unsigned long long *acc = T.get<unsigned long long>(nt), *buf = remote ? T.get<unsigned long long>(nt) : nullptr;
	if (!acc || (remote && !buf)) return DSB_ENOMEM;
	EMCK(copy_to(acc, c0->device, c0->lca.d_direct, c0->device, nt * 8, st));
	const unsigned grid = (unsigned)std::min<size_t>((nt + 255) / 256, 8192);
	for (size_t i = 1; i < m->ctx.size(); i++) {
		const dsb_ctx *c = m->ctx[i];
		const unsigned long long *src = c->lca.d_direct;
		if (c->device != c0->device) { EMCK(copy_to(buf, c0->device, src, c->device, nt * 8, st)); src = buf; }
		hipLaunchKernelGGL(k_lca_add, dim3(grid), dim3(256), 0, st, acc, src, (uint64_t)nt);
	}
	EMCK(hipGetLastError());
	return lca_rollup(c0, acc, st, out, cap, n);
}
