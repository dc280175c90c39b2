// The host-side state of a classify context and of a dsb_multi, shared by the units that drive it: dsb_gpu.hip (upload, the
// classify launches, fetch) and dsb_reductions.hip (the run-wide taxa, coverage and abundance).  Internal: the public surface
// is include/desamba_amd.h.
#pragma once
#include <stdio.h>
#include <string.h>
#include <time.h>
#include <string>
#include "dsb_seed_scan.h"
#include "dsb_reductions.h"               // (and through it the HIP runtime, desamba_amd.h and dsb_device.h)

#define HIPCHK(e) do { hipError_t _e = (e); if (_e != hipSuccess) { fprintf(stderr, "[desamba_amd] HIP error %s at %s:%d\n", hipGetErrorString(_e), __FILE__, __LINE__); return DSB_ENODEV; } } while (0)

struct DsbStaged;                                 // the index staged in one device's HBM (dsb_gpu.hip)

// ---- a staged input batch ("input slot"): what dsb_batch_upload* leaves in HBM ------------------------------
struct InSlot {
	DsbReadDesc *d_rd = nullptr; char *d_ascii = nullptr; size_t cap_rd = 0, cap_ascii = 0;
	std::vector<DsbReadDesc> h_rd;
	size_t n_reads = 0; uint64_t n_words_total = 0, total_bases = 0, total_windows = 0, seed_entries = 0; uint32_t max_len = 0, min_len = 0;
	uint32_t *d_scan_order = nullptr; size_t cap_scan_order = 0;   // reads longest first (ragged batches only), for k_seed_scan
	bool ragged = false;
	uint64_t upload_bytes = 0;     // what the sequences of this batch took over PCIe
	bool packed = false;           // d_ascii holds 2-bit packed sequences (dsb_batch_upload's gather), not text
	bool ord_set = false; uint64_t ord_first = 0;   // dsb_ctx_set_batch_ordinal: read i of the staged batch has ordinal ord_first + i (taken by the slot's next run)
};

// pinned staging of dsb_batch_upload: one per gather thread, two chunks each (one is filled while the other is on its way)
struct UpStage { char *buf[2] = {nullptr, nullptr}; hipEvent_t ev[2] = {nullptr, nullptr}; bool used[2] = {false, false}; hipStream_t st = nullptr; };

// Diagnostic and tuning switches of the environment, read ONCE per context (dsb_ctx_create; dsb_ctx_reload_env for tests that
// change them on a living context): nothing on the per-batch path calls getenv.  -1 / 0 = not set.
struct DsbKnobs {
	bool upload_text = false;          // DSB_UPLOAD_TEXT: dsb_batch_upload gathers the sequences as text (round 3's form) instead of packing them
	bool debug = false, upload_trace = false, no_turn = false, no_group = false, heavy_first_set = false;
	long hout_cap = 0, sms_cap = 0, anc_cap_rt = 0, upload_chunk_kb = 0, step_limit_rt = 0, group_head = -1;
	int upload_threads = 0, seed_scan = -1, heavy_mw = -1, heavy_first = 0;
	bool heavy_preds_set = false; uint32_t heavy_preds = 0;
	uint64_t em_hash_mask = ~0ull;     // DSB_EM_HASH_BITS=1..64: k_em_collect keeps only the low bits of a set's hash (tests of the collision path)
	bool anchor_kernel = true; long anc_pool_rt = 0;   // DSB_ANCHOR_KERNEL=0: the anchor stage inside k_classify (no k_anchor); DSB_ANC_POOL_RT: anchors the pool holds (diagnostics)
	bool scan_look_set = false; DsbScanLook scan_look;   // DSB_SCAN_LOOK=after_seed,back_fwd,fwd_n,stride_n: k_seed_scan's look-ahead (experiments; default dsb_scan_look_for)
	std::string order_file;
};
inline bool g_upload_trace = false;           // (the buffer helpers below have no context at hand: DSB_UPLOAD_TRACE of the last knobs_read)

struct dsb_ctx {
	bool ek_dense = false;                         // filter tables more than ~4 % full (DsbStaged::ek_dense, or the synthetic tables' fill)
	DsbKnobs knobs;
	dsb_index *idx = nullptr; int device = 0; hipStream_t stream = nullptr;
	DsbStaged *staged = nullptr; DsbDevIndex dx;
	std::vector<InSlot> in; int cur = 0;          // input slots (dsb_ctx_select_slot); upload / run / fetch work on slot `cur`
	// per-run buffers (grown on demand to the largest staged batch)
	DsbWordDesc *d_wd = nullptr; uint8_t *d_bin = nullptr; uint64_t *d_pk = nullptr; uint64_t *d_bits = nullptr;
	size_t cap_wd = 0, cap_bin = 0, cap_pk = 0, cap_bits = 0;
	DsbReadOut *d_rout = nullptr; DsbHitOut *d_hout = nullptr; size_t cap_rout = 0, cap_hout = 0;
	DsbCounters *d_counters = nullptr;             // the batch's counter block (dsb_device.h)
	DsbSlotArena arena; int n_slots = 0, n_extra = 0;   // n_extra: slots behind the n_slots of the main launch, for the early launch of the heaviest reads (batches of >= 4096 reads)
	DsbSlotArena arena_big; int n_slots_big = 0;  // second run of reads that outgrew an arena or their loop budget
	DsbSlotArena arena_anc; int n_slots_anc = 0;  // k_anchor's slots (only the island walk's scratch)
	DsbAncRec *d_arec = nullptr; DsbAnchor *d_apool = nullptr; size_t cap_arec = 0, cap_apool = 0;   // k_anchor's per-read records and anchor pool
	uint32_t hint_len = 0;                           // the read length the caller announced (dsb_opts.max_read_len): arenas are never built for less
	unsigned mw_reads = 16; bool mw_grown = false; int mw_calm = 0;   // reads of the early launch that get eight wavefronts each: follows what the batches of this ctx show (stage_adapt_mw)
	uint32_t *d_score = nullptr, *d_order = nullptr, *d_heavy = nullptr; size_t cap_score = 0, cap_order = 0, cap_heavy = 0;
	DsbSeed *d_seeds = nullptr; DsbSeedInfo *d_sinfo = nullptr; size_t cap_seeds = 0, cap_sinfo = 0;   // seed lists of the batch (k_seed_scan)
	uint8_t *d_summ = nullptr; int summ_shift = 0;   // summary of exist table 0 in use (the staged index's, or none with synthetic tables)
	uint8_t *syn0 = nullptr, *syn1 = nullptr; bool seed_only = false;   // dsb_ctx_use_synthetic_filter
	bool bits_valid = false, seeds_valid = false;   // what the last run left on the device (stage dumps)
	unsigned n_early = 0;                          // reads of the last run that went through the early launch
	std::vector<DsbReadOut> h_rout; std::vector<DsbHitOut> h_hout;
	std::vector<dsb_read_result> res_reads;
	int hist_max = 0;
	hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr}; dsb_timing timing;
	hipStream_t stream3 = nullptr; hipEvent_t ev_heavy3 = nullptr;    // k_classify_heavy: several wavefronts on each of the very heaviest reads
	hipStream_t stream2 = nullptr; hipEvent_t ev_order = nullptr, ev_heavy = nullptr, ev_hprobe = nullptr, ev_cls = nullptr, ev_cls_wait = nullptr;   // the heaviest reads run beside the seed probe
	uint32_t *dbg_host = nullptr, *dbg_dev = nullptr;
	std::vector<UpStage> up; size_t up_chunk = 0;     // pinned staging of dsb_batch_upload (upload_gather)
	dsb_opts opts;
	DsbTaxa taxa; DsbCover cover; DsbEmStore em; DsbLca lca; DsbIdent ident;   // the run reductions (dsb_reductions.h, dsb_identity.h)
	dsb_ctx() { memset(&dx, 0, sizeof dx); memset(&arena, 0, sizeof arena); memset(&arena_big, 0, sizeof arena_big); memset(&arena_anc, 0, sizeof arena_anc); memset(&timing, 0, sizeof timing); memset(&opts, 0, sizeof opts); }
};

struct dsb_multi {
	dsb_index *idx = nullptr; std::vector<dsb_ctx *> ctx; uint32_t hist = 0;
	uint32_t chunk_reads_env = 0;                 // DSB_SHARD_CHUNK_READS, read when the contexts are made (tests: many small chunks)
	std::vector<uint32_t> last_calls;             // dsb_classify_batch calls each context made in the last dsb_multi_classify_batch
	std::vector<dsb_read_result> reads; std::vector<dsb_hit> hits;
	const dsb_taxonomy *tx = nullptr; std::vector<dsb_read_taxon> taxa; bool taxa_ok = false;   // dsb_multi_set_taxonomy / dsb_multi_taxa
	std::vector<dsb_read_lca> lca; bool lca_on = false, lca_ok = false;                          // dsb_multi_enable_lca / dsb_multi_lca
	std::vector<dsb_hit_identity> ident; bool ident_on = false, ident_ok = false;                // dsb_multi_enable_identity / dsb_multi_identity
	std::vector<dsb_hit_alignment> aln; std::vector<uint32_t> aln_ops; bool aln_on = false, aln_ok = false;   // dsb_multi_enable_alignment / dsb_multi_alignment
};

// a device buffer grown to hold at least `need` elements (its contents are not kept)
template <class T> static int grow(T **p, size_t *cap, size_t need)
{
	if (need <= *cap) return 0;
	// (an allocation on the per-batch path: hipFree / hipMalloc wait for the device and were seen to stall a sibling context's
	// batch for seconds -- the hints of dsb_ctx_create exist to keep this from happening; DSB_UPLOAD_TRACE shows each one)
	const bool tr = g_upload_trace; struct timespec t0, t1; if (tr) clock_gettime(CLOCK_MONOTONIC, &t0);
	const size_t old = *cap;
	if (*p) hipFree(*p);
	size_t n = need + need / 8 + 1024;
	if (hipMalloc((void **)p, n * sizeof(T)) != hipSuccess) { *p = nullptr; *cap = 0; return DSB_ENOMEM; }
	*cap = n;
	if (tr) { clock_gettime(CLOCK_MONOTONIC, &t1); fprintf(stderr, "[upload] a device buffer grew from %zu to %zu elements of %zu bytes (needed: %zu) in %.3f s\n", old, n, sizeof(T), need, (t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec)); }
	return 0;
}
