// The run reductions of classify: per-read taxa (dsb_ctx_set_taxonomy), per-reference and per-window coverage (dsb_ctx_enable_coverage,
// dsb_ctx_enable_coverage_windows), per-reference abundance by EM (dsb_ctx_enable_abundance) and per-read LCA classification
// (dsb_ctx_enable_lca); per-hit edit distance and per-reference identity (dsb_ctx_enable_identity) keeps its state
// and kernels in dsb_identity.h / dsb_identity.hip and is driven through the same seam.  Each reads a batch's hit buffer
// after its last classify launch, keeps state for the whole run and is merged across the contexts of a dsb_multi
// (dsb_reductions.hip).  Internal: the public surface is include/desamba_amd.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>
#include "../../include/desamba_amd.h"
#include "dsb_device.h"
#include "dsb_identity.h"

struct DsbEmSet;

// taxonomy: the parent table and each reference's taxid in HBM, one k_read_taxon launch per batch
struct DsbTaxa {
	const dsb_taxonomy *tx = nullptr; uint32_t *d_parent = nullptr, *d_ref_tid = nullptr;
	dsb_read_taxon *d_taxa = nullptr; size_t cap_taxa = 0; std::vector<dsb_read_taxon> h_taxa;
	bool run = false, done = false;               // k_read_taxon ran for the batch of the current slot / its records are fetched and completed
};

// coverage: a bitmap of one bit per reference base (each reference from a word boundary; off: the prefix sum of ceil(LN / 64),
// n_ref + 1 words), the lengths, and the four counters per reference; one k_ref_cover launch per batch.
// Windows (dsb_ctx_enable_coverage_windows; on exactly when win != 0): the window size, each reference's first
// window (d_first: the prefix sum of ceil(LN / win), n_ref + 1 words), {starts, aligned_bases} per window (d_win, 16 bytes each, one
// k_ref_windows launch per batch) and the covbases slot per window that a fetch fills (d_wcov)
struct DsbCover {
	uint64_t *d_bits = nullptr, *d_off = nullptr, *d_len = nullptr; dsb_ref_coverage *d_cov = nullptr; uint64_t words = 0;
	uint32_t win = 0; uint64_t n_win = 0, *d_first = nullptr, *d_win = nullptr, *d_wcov = nullptr;
};

// abundance: the run's candidate sets (DsbEmSet + their elements, grown geometrically between batches), the store's counters,
// and the reads the batches held; one k_em_collect launch per batch.  log: one entry per k_em_collect launch -- the
// batch's n records start at store position base, and record i is the read of ordinal first + i (dsb_ctx_set_batch_ordinal)
struct DsbEmLog { uint64_t base, first, n; };
struct DsbEmStore {
	DsbEmSet *d_sets = nullptr; uint32_t *d_elems = nullptr; unsigned long long *d_cnt = nullptr;
	size_t cap_sets = 0, cap_elems = 0, used_sets = 0, used_elems = 0; uint64_t reads = 0; uint32_t permille = 0;
	std::vector<DsbEmLog> log;
};

// LCA classification: a depth table beside DsbTaxa's parent table (u16, DSB_DEPTH_UNROOTED for an unrooted taxid), the
// batch's per-read records, and the run's counts -- direct[t] = reads whose LCA is t (max_tid + 1 u64), sum = {reads, classified,
// no_taxon, ambiguous}; clade is the roll-up's table, zeroed and filled by every dsb_ctx_lca_counts.  One k_read_lca and one
// k_lca_count launch per batch.  On exactly when d_direct is set.
struct DsbLca {
	uint16_t *d_depth = nullptr; unsigned long long *d_direct = nullptr, *d_clade = nullptr, *d_sum = nullptr;
	dsb_read_lca *d_rec = nullptr; size_t cap_rec = 0; std::vector<dsb_read_lca> h_rec;
	uint32_t permille = 0;
	bool run = false, done = false;               // as DsbTaxa's
};

// a batch's results on the device after its last classify launch (the second runs and the run after a regrown hit buffer included)
struct DsbBatchView {
	hipStream_t st;
	const DsbReadOut *rout; const DsbHitOut *hout; const DsbCounters *counters; size_t cap_hout;
	const DsbReadDesc *rd; uint32_t n;
	const uint64_t *pk;                           // both packed strands of every read (k_encode_pack), at rd[i].pk_off
	bool ord_set; uint64_t ord_first;             // dsb_ctx_set_batch_ordinal was called for this batch / with this ordinal
};

struct dsb_ctx;
// dsb_batch_run: the launches of the reductions that are on, on b.st
int reductions_run(dsb_ctx *c, const DsbBatchView &b);
// dsb_batch_fetch, once the copies of the batch's reads and hits are queued on c's stream: queues the copy of the batch's taxa and LCA records,
// waits for all of them (one synchronisation, skipped when nothing was queued) and gives the reads the device left to the host
// their taxon
int reductions_fetch(dsb_ctx *c, size_t n, bool queued);
// dsb_ctx_destroy
void reductions_release(dsb_ctx *c);
