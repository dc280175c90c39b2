// Per-hit edit distance and per-reference identity (dsb_ctx_enable_identity): the state a context keeps for it and the
// seam with the other run reductions (dsb_reductions.hip calls the three functions below from reductions_run, reductions_fetch and
// reductions_release).  The base-level alignment of the same records (dsb_ctx_enable_alignment) keeps its state here too.
// The kernels and the host side are in dsb_identity.hip.  Internal: the public surface is include/desamba_amd.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>
#include "../../include/desamba_amd.h"

// On exactly when d_tab is set.  d_rec: one record per entry of the hit buffer (grown with it); d_list: the batch's work list, {hit,
// read} per counted record; d_cnt: [0] listed records, [1] the work counter of k_hit_edits; d_arena: two generations of furthest-
// reaching points per wavefront of k_hit_edits' grid (stride ints each); d_tab: the run's table, one dsb_ref_identity per reference.
struct DsbIdent {
	dsb_hit_identity *d_rec = nullptr; size_t cap_rec = 0;
	uint2 *d_list = nullptr; size_t cap_list = 0;
	unsigned int *d_cnt = nullptr;
	int *d_arena = nullptr; uint32_t stride = 0, n_waves = 0;
	dsb_ref_identity *d_tab = nullptr;
	uint32_t band = 0, permille = 0;
	std::vector<dsb_hit_identity> h_rec;
	bool run = false, done = false;               // as DsbTaxa's
	// base-level alignment (dsb_ctx_enable_alignment): on exactly when d_trace is set, and only while identity is on
	// (identity_release frees both).  d_trace: trace_kib KiB per wavefront of the grid, the bit planes of k_hit_align's move codes;
	// d_aln: one record per entry of the hit buffer; d_ops: the batch's operation array (ops_room operations: ops_fixed, or sized
	// per batch); d_ops_used: the operations the batch's records reserved.  aln_run: the last batch ran with alignment on.
	// aln_mode (dsb_ctx_alignment_mode): k_hit_align, or k_hit_align_ck dividing the same trace place by the record's plan.
	uint64_t *d_trace = nullptr; uint32_t trace_kib = 0, aln_mode = DSB_ALN_MODE_FULL;
	dsb_hit_alignment *d_aln = nullptr; size_t cap_aln = 0;
	uint32_t *d_ops = nullptr; size_t cap_ops = 0; uint64_t ops_fixed = 0, ops_room = 0;
	unsigned long long *d_ops_used = nullptr;
	std::vector<dsb_hit_alignment> h_aln; std::vector<uint32_t> h_ops;
	bool aln_run = false;
};

struct dsb_ctx;
struct DsbBatchView;
int identity_run(dsb_ctx *c, const DsbBatchView &b);         // the three launches of a batch, on b.st
int identity_fetch_queue(dsb_ctx *c, size_t n_hits);         // queues the copy of the batch's records on c's stream (the caller waits)
void identity_release(dsb_ctx *c);
