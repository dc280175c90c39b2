// TEST INFRASTRUCTURE: stage a-12 (sdp_match in its five forms, gap_lane, sdp_middle_M2, the sparse DP's predecessor scan; dsb_classify_dev.h) and, further down, the
// chain stages a-10, a-13, a-14 and a-17 (resolve_tree in every form, the tail of delete_small_score_rst, detect_primary, glibc_sort_chains) called form by form
// on cases that a test lays out in flat arrays, so that a test knows which code produced a node list.  One text for the three
// legs: tests/emu/emu_classify.cpp compiles it for the host (1 lane, or 64 lanes with the race detector), tests/stage/dsb_stage.hip
// for gfx950 (one wavefront per case).  Included after dsb_classify_dev.h; nothing here is part of libdesamba_amd.so.
//
// Layout of a case's inputs (tests/stage_lib.py builds them):
//   bin   byte strands of the reads, each [DSB_QPAD_L x 0][F][R][DSB_QPAD_R x DSB_QPAD_R_VAL]   (bin_off: the first pad byte)
//   pk    packed strands, (L + 31) / 32 + 1 words of F, then as many of R                       (pk_off: in words)
//   win   reference windows as bytes: >= DSB_REFWIN_FRONT bytes in front of t_str, behind t_len what the caller has there
//         followed by DSB_TPAD_VAL, 128 bytes in all                                            (win_off: t_str)
//   nodes one region of sms_cap + 4 DsbSms per case, filled with a pattern by the test          (node_off: in entries)
#pragma once

namespace DSB_NS {

enum { STAGE_WTAB = 0, STAGE_WTAB_PK = 1, STAGE_INV = 2, STAGE_N = 3, STAGE_N_PK = 4, STAGE_LDS = 5, STAGE_LDS_PK = 6, STAGE_FORMS = 7 };
enum { STAGE_KIND_MIDDLE = 0, STAGE_KIND_RIGHT = 1, STAGE_KIND_LEFT = 2 };

struct StageSdp {                 // one sdp_match call
	uint32_t L, strand, q_bg, q_ed, t_len, t_st, fwd, sms_cap, kind, pad0;
	uint64_t bin_off, pk_off, win_off, node_off;
	uint32_t rv, status, defined, pad1;     // out: what the form returned, w.status, whether the form is defined for the case
};
struct StageChain {               // gaps [g0, g1) for gap_lane, or the chain of anchors [a0, a0 + n_anc) ending at c_a for sdp_middle_M2
	uint32_t L, strand, g0, g1, a0, n_anc; int32_t c_a; uint32_t use_pk;
	uint64_t bin_off, pk_off, ref_off, ref_bases;                         // ref_off: bytes into the 2-bit text blob (one text per case, seq_offset 0)
	int32_t score; uint32_t status, pad0, pad1;                           // out
};
#define STAGE_MAX_ANC 400u
#define STAGE_CHAIN_SMS 4096u     /* match nodes of one gap (sdp_middle_M2's list is local to a gap) */
// the per-wavefront slice of global scratch: what classify_kernel_body takes from its arena slot and stage a-12 touches
#define STAGE_OFF_SORTKEY 0u                                         /* sdp_visit's bitmaps: 64 lanes x 64 words */
#define STAGE_OFF_SORTIDX (STAGE_OFF_SORTKEY + 16384u)
#define STAGE_OFF_ANC (STAGE_OFF_SORTIDX + 4096u)
#define STAGE_OFF_ANC_TMP (STAGE_OFF_ANC + 16384u)
#define STAGE_OFF_WIN (STAGE_OFF_ANC_TMP + 16384u)
#define STAGE_OFF_SMS (STAGE_OFF_WIN + 6656u)
#define STAGE_SLICE (STAGE_OFF_SMS + STAGE_CHAIN_SMS * 16u)
static_assert(STAGE_MAX_ANC * sizeof(DsbAnchor) <= 16384u && STAGE_MAX_ANC * sizeof(DsbGap) <= 16384u && STAGE_MAX_ANC * 4u <= 4096u, "slice: anchors, gaps, gap order");
static_assert(DSB_REFWIN_FRONT + 3u * DSB_REFWIN <= 6656u && (DSB_WTAB_MAXQ / 32u) * 64u * 4u <= 16384u, "slice: windows, bitmaps");

// the context as classify_kernel_body sets it up, as far as stage a-12 reads it (all lanes store the same values)
DV void stage_ctx(WCtxL &w, DSB_LDS_AS DsbDevIndex *sx, uint8_t *slice, uint32_t *wtab, uint4 *ring, uint32_t *red, uint32_t *cnt, const DsbRefInfo *refinfo)
{
	sx->refinfo = refinfo; sx->refbin = nullptr; sx->ref_bases = 0; sx->sms_cap = 0; sx->step_limit = DSB_STEP_LIMIT; sx->heavy_limit = 0;
	w.x = (DsbXP)sx; w.dbg = nullptr; w.mw = nullptr; w.n_waves = 1; w.wtab = wtab; w.ring = ring; w.red = red; w.k.c = (lds_u32 *)cnt; w.k.uni = 1;
	w.sortkey = (uint64_t *)(slice + STAGE_OFF_SORTKEY); w.sortidx = (uint32_t *)(slice + STAGE_OFF_SORTIDX);
	w.anc = (DsbAnchor *)(slice + STAGE_OFF_ANC); w.anc_tmp = (DsbAnchor *)(slice + STAGE_OFF_ANC_TMP);
	w.win_mid = slice + STAGE_OFF_WIN + DSB_REFWIN_FRONT; w.win_right = w.win_mid + DSB_REFWIN; w.win_left = w.win_right + DSB_REFWIN;
	w.sms = (DsbSms *)(slice + STAGE_OFF_SMS);
	w.step_limit = DSB_STEP_LIMIT; w.heavy_limit = 0; w.dp_preds = 0; w.boosted = 0; w.status = 0; w.steps = w.lsteps = 0; w.n_sms = 0; w.n_anc = 0; w.stage = 0;
	w.pre_seeds = nullptr; w.pre_info = nullptr; w.pk[0] = w.pk[1] = nullptr;
	wave_sync();
}
DV void stage_read(WCtxL &w, const uint8_t *bin, uint64_t bin_off, const uint64_t *pk, uint64_t pk_off, uint32_t L, bool use_pk)
{
	w.bin = const_cast<uint8_t *>(bin) + bin_off + DSB_QPAD_L; w.L = L; w.status = 0; w.steps = w.lsteps = 0; w.n_sms = 0; w.dp_preds = 0;
	w.pk[0] = use_pk ? pk + pk_off : nullptr; w.pk[1] = use_pk ? pk + pk_off + ((L + 31) / 32 + 1) : nullptr;
}

// forms (a) .. (e) on one case; mirror: 64 entries, the LDS mirror of the first nodes as sdp_match_lds left it
DN void stage_sdp(WCtxL &w, DSB_LDS_AS DsbDevIndex *sx, const int form, StageSdp *cs, const uint8_t *bin, const uint64_t *pk, const uint8_t *win, DsbSms *nodes, uint4 *mirror)
{
	const StageSdp c = *cs;
	const int lane = DSB_LANE;
	const uint32_t L = c.L, nw = (L + 31) / 32 + 1;
	const bool fwd = c.fwd != 0, with_pk = form == STAGE_WTAB_PK || form == STAGE_INV || form == STAGE_N_PK || form == STAGE_LDS_PK;
	wave_sync();
	stage_read(w, bin, c.bin_off, pk, c.pk_off, L, true);
	sx->sms_cap = c.sms_cap; w.sms = nodes + c.node_off;
	wave_sync();
	const uint8_t *q_str = w.bin + (c.strand == D_FORWARD ? 0u : L), *t_str = win + c.win_off;
	const uint64_t *qpk = with_pk ? pk + c.pk_off + (c.strand == D_FORWARD ? 0u : nw) : nullptr;
	uint32_t *const wtab = w.wtab;
	const uint32_t n_q = sdp_nq(L, c.q_bg, c.q_ed), t_kmer_num = c.t_len - 9 + 1;
	// what sdp_match_p checks before it builds a table: the window fits the table, there is something to look up
	const bool fits = n_q <= DSB_WTAB_MAXQ, runs = fits && n_q > 0 && t_kmer_num <= 0x7fffffffu && t_kmer_num > 4;
	uint32_t rv = 0, defined = 0;
	SdpArgsT<gp8> a; a.lnodes = nullptr; a.q_bg = c.q_bg; a.q_ed = c.q_ed; a.q_base = q_str; a.q_lo = 0; a.t_str = t_str; a.t_len = c.t_len; a.t_st = c.t_st;
	a.tab = (const lds_u32 *)wtab; a.bm = reinterpret_cast<uint32_t *>(w.sortkey) + lane; a.n_q = n_q;
	if (form == STAGE_N || form == STAGE_N_PK) {
		if (fits) { defined = 1; rv = sdp_match_n(w, 0, c.q_bg, c.q_ed, q_str, t_str, c.t_len, c.t_st, fwd, nullptr, qpk); }
	} else if (form == STAGE_WTAB || form == STAGE_WTAB_PK) {
		if (runs) {
			defined = 1;
			if (form == STAGE_WTAB_PK) wtab_build_pk((lds_u32 *)wtab, lane, qpk, nw, c.q_bg, n_q);
			else wtab_build<gp8>((lds_u32 *)wtab, lane, q_str + (int32_t)c.q_bg, 0u, n_q);
			rv = fwd ? sdp_match_t<true, gp8>(w, a, 0) : sdp_match_t<false, gp8>(w, a, 0);
		}
	} else if (form == STAGE_INV) {
		if (runs && n_q >= DSB_INV_MINQ && t_kmer_num <= 4 * DSB_INV_MAXPOS) {
			defined = 1;
			rv = fwd ? sdp_match_inv<true, gp8>(w, a, 0, qpk, nw) : sdp_match_inv<false, gp8>(w, a, 0, qpk, nw);
		}
	} else {
		// read and window staged in LDS behind the table, as sdp_middle_M2 stages them for a small gap
		const uint32_t slots = wtab_size(n_q);
		const int32_t q_lo = (int32_t)c.q_bg - 16, q_hi = (int32_t)c.q_ed + MAXV(80, (int32_t)c.t_len + 4);
		const uint32_t q_bytes = q_hi > q_lo ? (uint32_t)(q_hi - q_lo + 7) & ~7u : 0u, t_bytes = (c.t_len + 64 + 7) & ~7u;
		const uint32_t tbase = qpk ? MAXV(slots, (DSB_INV_WORDS + 3u) & ~3u) : slots;
		if (fwd && c.kind == STAGE_KIND_MIDDLE && fits && n_q > 0 && q_bytes && q_lo >= -(int32_t)DSB_QPAD_L + 8 && 4 * tbase + q_bytes + 8 + t_bytes + 8 + 1024 <= 4 * DSB_WTAB_SLOTS) {
			defined = 1;
			uint8_t *lq = reinterpret_cast<uint8_t *>(wtab + tbase), *lt = lq + q_bytes + 8;
			uint4 *lnodes = reinterpret_cast<uint4 *>(lt + t_bytes + (((4 * tbase + q_bytes + t_bytes) & 8u) ? 0 : 8));
			const int32_t q_last = (int32_t)((w.bin + 2 * (size_t)L + DSB_QPAD_R) - q_str) - 8;
			for (uint32_t k = 8 * lane; k < q_bytes; k += 8 * DSB_WAVE) *reinterpret_cast<uint64_t *>(lq + k) = ld_u64(q_str + MINV(q_lo + (int32_t)k, q_last));
			for (uint32_t k = (uint32_t)lane; k < c.t_len + 64; k += DSB_WAVE) lt[k] = k < c.t_len ? t_str[k] : (uint8_t)DSB_TPAD_VAL;
			wave_sync();
			rv = sdp_match_lds(w, 0, c.q_bg, c.q_ed, lq, q_lo, lt, c.t_len, c.t_st, lnodes, qpk);
			wave_sync();
			const uint32_t n = rv & 0x7fffffffu;
			for (uint32_t k = (uint32_t)lane; k < 64u && k < n; k += DSB_WAVE) mirror[k] = lnodes[k];
		}
	}
	wave_sync();
	if (lane == 0) { cs->rv = rv; cs->status = (uint32_t)w.status; cs->defined = defined; }
	wave_sync();
}

// form (f): gap_lane, one gap per lane as sdp_middle_M2 calls it
DN void stage_gap_lane(WCtxL &w, DSB_LDS_AS DsbDevIndex *sx, StageChain *cs, const uint8_t *bin, const uint64_t *pk, const uint8_t *ref, DsbGap *G)
{
	const StageChain c = *cs;
	wave_sync();
	stage_read(w, bin, c.bin_off, pk, c.pk_off, c.L, true);
	sx->refbin = ref + c.ref_off; sx->ref_bases = c.ref_bases; sx->sms_cap = STAGE_CHAIN_SMS;
	wave_sync();
	const uint64_t *qpk = w.pk[c.strand == D_FORWARD ? 0 : 1];
	for (uint32_t k = c.g0 + (uint32_t)DSB_LANE; k < c.g1; k += DSB_WAVE) G[k].gain = gap_lane(w, G[k], qpk, 0);
	wave_sync();
	if (DSB_LANE == 0) { cs->score = 0; cs->status = (uint32_t)w.status; }
	wave_sync();
}
// form (g): sdp_middle_M2 on a chain (anchors: rows of index_in_read, ref_offset, mtch_len, pre)
DN void stage_middle(WCtxL &w, DSB_LDS_AS DsbDevIndex *sx, StageChain *cs, const uint8_t *bin, const uint64_t *pk, const uint8_t *ref, const int32_t *anchors)
{
	const StageChain c = *cs;
	wave_sync();
	stage_read(w, bin, c.bin_off, pk, c.pk_off, c.L, c.use_pk != 0);
	sx->refbin = ref + c.ref_off; sx->ref_bases = c.ref_bases; sx->sms_cap = STAGE_CHAIN_SMS;
	int score = 0;
	if (c.n_anc <= STAGE_MAX_ANC) {
		for (uint32_t i = (uint32_t)DSB_LANE; i < c.n_anc; i += DSB_WAVE) {
			const int32_t *r = anchors + 4 * (size_t)(c.a0 + i);
			DsbAnchor an; an.mtch_len = (uint16_t)r[2]; an.score = 0; an.left_len = an.left_ED = an.rigt_len = an.rigt_ED = 0; an.direction = (uint8_t)c.strand; an.useless = an.duplicate = an.pad0 = 0;
			an.seed_ID = an.chain_id = 0; an.ref_ID = 0; an.ref_offset = (uint32_t)r[1]; an.index_in_read = (uint32_t)r[0]; an.pre = r[3]; an.global_offset = 0;
			w.anc[i] = an;
		}
		wave_sync();
		w.n_anc = c.n_anc;
		wave_sync();
		score = sdp_middle_M2(w, c.c_a, w.bin + (c.strand == D_FORWARD ? 0u : c.L), c.strand == D_FORWARD ? 0 : 1, 0);
	}
	wave_sync();
	if (DSB_LANE == 0) { cs->score = score; cs->status = c.n_anc <= STAGE_MAX_ANC ? (uint32_t)w.status : 0xffffffffu; }
	wave_sync();
}

// ---- the sparse DP of stage a-12 on a bare node list (tests/test_stage_dp.py): the predecessor scan in each of its restatements.  A case is a
// list of nodes (t_pos, q_pos, len) whose node 0 carries its score; a form scores every other node in place.
//   nodes   one region of n + STAGE_DP_GUARD DsbSms per case; the test fills the scores of nodes 1 .. and the guards with a pattern
//   sizes   block sizes of form (c) / batch sizes of form (d), taken in turn and cyclically ([s0, s0 + n_sizes); none: the callers' own)
enum { DP_PRED = 0, DP_BATCH = 1, DP_BLOCK = 2, DP_MW = 3 };
#define STAGE_DP_GUARD 4u
struct StageDp {
	uint32_t n, mode, form, waves;                    // mode 0 middle (form DP_PRED only), 1 right, 2 left; waves: wavefronts of form DP_MW
	uint32_t s0, n_sizes, heavy_limit, pad0;
	uint64_t node_off;
	uint32_t status, dp_preds, scored, defined;       // out: w.status, w.dp_preds, nodes scored before the form returned, whether the form is defined for the case
};
DV void stage_dp_begin(WCtxL &w, DSB_LDS_AS DsbDevIndex *sx, const StageDp &c, DsbSms *sms)
{
	wave_sync();
	w.sms = sms; w.n_sms = c.n; sx->sms_cap = c.n; w.status = 0; w.dp_preds = 0; w.steps = 0; w.heavy_limit = c.heavy_limit; w.boosted = 0; w.mw = nullptr; w.n_waves = 1;
	wave_sync();
}
// (a) sdp_best_pred node by node: modes 1 and 2 keep the ring as the node-by-node extensions do, mode 0 runs without it (sdp_middle_M2)
template <int MODE>
DV uint32_t stage_dp_pred(WCtxL &w, DsbSms *sms, const uint32_t n)
{
	if (MODE != 0 && n) { const DsbSms s0 = sms[0]; ring_put(w, 0, s0.t_pos, s0.q_pos, s0.len, s0.score); wave_sync(); }
	uint32_t cur = 1;
	for (; cur < n; cur++) {
		const DsbSms nd = sms[cur];
		const int sc = sdp_best_pred<MODE>(w, nd, (int32_t)cur);
		sms[cur].score = (uint32_t)sc;
		if (MODE != 0) { ring_put(w, cur, nd.t_pos, nd.q_pos, nd.len, (uint32_t)sc); wave_sync(); }
	}
	return n ? cur : 0;
}
// (b) sdp_best_pred_b on one wavefront, through node_get / NodeBlock and the ring, as sdp_right_M2_mw / sdp_left_M2_mw run it
template <int MODE>
DV uint32_t stage_dp_batch(WCtxL &w, DsbSms *sms, const uint32_t n)
{
	if (!n) return 0;
	{ const DsbSms s0 = sms[0]; ring_put(w, 0, s0.t_pos, s0.q_pos, s0.len, s0.score); }
	NodeBlock nb; nb.base = 0; nb.valid = 0;
	DpBatchL &db = *w.dpb; db.n0 = 0; db.K = 0;
	uint32_t bn0 = 0, bK = 0, cur = 1, steps = w.steps; const uint32_t step_limit = w.step_limit; uint4 *const ring = w.ring;
	wave_sync();
	while (cur < n) {
		if (++steps > step_limit) { w.status |= DSB_ST_TIMEOUT; break; }
		DsbSms *c_sms = sms + cur;
		const DsbSms nd = node_get(w, nb, cur); cur++;
		const int sc = sdp_best_pred_b<MODE>(w, db, nd, (int32_t)cur - 1, nb, n, ring, steps, bn0, bK);
		c_sms->score = (uint32_t)sc;
		{ uint4 r_; r_.x = nd.t_pos; r_.y = nd.q_pos; r_.z = nd.len; r_.w = (uint32_t)sc; ring_st(ring, (cur - 1) & (DSB_RING - 1), r_); }
	}
	w.steps = steps;
	return cur;
}
// (c) sdp_block_scores block by block, the scores written back between the blocks as ext_block does
template <int MODE>
DV uint32_t stage_dp_block(WCtxL &w, DsbSms *sms, const uint32_t n, const uint32_t *sizes, const uint32_t n_sizes)
{
	const int lane = DSB_LANE;
	uint32_t cur = 1, k = 0;
	while (cur < n) {
		uint32_t m = MINV((uint32_t)DSB_WAVE, n - cur);
		if (n_sizes) { m = MINV(m, MAXV(1u, sizes[k % n_sizes])); k++; }
		const bool mine = (uint32_t)lane < m;
		DsbSms nd; nd.t_pos = nd.q_pos = nd.len = nd.score = 0;
		if (mine) nd = sms[cur + lane];
		const int sc = sdp_block_scores<MODE>(w, cur, m, nd);
		if (mine) sms[cur + lane].score = (uint32_t)sc;
		wave_sync();                                                // (the scores: the next block's old predecessors)
		cur += m;
		if (w.status & DSB_ST_HEAVY) break;                         // ext_block spends the loop budget here: the extension stops at its next test
	}
	return n ? cur : 0;
}
DN void stage_dp(WCtxL &w, DSB_LDS_AS DsbDevIndex *sx, StageDp *cs, DsbSms *nodes, const uint32_t *sizes)
{
	const StageDp c = *cs;
	DsbSms *const sms = nodes + c.node_off;
	stage_dp_begin(w, sx, c, sms);
	uint32_t scored = 0, defined = 1;
	if (c.form == DP_PRED) scored = c.mode == 0 ? stage_dp_pred<0>(w, sms, c.n) : c.mode == 1 ? stage_dp_pred<1>(w, sms, c.n) : stage_dp_pred<2>(w, sms, c.n);
	else if (c.mode == 0) defined = 0;
	else if (c.form == DP_BATCH) scored = c.mode == 1 ? stage_dp_batch<1>(w, sms, c.n) : stage_dp_batch<2>(w, sms, c.n);
	else if (c.form == DP_BLOCK) scored = c.mode == 1 ? stage_dp_block<1>(w, sms, c.n, sizes + c.s0, c.n_sizes) : stage_dp_block<2>(w, sms, c.n, sizes + c.s0, c.n_sizes);
	else defined = 0;
	wave_sync();
	if (DSB_LANE == 0) { cs->status = (uint32_t)w.status; cs->dp_preds = w.dp_preds; cs->scored = scored; cs->defined = defined; }
	wave_sync();
}
static inline int stage_dp_check(const StageDp *cs, uint32_t n, size_t n_nodes, size_t n_sizes)
{
	for (uint32_t k = 0; k < n; k++) {
		const StageDp &c = cs[k];
		if (c.node_off + c.n + STAGE_DP_GUARD > n_nodes || (size_t)c.s0 + c.n_sizes > n_sizes || c.mode > 2 || c.form > DP_MW || c.n > 0x7fffff00u) return 1;
		if (c.form == DP_MW && (c.waves < 2 || c.waves > DSB_MW_MAXW)) return 1;
	}
	return 0;
}

// ---- the right / left extensions of stage a-12 on their own (tests/test_stage_ext.py): one sdp_right_M2 / sdp_left_M2, block-wise (through
// ext_block) or node by node (the _mw forms with w.mw == nullptr), on a read, a 2-bit text of two references, a chain list with its anchors.
//   chains  the chain list of a case, changed in place;  anchors: rows of 5 (index_in_read, ref_offset, mtch_len, pre, ref_ID)
//   nodes   one region of sms_cap + STAGE_DP_GUARD DsbSms per case, filled with a pattern;  sc: 256 + 2 n_chains + 8 DsbScHash per case
//   ris     DsbRefInfo of the case's references (ri_off: in entries)
struct StageExt {
	uint32_t L, strand, left, mw, c0, n_chains, chain_ID, a0, n_anc, sms_cap, heavy_limit, n_ref; int32_t score_ori; uint32_t pad0;
	uint64_t bin_off, pk_off, ref_off, ref_bases, node_off, sc_off, ri_off;
	int32_t score; uint32_t status, n_sms, defined;                     // out
};
DN void stage_ext(WCtxL &w, DSB_LDS_AS DsbDevIndex *sx, StageExt *cs, const uint8_t *bin, const uint64_t *pk, const uint8_t *ref, DsbChain *chains, const int32_t *anchors,
                  DsbSms *nodes, DsbScHash *scs, const DsbRefInfo *ris)
{
	const StageExt c = *cs;
	wave_sync();
	stage_read(w, bin, c.bin_off, pk, c.pk_off, c.L, true);
	sx->refbin = ref + c.ref_off; sx->ref_bases = c.ref_bases; sx->sms_cap = c.sms_cap; sx->refinfo = ris + c.ri_off;
	w.sms = nodes + c.node_off; w.hit = chains + c.c0; w.n_hit = c.n_chains; w.sc = scs + c.sc_off; w.heavy_limit = c.heavy_limit; w.boosted = 0; w.mw = nullptr; w.n_waves = 1;
	for (uint32_t i = (uint32_t)DSB_LANE; i < c.n_anc; i += DSB_WAVE) {
		const int32_t *r = anchors + 5 * (size_t)(c.a0 + i);
		DsbAnchor an; an.mtch_len = (uint16_t)r[2]; an.score = 0; an.left_len = an.left_ED = an.rigt_len = an.rigt_ED = 0; an.direction = (uint8_t)c.strand; an.useless = an.duplicate = an.pad0 = 0;
		an.seed_ID = an.chain_id = 0; an.ref_ID = (uint32_t)r[4]; an.ref_offset = (uint32_t)r[1]; an.index_in_read = (uint32_t)r[0]; an.pre = r[3]; an.global_offset = 0;
		w.anc[i] = an;
	}
	for (uint32_t k = (uint32_t)DSB_LANE; k < 256u; k += DSB_WAVE) { DsbScHash z; z.next = 0; z.seed_ID = 0; w.sc[k] = z; }
	wave_sync();
	w.n_anc = c.n_anc;
	wave_sync();
	DSB_SERIAL(w) sc_hash_idx(w.sc, w.hit, w.n_hit);
	serial_end(w);
	wave_sync();
	const uint8_t *q_str = w.bin + (c.strand == D_FORWARD ? 0u : c.L); const int tbl = c.strand == D_FORWARD ? 0 : 1;
	int score;
	if (!c.left) score = c.mw ? sdp_right_M2_mw(w, q_str, tbl, 0, w.hit, (int)c.chain_ID, c.L, w.sc, c.score_ori) : sdp_right_M2(w, q_str, tbl, 0, w.hit, (int)c.chain_ID, c.L, w.sc, c.score_ori);
	else score = c.mw ? sdp_left_M2_mw(w, q_str, tbl, 0, w.hit, (int)c.chain_ID, c.L, w.sc, c.score_ori) : sdp_left_M2(w, q_str, tbl, 0, w.hit, (int)c.chain_ID, c.L, w.sc, c.score_ori);
	wave_sync();
	if (DSB_LANE == 0) { cs->score = score; cs->status = (uint32_t)w.status; cs->n_sms = w.n_sms; cs->defined = 1; }
	wave_sync();
}
static inline int stage_ext_check(const StageExt *cs, uint32_t n, size_t n_chains, size_t n_rows, const int32_t *anchors, const DsbChain *chains, size_t n_nodes, size_t n_sc, size_t n_ri)
{
	for (uint32_t k = 0; k < n; k++) {
		const StageExt &c = cs[k];
		if ((size_t)c.c0 + c.n_chains > n_chains || c.chain_ID >= c.n_chains || c.n_chains > 16000 || (size_t)c.a0 + c.n_anc > n_rows || c.n_anc > STAGE_MAX_ANC) return 1;
		if (c.node_off + c.sms_cap + STAGE_DP_GUARD > n_nodes || c.sms_cap < 2 || c.sc_off + 256 + 2 * (size_t)c.n_chains + 8 > n_sc || c.ri_off + c.n_ref > n_ri || c.L < 9) return 1;
		for (uint32_t i = 0; i < c.n_anc; i++) { const int32_t *r = anchors + 5 * (size_t)(c.a0 + i); if (r[3] < -1 || r[3] >= (int32_t)i || (uint32_t)r[4] >= c.n_ref) return 1; }
		for (uint32_t i = 0; i < c.n_chains; i++) { const DsbChain &h = chains[c.c0 + i]; if (h.ref_ID >= c.n_ref || h.cur < -1 || (h.cur >= 0 && (uint32_t)h.cur >= c.n_anc)) return 1; }      // (cur: the last anchor of a chain that can be merged in, or -1)
	}
	return 0;
}

// ---- stages a-10 (resolve_tree), a-13 behind get_score_M2, a-14 (detect_primary), a-17 (glibc_sort_chains): tests/test_stage_chain.py,
// tests/test_stage_finish.py.  Inputs are arrays of anchors or chains; no read, no index.
//   rows    anchors, 8 u32 each: index_in_read, ref_ID, ref_offset, mtch_len, score, direction, useless, duplicate (pre = -1)
//   order   per anchor place: the input row that stands there afterwards;  pre: its predecessor link
//   hits    one region of hit_cap + STAGE2_GUARD DsbChain per case, filled with a pattern by the test: w.hit itself
//   raw     one region of hit_cap DsbChain per case: the chains as the DP left them, before chain_top_select
enum { RES_SORT_DISTINCT = 1, RES_SORT_TIE = 2, RES_SORT_MERGE = 3 };
enum { RES_DP_M2 = 1, RES_DP_LDS = 2, RES_DP_GLOBAL = 3, RES_DP_SERIAL = 4 };
enum { RES_SEL_RANK = 1, RES_SEL_GLIBC = 2 };
struct StageRes {                 // one resolve_tree; sort = dp = sel = 0: resolve_tree itself, else the forms named (sort: none for RES_DP_M2)
	uint32_t a0, n_anc, hit_cap, sort, dp, sel, pad0, pad1;
	uint64_t hit_off, raw_off;
	// out: chains before the selection (0xffffffff: resolve_tree itself, unknown) and after it, w.status, whether the forms are defined for
	// the case, and the forms resolve_tree's own tests lead to (nat_sort 0: no sort, fewer than 50 anchors; nat_sel 0: at most one chain)
	uint32_t n_raw, n_hit, status, defined, nat_sort, nat_dp, nat_sel, pad2;
};
struct StageFin {                 // which 0: the cut at the head of delete_small_score_rst, its part behind get_score_M2, detect_primary; 1 .. 3: glibc_sort_chains<which - 1>
	uint32_t c0, n, read_len, which; int32_t max_read_l, min_length, min_score, min_score_LV3;
	uint32_t n_cut, n_hit, status; int32_t max_read_l_out;        // out
};
#define STAGE2_MAX_ANC 3072u
#define STAGE2_MAX_HIT 3200u
#define STAGE2_GUARD 2u            /* guard chains behind a case's region */
// its own slice: both anchor arrays, both halves of the sort keys and indices, score_v, one reference window (detect_primary's bytes), hit_tmp
#define STAGE2_OFF_ANC 0u
#define STAGE2_OFF_ANC_TMP (STAGE2_OFF_ANC + STAGE2_MAX_ANC * 40u)
#define STAGE2_OFF_SORTKEY (STAGE2_OFF_ANC_TMP + STAGE2_MAX_ANC * 40u)
#define STAGE2_OFF_SORTIDX (STAGE2_OFF_SORTKEY + 2u * STAGE2_MAX_ANC * 8u)
#define STAGE2_OFF_SCOREV (STAGE2_OFF_SORTIDX + 2u * STAGE2_MAX_ANC * 4u)
#define STAGE2_OFF_WIN (STAGE2_OFF_SCOREV + 4096u)
#define STAGE2_OFF_HIT_TMP (STAGE2_OFF_WIN + 4096u)
#define STAGE2_SLICE (STAGE2_OFF_HIT_TMP + STAGE2_MAX_HIT * 48u)
static_assert(sizeof(DsbAnchor) == 40 && sizeof(DsbChain) == 48 && DSB_REFWIN_FRONT + DSB_REFWIN <= 4096u, "slice of the chain stages");

DV void stage2_ctx(WCtxL &w, uint8_t *slice)
{
	w.anc = (DsbAnchor *)(slice + STAGE2_OFF_ANC); w.anc_tmp = (DsbAnchor *)(slice + STAGE2_OFF_ANC_TMP);
	w.sortkey = (uint64_t *)(slice + STAGE2_OFF_SORTKEY); w.sortidx = (uint32_t *)(slice + STAGE2_OFF_SORTIDX);
	w.score_v = (int *)(slice + STAGE2_OFF_SCOREV); w.win_mid = slice + STAGE2_OFF_WIN + DSB_REFWIN_FRONT;
	w.hit_tmp = (DsbChain *)(slice + STAGE2_OFF_HIT_TMP);
	w.anc_cap = w.anc_cap_main = STAGE2_MAX_ANC; w.n_anc = 0; w.n_hit = 0; w.status = 0;
}
// a-10: the sort, the DP and the selection in the forms the case names, or resolve_tree as it is
DN void stage_resolve(WCtxL &w, StageRes *cs, const uint32_t *rows, uint32_t *order, int32_t *pre, DsbChain *hits, DsbChain *raw, uint8_t *slice)
{
	const StageRes c = *cs;
	const int lane = DSB_LANE; const uint32_t n = c.n_anc;
	wave_sync();
	stage2_ctx(w, slice);
	w.hit = hits + c.hit_off; w.hit_cap = c.hit_cap;
	wave_sync();
	uint32_t *const wtab = w.wtab;
	uint32_t defined = n <= STAGE2_MAX_ANC && c.hit_cap >= 1 && c.hit_cap <= STAGE2_MAX_HIT, n_raw = 0xffffffffu, nat_sort = 0, nat_dp = RES_DP_M2, nat_sel = 0;
	if (defined) {
		uint32_t max_ref = 0;
		for (uint32_t i = (uint32_t)lane; i < n; i += DSB_WAVE) {
			const uint32_t *r = rows + 8 * (size_t)(c.a0 + i);
			DsbAnchor an; an.mtch_len = (uint16_t)r[3]; an.score = (int16_t)r[4]; an.left_len = an.left_ED = an.rigt_len = an.rigt_ED = 0; an.direction = (uint8_t)r[5];
			an.useless = (uint8_t)r[6]; an.duplicate = (uint8_t)r[7]; an.pad0 = 0; an.seed_ID = an.chain_id = 0; an.ref_ID = r[1]; an.ref_offset = r[2]; an.index_in_read = r[0];
			an.pre = -1; an.global_offset = i;
			w.anc[i] = an; max_ref = MAXV(max_ref, r[1]);
		}
		max_ref = (uint32_t)grp_max_i((int)max_ref);
		wave_sync();
		w.n_anc = n;
		wave_sync();
		// resolve_tree's and chain_sort_M3's own tests, restated: what they lead to, not an observation of the path taken -- a change of the
		// product's thresholds shows in the results of the natural run, not in these words.  (nat_sel follows from the chains the DP leaves, so
		// only a forced run reports it; for resolve_tree itself the test takes it from the oracle's chain count.)
		if (n >= 50) {
			nat_sort = n <= DSB_RANKSORT_MAX ? (max_ref < (1u << 21) && n <= 1024 ? RES_SORT_DISTINCT : RES_SORT_TIE) : RES_SORT_MERGE;
			nat_dp = n <= DSB_CHAINDP_LDS ? RES_DP_LDS : RES_DP_GLOBAL;
		}
		if (!c.sort && !c.dp && !c.sel) resolve_tree(w);
		else {
			if (c.dp != RES_DP_M2) {
				if (c.sort == RES_SORT_DISTINCT) defined = n <= 1024 && max_ref < (1u << 21);
				if (c.sort == RES_SORT_TIE) defined = n <= DSB_WTAB_SLOTS / 2;
				if (c.dp == RES_DP_LDS) defined = defined && n <= DSB_CHAINDP_LDS;
			}
			if (defined) {
				if (c.dp != RES_DP_M2) { if (c.sort == RES_SORT_DISTINCT) chain_sort_M3<1>(w); else if (c.sort == RES_SORT_TIE) chain_sort_M3<2>(w); else chain_sort_M3<3>(w); }
				if (c.dp == RES_DP_LDS) { lds_w32 *L = (lds_w32 *)w.wtab; chain_stage_M3(w, L, DSB_CHAINDP_LDS); chain_dp_M3_wave(w, L, DSB_CHAINDP_LDS); chain_unstage_M3(w, L, DSB_CHAINDP_LDS); }
				else if (c.dp == RES_DP_GLOBAL) { uint32_t *L = reinterpret_cast<uint32_t *>(w.anc_tmp); chain_stage_M3(w, L, n); chain_dp_M3_wave(w, L, n); chain_unstage_M3(w, L, n); }
				else {
					DSB_SERIAL(w) {
						if (c.dp == RES_DP_M2) for (uint32_t i = 0; i < w.n_anc; i++) chain_insert_M2(w, i);
						else chain_dp_M3(w);
					}
					serial_end(w);
				}
				n_raw = w.n_hit;
				for (uint32_t i = (uint32_t)lane; i < n_raw; i += DSB_WAVE) raw[c.raw_off + i] = w.hit[i];
				wave_sync();
				nat_sel = n_raw <= 1 ? 0 : n_raw > DSB_WTAB_SLOTS / 2 ? RES_SEL_GLIBC : RES_SEL_RANK;
				if (c.sel == RES_SEL_GLIBC) { w.wtab = nullptr; wave_sync(); chain_top_select(w); w.wtab = wtab; wave_sync(); }
				else if (n_raw <= DSB_WTAB_SLOTS / 2) chain_top_select(w);
				else defined = 0;
			}
		}
		wave_sync();
		if (defined) for (uint32_t i = (uint32_t)lane; i < n; i += DSB_WAVE) { order[c.a0 + i] = (uint32_t)w.anc[i].global_offset; pre[c.a0 + i] = w.anc[i].pre; }
	}
	wave_sync();
	if (lane == 0) { cs->n_raw = n_raw; cs->n_hit = w.n_hit; cs->status = (uint32_t)w.status; cs->defined = defined; cs->nat_sort = nat_sort; cs->nat_dp = nat_dp; cs->nat_sel = nat_sel; }
	wave_sync();
}
// The part of delete_small_score_rst behind get_score_M2 (dsb_classify_dev.h, src/cly.c:2921-2993) is not callable on its own: the same
// statements in the same order, replayed here -- glibc_sort_chains<1>, absorb and merge, the three filters, glibc_sort_chains<2>, the cut.
// (Moving them into a function of the product changed the compiler's resource report of the k_classify kernels, see DESIGN.md.)
DV void stage_small_score_tail(WCtxL &w, uint32_t l_read)
{
	DsbXP x = w.x;
	DsbChain *st_c = w.hit, *ed_c = st_c + w.n_hit, *c_c;
	if (w.n_hit > 1) glibc_sort_chains<1>(w, w.n_hit);
	for (c_c = st_c; c_c < ed_c - 1; c_c++) {
		if (c_c->sum_score == 0) continue;
		DsbChain *nx = c_c + 1;
		for (; nx < ed_c; nx++) {
			if (c_c->ref_ID == nx->ref_ID) {
				if (c_c->direction != nx->direction) continue;
				if (nx->sum_score == 0) continue;
				if (nx->t_st < c_c->t_st + 5 && nx->q_st < c_c->q_st + 5 && nx->sum_score < c_c->sum_score + 5) {
					nx->sum_score = 0; nx->q_ed = nx->q_st; nx->t_ed = nx->t_st;
					continue;
				}
				int dis_t = nx->t_st - c_c->t_ed, dis_q = nx->q_st - c_c->q_ed;
				int dis_t_q = ABSV(dis_t - dis_q);
				if ((dis_t > -20 && dis_t < 1000 && dis_q > -20 && dis_q < 1000) && dis_t_q < 200) {
					c_c->t_ed = MAXV(c_c->t_ed, nx->t_ed); c_c->q_ed = MAXV(c_c->q_ed, nx->q_ed);
					c_c->sum_score += nx->sum_score;
					nx->sum_score = 0; nx->q_ed = nx->q_st; nx->t_ed = nx->t_st;
				}
			} else break;
		}
	}
	w.max_read_l = MAXV((uint32_t)w.max_read_l, l_read);
	if (w.max_read_l < 510) {
		for (c_c = st_c; c_c < ed_c; c_c++) { int s = c_c->sum_score + ((c_c->q_ed - c_c->q_st) >> 5); if (s < 26) c_c->sum_score = 0; }
	} else if (l_read < 310) {
		for (c_c = st_c; c_c < ed_c; c_c++) { int s = c_c->sum_score + ((c_c->q_ed - c_c->q_st) >> 5); if (s < 30) c_c->sum_score = 0; }
	} else {
		for (c_c = st_c; c_c < ed_c; c_c++) {
			int s = c_c->sum_score + ((c_c->q_ed - c_c->q_st) >> 5);
			if (s < (x->filter_min_score_LV3) && (c_c->q_ed - c_c->q_st < (uint32_t)x->filter_min_length || s < x->filter_min_score)) c_c->sum_score = 0;
		}
	}
	if (w.n_hit > 1) glibc_sort_chains<2>(w, w.n_hit);
	for (c_c = st_c; c_c < ed_c; c_c++) if (c_c->sum_score == 0) break;
	w.n_hit = c_c - st_c;
}
// a-13 / a-14 / a-17 on the chains [c0, c0 + n) of `chains` (in place); tail: the same places, the chains as the tail of delete_small_score_rst left them
DN void stage_finish(WCtxL &w, DSB_LDS_AS DsbDevIndex *sx, StageFin *cs, DsbChain *chains, DsbChain *tail, uint8_t *slice)
{
	const StageFin c = *cs;
	const int lane = DSB_LANE;
	wave_sync();
	stage2_ctx(w, slice);
	w.hit = chains + c.c0; w.hit_cap = c.n; w.n_hit = c.n; w.max_read_l = c.max_read_l;
	sx->filter_min_length = c.min_length; sx->filter_min_score = c.min_score; sx->filter_min_score_LV3 = c.min_score_LV3;
	wave_sync();
	uint32_t n_cut = c.n;
	if (c.n > STAGE2_MAX_HIT) n_cut = 0;
	else if (c.which) {
		DSB_SERIAL(w) { if (c.which == 1) glibc_sort_chains<0>(w, c.n); else if (c.which == 2) glibc_sort_chains<1>(w, c.n); else glibc_sort_chains<2>(w, c.n); }
		serial_end(w);
	} else {
		if (w.n_hit != 0) {
			// delete_small_score_rst without its extensions: the product's own cut at its head, then its part behind get_score_M2 replayed (stage_small_score_tail)
			DSB_SERIAL(w) small_score_head_cut(w);
			serial_end(w);
			n_cut = w.n_hit;
			DSB_SERIAL(w) stage_small_score_tail(w, c.read_len);
			serial_end(w);
		}
		for (uint32_t i = (uint32_t)lane; i < n_cut; i += DSB_WAVE) tail[c.c0 + i] = w.hit[i];
		wave_sync();
		DSB_SERIAL(w) detect_primary(w, c.read_len);
		serial_end(w);
	}
	wave_sync();
	if (lane == 0) { cs->n_cut = n_cut; cs->n_hit = w.n_hit; cs->status = c.n > STAGE2_MAX_HIT ? 0xffffffffu : (uint32_t)w.status; cs->max_read_l_out = w.max_read_l; }
	wave_sync();
}
// what the host entries refuse before a case reaches the device code: regions outside the arrays, scores outside the domain (a group
// without a positive score has no best anchor, in the reference as here)
static inline int stage_resolve_check(const StageRes *cs, uint32_t n, const uint32_t *rows, size_t n_rows, size_t n_hits, size_t n_raw)
{
	for (uint32_t k = 0; k < n; k++) {
		const StageRes &c = cs[k];
		if ((size_t)c.a0 + c.n_anc > n_rows || c.hit_off + c.hit_cap + STAGE2_GUARD > n_hits || c.raw_off + c.hit_cap > n_raw) return 1;
		for (uint32_t i = 0; i < c.n_anc; i++) { const uint32_t *r = rows + 8 * (size_t)(c.a0 + i); if (r[4] < 1 || r[4] > 32767 || r[3] > 65535 || r[5] > 1) return 1; }
	}
	return 0;
}
static inline int stage_finish_check(const StageFin *cs, uint32_t n, size_t n_chains)
{
	for (uint32_t k = 0; k < n; k++) if ((size_t)cs[k].c0 + cs[k].n > n_chains || cs[k].which > 3) return 1;
	return 0;
}

// ---- the anchor stage a-4 .. a-8 (tests/test_stage_anchor.py): the FM search, fast_island, fast_classify, fast_classify_lane and slow_classify, called
// as they are on a read's byte strands, its seed lists and a loaded index.
//   dx      the index descriptor (host pointers in the emulation, device pointers on the GPU): copied to the LDS descriptor before each case
//   seeds   per read (L >> 1) + 64 DsbSeed: the forward strand's list at seed_off, the reverse strand's at seed_off + (L >> 2) (the product's layout)
//   anchors one region of anc_cap + STAGE3_GUARD DsbAnchor per case, filled with a pattern by the test: w.anc itself (ANC_LANE: the lane's scratch, copied)
//   calls   form ANC_MEM: rows of 4 (string_index, max_rst, l_min, l_max), the searches of one walk in its order: the visited-row set carries over
//   mems    form ANC_MEM: per call a row of STAGE3_MEM int64 in the layout of the oracle's trace: [5] MEMs found, [8 + 4 i ..] sp, match_len, sa_sp, sa_sp_l
enum { ANC_MEM = 0, ANC_ISLAND = 1, ANC_FAST = 2, ANC_LANE = 3, ANC_SLOW = 4, ANC_WHOLE = 5 };
#define STAGE3_GUARD 4u
#define STAGE3_MEM 40u
#define STAGE3_MAX_SEEDS 16384u    /* entries of the island lists of a slice: reads of up to 2 * (16384 - 64) bases */
struct StageAnc {
	uint32_t L, form, strand, anc_cap, step_limit, sp_gen, q0, n_q;       // q0, n_q: ANC_MEM the calls [q0, q0 + n_q); ANC_ISLAND q0 = the seed's index
	uint32_t n_seed[2], total[2];                                         // [0] forward strand, [1] reverse strand
	uint64_t bin_off, seed_off, anc_off, mem_off;
	uint32_t n_anc, status, flag, lsteps, steps, sp_gen_out, defined, pad1;   // out; flag: fast_island's return value, fast_classify_lane's ovf
};
// its own slice: the visited-row sets (zeroed by the host entries once, as the kernels zero theirs once per launch), the lane scratch, the island
// lists, fast_classify's order (w.sortidx), slow_classify's MEM list
#define STAGE3_OFF_SPSET 0u
#define STAGE3_OFF_LANE_SP (STAGE3_OFF_SPSET + DSB_SPHASH * 8u)
#define STAGE3_OFF_LANE_ANC (STAGE3_OFF_LANE_SP + 64u * DSB_SPHASH * 8u)
#define STAGE3_OFF_TOP (STAGE3_OFF_LANE_ANC + 64u * DSB_LANE_ANC_CAP * 40u)
#define STAGE3_OFF_ROUND (STAGE3_OFF_TOP + STAGE3_MAX_SEEDS * 4u)
#define STAGE3_OFF_ORD (STAGE3_OFF_ROUND + STAGE3_MAX_SEEDS * 4u)
#define STAGE3_OFF_MEM (STAGE3_OFF_ORD + STAGE3_MAX_SEEDS * 4u)
#define STAGE3_SLICE (STAGE3_OFF_MEM + ((DSB_MEMSLOW_CAP * 32u + 255u) & ~255u))
static_assert(sizeof(DsbMem) == 32 && sizeof(DsbAnchor) == 40 && sizeof(DsbSeed) == 8, "slice of the anchor stage");

DV void stage3_ctx(WCtxL &w, DSB_LDS_AS DsbDevIndex *sx, const DsbDevIndex *dx, uint8_t *slice, const StageAnc &c, DsbAnchor *anchors)
{
	wave_sync();
	for (uint32_t i = (uint32_t)DSB_LANE; i < sizeof(DsbDevIndex) / 4u; i += DSB_WAVE) reinterpret_cast<DSB_LDS_AS uint32_t *>(sx)[i] = reinterpret_cast<const uint32_t *>(dx)[i];
	wave_sync();
	sx->step_limit = c.step_limit; sx->heavy_limit = 0;
	w.spset = (uint64_t *)(slice + STAGE3_OFF_SPSET); w.lane_spset = (uint64_t *)(slice + STAGE3_OFF_LANE_SP); w.lane_anc = (DsbAnchor *)(slice + STAGE3_OFF_LANE_ANC);
	w.top_idx = (uint32_t *)(slice + STAGE3_OFF_TOP); w.round_info = (uint32_t *)(slice + STAGE3_OFF_ROUND); w.sortidx = (uint32_t *)(slice + STAGE3_OFF_ORD);
	w.mem_slow = (DsbMem *)(slice + STAGE3_OFF_MEM);
	// (a case starts with empty sets whatever generation it starts at: the case before it on this slice may have used the same generations; the lanes' own
	// sets are used by the lane-parallel forms only)
	for (uint32_t i = (uint32_t)DSB_LANE; i < DSB_SPHASH; i += DSB_WAVE) w.spset[i] = 0;
	if (c.form == ANC_FAST || c.form == ANC_WHOLE || c.form == ANC_LANE) for (uint32_t i = (uint32_t)DSB_LANE; i < (uint32_t)DSB_WAVE * DSB_SPHASH; i += DSB_WAVE) w.lane_spset[i] = 0;
	w.anc = anchors + c.anc_off; w.anc_cap = w.anc_cap_main = c.anc_cap; w.n_anc = 0; w.status = 0; w.steps = w.lsteps = 0; w.step_limit = c.step_limit; w.sp_gen = c.sp_gen;
	w.k.uni = 1;
	wave_sync();
}
// forms (a), (b), (c), (e) and the whole read on one case
DN void stage_anchor(WCtxL &w, DSB_LDS_AS DsbDevIndex *sx, const DsbDevIndex *dx, StageAnc *cs, const uint8_t *bin, DsbSeed *seeds, DsbAnchor *anchors, const int32_t *calls, int64_t *mems, uint8_t *slice)
{
	const StageAnc c = *cs;
	const int lane = DSB_LANE;
	stage3_ctx(w, sx, dx, slice, c, anchors);
	w.bin = const_cast<uint8_t *>(bin) + c.bin_off + DSB_QPAD_L; w.L = c.L;
	DsbXP x = w.x;
	DsbSeed *const svF = seeds + c.seed_off, *const svR = svF + (c.L >> 2);
	uint8_t *const binF = w.bin, *const binR = w.bin + c.L;
	const bool fwd = c.strand == D_FORWARD;
	SDirL *sd = w.sd;
	uint32_t flag = 0, defined = 1;
	if (c.L < 40) defined = c.form == ANC_WHOLE;                             // (classify_read returns before the anchor stage)
	else if (c.form == ANC_MEM) {
		LCtx l = lctx_main(w);
		SpSet sp_set = {l.spset, 0, DSB_SPSET_CAP, l.sp_gen};
		sp_set_reset(sp_set);
		const uint8_t *bin_read = fwd ? binF : binR;
		for (uint32_t q = 0; q < c.n_q; q++) {
			const int32_t *r = calls + 4 * (size_t)(c.q0 + q);
			DsbMem mem[8];
			const int n = bwt_MEM_search(x, l.k, bin_read + r[0], prefix13(bin_read, r[0]), r[1], r[2], r[3], sp_set, mem);
			wave_sync();
			if (lane == 0) {
				int64_t *o = mems + STAGE3_MEM * (c.mem_off + q);
				o[5] = n;
				for (int i = 0; i < n && i < 8; i++) { o[8 + 4 * i] = (int64_t)mem[i].sp; o[9 + 4 * i] = mem[i].match_len; o[10 + 4 * i] = (int64_t)mem[i].sa_sp; o[11 + 4 * i] = mem[i].sa_sp_l; }
			}
		}
		l.sp_gen = sp_set.gen; lctx_done(w, l);
	} else if (c.form == ANC_ISLAND) {
		// the redo form of fast_classify's commit: the whole wavefront walks one island straight into the main array
		const SDirV s_d = {fwd ? svF : svR, fwd ? binF : binR, c.strand};
		LCtx l = lctx_main(w); l.anc_cap = w.anc_cap_main;
		flag = (uint32_t)fast_island(x, l, s_d, c.L, c.q0);
		lctx_done(w, l);
	} else if (c.form == ANC_FAST || c.form == ANC_SLOW) {
		sdir_set(sd, fwd ? svF : svR, c.n_seed[fwd ? 0 : 1], fwd ? binF : binR, nullptr, c.strand, c.total[fwd ? 0 : 1]);
		wave_sync();
		if (c.form == ANC_FAST) fast_classify(w, sd, c.L); else slow_classify(w, sd, c.L);
	} else if (c.form == ANC_WHOLE) {
		// RESTATED, not called: the strand swap and the both-direction rule of classify_read and k_anchor (dsb_gpu.hip) around fast_classify; a change
		// of theirs shows in the whole-read tests, not here
		sdir_set(sd, svF, c.n_seed[0], binF, nullptr, D_FORWARD, c.total[0]);
		sdir_set(sd + 1, svR, c.n_seed[1], binR, nullptr, D_REVERSE, c.total[1]);
		wave_sync();
		if (sd[0].total_score < sd[1].total_score) sdir_swap(sd, sd + 1);
		wave_sync();
		const bool both_direction = ((sd[0].total_score - sd[1].total_score) <= (sd[0].total_score >> 3));
		fast_classify(w, sd, c.L);
		if (both_direction) fast_classify(w, sd + 1, c.L);
	} else defined = 0;
	wave_sync();
	if (lane == 0) { cs->n_anc = w.n_anc; cs->status = (uint32_t)w.status; cs->flag = flag; cs->lsteps = w.lsteps; cs->steps = w.steps; cs->sp_gen_out = w.sp_gen; cs->defined = defined; }
	wave_sync();
}
// form (d): fast_classify_lane, one read per lane: the cases [k0, k0 + DSB_WAVE) of the list, each lane's anchors copied from its scratch to its case's region
DN void stage_anchor_lane(WCtxL &w, DSB_LDS_AS DsbDevIndex *sx, const DsbDevIndex *dx, StageAnc *cases, uint32_t k0, uint32_t n, const uint8_t *bin, DsbSeed *seeds, DsbAnchor *anchors, uint8_t *slice)
{
	const int lane = DSB_LANE;
	const bool valid = k0 + (uint32_t)lane < n;
	StageAnc c = cases[valid ? k0 + (uint32_t)lane : k0];
	{ StageAnc c0 = cases[k0]; c0.anc_off = 0; stage3_ctx(w, sx, dx, slice, c0, anchors); }     // (wave-uniform: the first case's budget and generation)
	DsbSeedInfo si; si.n_seed[0] = c.n_seed[0]; si.n_seed[1] = c.n_seed[1]; si.total[0] = c.total[0]; si.total[1] = c.total[1]; si.flags = 0; si.pad = 0;
	uint32_t na = 0, ovf = 0;
	fast_classify_lane(w, valid, const_cast<uint8_t *>(bin) + c.bin_off + DSB_QPAD_L, c.L, seeds + c.seed_off, &si, &na, &ovf);
	if (valid) {
		const DsbAnchor *src = w.lane_anc + (size_t)lane * DSB_LANE_ANC_CAP;
		DsbAnchor *dst = anchors + c.anc_off;
		for (uint32_t i = 0; i < na && i < c.anc_cap; i++) dst[i] = src[i];
		StageAnc *o = cases + k0 + lane;
		o->n_anc = na; o->flag = ovf; o->status = 0; o->defined = c.anc_cap >= DSB_LANE_ANC_CAP; o->sp_gen_out = w.sp_gen; o->lsteps = 0; o->steps = 0;
	}
	wave_sync();
}
static inline int stage_anchor_check(const StageAnc *cs, uint32_t n, size_t bin_bytes, size_t n_seeds, size_t n_anchors, const int32_t *calls, size_t n_calls, size_t n_mems, const DsbSeed *seeds, int ek_len)
{
	for (uint32_t k = 0; k < n; k++) {
		const StageAnc &c = cs[k];
		if (c.form > ANC_WHOLE || c.strand > 1 || c.bin_off + DSB_QPAD_L + 2 * (size_t)c.L + DSB_QPAD_R > bin_bytes || c.seed_off + (c.L >> 1) + 64 > n_seeds) return 1;
		if ((c.L >> 1) + 64 > STAGE3_MAX_SEEDS || c.n_seed[0] > (c.L >> 2) || c.n_seed[1] > (c.L >> 2) + 64 || c.anc_cap < 1 || c.anc_off + c.anc_cap + STAGE3_GUARD > n_anchors) return 1;
		if (c.form == ANC_LANE && c.anc_cap < DSB_LANE_ANC_CAP) return 1;
		if (c.L < 40) continue;
		for (int s = 0; s < 2; s++)                                          // every window of a seed lies in the read
			for (uint32_t i = 0; i < c.n_seed[s]; i++) { const DsbSeed &v = seeds[c.seed_off + (s ? (c.L >> 2) : 0) + i]; if (v.len < 1 || v.len > 61 || (size_t)v.offset + v.len + (size_t)ek_len - 1 > c.L) return 1; }
		if (c.form == ANC_ISLAND && c.q0 >= c.n_seed[c.strand == D_FORWARD ? 0 : 1]) return 1;
		if (c.form == ANC_MEM) {
			if ((size_t)c.q0 + c.n_q > n_calls || c.mem_off + c.n_q > n_mems) return 1;
			for (uint32_t q = 0; q < c.n_q; q++) { const int32_t *r = calls + 4 * (size_t)(c.q0 + q); if (r[0] < 12 || (uint32_t)r[0] >= c.L || r[1] < 1 || r[1] > 8 || r[3] != r[0]) return 1; }
		}
	}
	return 0;
}

}  // namespace
