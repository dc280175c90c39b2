// TEST INFRASTRUCTURE: stage a-12 (sdp_match in its five forms, gap_lane, sdp_middle_M2; dsb_classify_dev.h) called form by form
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

}  // namespace
