// TEST INFRASTRUCTURE: stage a-12 of the device code (dsb_classify_dev.h: sdp_match in its five forms, gap_lane, sdp_middle_M2) and the
// chain stages a-10, a-13, a-14 and a-17 (resolve_tree in every form, the tail of delete_small_score_rst, detect_primary, glibc_sort_chains) on
// the GPU, form by form, with the real wavefront primitives of dsb_wave.h (tests/stage/dsb_stage_forms.h holds the forms; the
// host emulation runs the same text).  One wavefront per workgroup (k_stage_dp_mw: 2, 4 or 8), one workgroup per case; the context is set up as
// classify_kernel_body (dsb_gpu.hip) sets it up.  Built into tests/stage/libdsbstage.so; nothing of it is in libdesamba_amd.so.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "dsb_device.h"
#define DSB_GROUP 64
#define DSB_NS dsb_stage
#include "dsb_classify_dev.h"
#include "dsb_stage_forms.h"
#undef DSB_GROUP
using namespace dsb_stage;

#define STAGE_GRID 1024u      /* workgroups (and scratch slices) per launch */

// (a macro, not a function: the arrays must be the kernel's own __shared__ objects)
#define STAGE_KERNEL_CTX                                                                                           \
	__shared__ DsbDevIndex sx;                                                                                     \
	__shared__ uint4 lds_ring[DSB_RING];                                                                           \
	__shared__ __attribute__((aligned(16))) uint32_t lds_wtab[DSB_WTAB_SLOTS];                                     \
	__shared__ uint32_t lds_red[2];                                                                                \
	__shared__ uint32_t lds_cnt[4];                                                                                \
	__shared__ DpBatch lds_dpb;                                                                                    \
	__shared__ WCtx s_w;                                                                                           \
	WCtxL &w = *(WCtxL *)&s_w;                                                                                     \
	if (threadIdx.x < 4) lds_cnt[threadIdx.x] = 0;                                                                 \
	__syncthreads();                                                                                               \
	w.dpb = (DpBatchL *)&lds_dpb;                                                                                  \
	stage_ctx(w, (DSB_LDS_AS DsbDevIndex *)&sx, slices + (size_t)blockIdx.x * STAGE_SLICE, lds_wtab, lds_ring, lds_red, lds_cnt, refinfo);   \
	__syncthreads();

__global__ void __launch_bounds__(64) k_stage_sdp(int form, StageSdp *cases, uint32_t base, uint32_t n, const uint8_t *bin, const uint64_t *pk, const uint8_t *win,
                                                  DsbSms *nodes, uint4 *mirror, uint8_t *slices, const DsbRefInfo *refinfo)
{
	const uint32_t k = base + blockIdx.x;
	if (k >= n) return;
	STAGE_KERNEL_CTX
	stage_sdp(w, (DSB_LDS_AS DsbDevIndex *)&sx, form, cases + k, bin, pk, win, nodes, mirror + 64 * (size_t)k);
}
__global__ void __launch_bounds__(64) k_stage_gap_lane(StageChain *cases, uint32_t base, uint32_t n, const uint8_t *bin, const uint64_t *pk, const uint8_t *ref, DsbGap *G,
                                                       uint8_t *slices, const DsbRefInfo *refinfo)
{
	const uint32_t k = base + blockIdx.x;
	if (k >= n) return;
	STAGE_KERNEL_CTX
	stage_gap_lane(w, (DSB_LDS_AS DsbDevIndex *)&sx, cases + k, bin, pk, ref, G);
}
__global__ void __launch_bounds__(64) k_stage_middle(StageChain *cases, uint32_t base, uint32_t n, const uint8_t *bin, const uint64_t *pk, const uint8_t *ref, const int32_t *anchors,
                                                     uint8_t *slices, const DsbRefInfo *refinfo)
{
	const uint32_t k = base + blockIdx.x;
	if (k >= n) return;
	STAGE_KERNEL_CTX
	stage_middle(w, (DSB_LDS_AS DsbDevIndex *)&sx, cases + k, bin, pk, ref, anchors);
}

// ---- host entries: copy the cases in, launch, synchronise once, copy the results out; -> 0 or the line of the call that failed
struct DevBuf {
	void *p = nullptr; size_t n = 0;
	int up(const void *src, size_t bytes) { n = bytes ? bytes : 16; if (hipMalloc(&p, n) != hipSuccess) { p = nullptr; return 1; } return bytes && src ? hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) != hipSuccess : 0; }
	int down(void *dst) { return hipMemcpy(dst, p, n, hipMemcpyDeviceToHost) != hipSuccess; }
	~DevBuf() { if (p) (void)hipFree(p); }
};
#define CK(e) do { if (e) { fprintf(stderr, "dsb_stage: %s failed at line %d (%s)\n", #e, __LINE__, hipGetErrorString(hipGetLastError())); return __LINE__; } } while (0)
static int stage_common(DevBuf &slices, DevBuf &ri)
{
	const DsbRefInfo r = {~0ULL, 0};
	CK(hipMalloc(&slices.p, (size_t)STAGE_GRID * STAGE_SLICE) != hipSuccess);
	slices.n = (size_t)STAGE_GRID * STAGE_SLICE;
	CK(ri.up(&r, sizeof r));
	return 0;
}
extern "C" uint32_t stage_dev_sizes(uint32_t *out)
{
	out[0] = sizeof(StageSdp); out[1] = sizeof(StageChain); out[2] = sizeof(DsbGap); out[3] = DSB_WTAB_SLOTS; out[4] = DSB_WTAB_MAXQ; out[5] = DSB_INV_PAIRS; out[6] = DSB_INV_MINQ; out[7] = DSB_INV_MAXPOS;
	out[8] = DSB_SDP_CAND; out[9] = DSB_SDP_KEEP; out[10] = DSB_GL_QW; out[11] = DSB_GL_NODES; out[12] = DSB_GL_MAXT; out[13] = DSB_INV_WORDS; out[14] = 64; out[15] = STAGE_MAX_ANC;
	return 16;
}
extern "C" int stage_dev_sdp(int form, StageSdp *cases, uint32_t n, const uint8_t *bin, size_t bin_bytes, const uint64_t *pk, size_t pk_words, const uint8_t *win, size_t win_bytes,
                             DsbSms *nodes, size_t node_entries, uint4 *mirror)
{
	DevBuf dc, db, dp, dw, dn, dm, ds, dr;
	CK(stage_common(ds, dr));
	CK(dc.up(cases, (size_t)n * sizeof(StageSdp))); CK(db.up(bin, bin_bytes)); CK(dp.up(pk, 8 * pk_words)); CK(dw.up(win, win_bytes));
	CK(dn.up(nodes, node_entries * sizeof(DsbSms))); CK(dm.up(mirror, (size_t)n * 64 * sizeof(uint4)));
	for (uint32_t base = 0; base < n; base += STAGE_GRID)
		hipLaunchKernelGGL(k_stage_sdp, dim3(n - base < STAGE_GRID ? n - base : STAGE_GRID), dim3(64), 0, 0, form, (StageSdp *)dc.p, base, n, (const uint8_t *)db.p, (const uint64_t *)dp.p,
		                   (const uint8_t *)dw.p, (DsbSms *)dn.p, (uint4 *)dm.p, (uint8_t *)ds.p, (const DsbRefInfo *)dr.p);
	CK(hipGetLastError() != hipSuccess);
	CK(hipDeviceSynchronize() != hipSuccess);
	if (n) { CK(dc.down(cases)); CK(dn.down(nodes)); CK(dm.down(mirror)); }
	return 0;
}
extern "C" int stage_dev_gap_lane(StageChain *cases, uint32_t n, const uint8_t *bin, size_t bin_bytes, const uint64_t *pk, size_t pk_words, const uint8_t *ref, size_t ref_bytes, DsbGap *G, size_t n_gaps)
{
	DevBuf dc, db, dp, dt, dg, ds, dr;
	CK(stage_common(ds, dr));
	CK(dc.up(cases, (size_t)n * sizeof(StageChain))); CK(db.up(bin, bin_bytes)); CK(dp.up(pk, 8 * pk_words)); CK(dt.up(ref, ref_bytes)); CK(dg.up(G, n_gaps * sizeof(DsbGap)));
	for (uint32_t base = 0; base < n; base += STAGE_GRID)
		hipLaunchKernelGGL(k_stage_gap_lane, dim3(n - base < STAGE_GRID ? n - base : STAGE_GRID), dim3(64), 0, 0, (StageChain *)dc.p, base, n, (const uint8_t *)db.p, (const uint64_t *)dp.p,
		                   (const uint8_t *)dt.p, (DsbGap *)dg.p, (uint8_t *)ds.p, (const DsbRefInfo *)dr.p);
	CK(hipGetLastError() != hipSuccess);
	CK(hipDeviceSynchronize() != hipSuccess);
	if (n) { CK(dc.down(cases)); if (n_gaps) CK(dg.down(G)); }
	return 0;
}
extern "C" int stage_dev_middle(StageChain *cases, uint32_t n, const uint8_t *bin, size_t bin_bytes, const uint64_t *pk, size_t pk_words, const uint8_t *ref, size_t ref_bytes, const int32_t *anchors, size_t n_rows)
{
	DevBuf dc, db, dp, dt, da, ds, dr;
	CK(stage_common(ds, dr));
	CK(dc.up(cases, (size_t)n * sizeof(StageChain))); CK(db.up(bin, bin_bytes)); CK(dp.up(pk, 8 * pk_words)); CK(dt.up(ref, ref_bytes)); CK(da.up(anchors, n_rows * 16));
	for (uint32_t base = 0; base < n; base += STAGE_GRID)
		hipLaunchKernelGGL(k_stage_middle, dim3(n - base < STAGE_GRID ? n - base : STAGE_GRID), dim3(64), 0, 0, (StageChain *)dc.p, base, n, (const uint8_t *)db.p, (const uint64_t *)dp.p,
		                   (const uint8_t *)dt.p, (const int32_t *)da.p, (uint8_t *)ds.p, (const DsbRefInfo *)dr.p);
	CK(hipGetLastError() != hipSuccess);
	CK(hipDeviceSynchronize() != hipSuccess);
	if (n) CK(dc.down(cases));
	return 0;
}

// ---- the sparse DP on bare node lists (tests/test_stage_dp.py): forms (a) .. (c) on one wavefront per case ...
__global__ void __launch_bounds__(64) k_stage_dp(StageDp *cases, uint32_t base, uint32_t n, DsbSms *nodes, const uint32_t *sizes, uint8_t *slices, const DsbRefInfo *refinfo)
{
	const uint32_t k = base + blockIdx.x;
	if (k >= n) return;
	STAGE_KERNEL_CTX
	stage_dp(w, (DSB_LDS_AS DsbDevIndex *)&sx, cases + k, nodes, sizes);
}
// ... and form (d): the pass over the old predecessors of a batch on W wavefronts (sdp_batch_old_mw), called directly whatever DSB_MW_MIN_PREDS
// says.  Wave 0 posts a batch of K nodes (K from the case's sizes, 1 .. DSB_DPB) as sdp_best_pred_b posts it, every wave runs the pass with its
// own wave number, wave 0 combines the waves' maxima as sdp_best_pred_b does and scores the batch's nodes through sdp_best_pred_b itself (its
// own old pass is skipped: the batch bounds and old_best are in place), keeping the ring.  Every wave reaches every barrier: the batch
// bounds come from the case, and the exits of sdp_batch_old_mw's round loop depend on n0, W and the cut flags all waves read from LDS.
template <int W>
__global__ void __launch_bounds__(64 * W) k_stage_dp_mw(StageDp *cases, uint32_t base, uint32_t n, DsbSms *nodes, const uint32_t *sizes)
{
	const uint32_t k = base + blockIdx.x;
	if (k >= n) return;
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	__shared__ DsbDevIndex sx;
	__shared__ uint4 lds_ring[DSB_RING];
	__shared__ uint32_t lds_red[W + 1];
	__shared__ uint32_t lds_cnt[4];
	__shared__ DpBatch lds_dpb;
	__shared__ DsbMw mw;
	__shared__ WCtx s_w;
	WCtxL &w = *(WCtxL *)&s_w;
	const StageDp c = cases[k];
	DsbSms *const sms = nodes + c.node_off;
	const uint32_t *const sz = sizes + c.s0;
	if (threadIdx.x < 4) lds_cnt[threadIdx.x] = 0;
	__syncthreads();
	if (wv == 0) {
		w.dpb = (DpBatchL *)&lds_dpb;
		w.x = (DsbXP)&sx; w.dbg = nullptr; w.ring = lds_ring; w.red = lds_red; w.k.c = (lds_u32 *)lds_cnt; w.k.uni = 1; w.step_limit = DSB_STEP_LIMIT; w.stage = 0;
		stage_dp_begin(w, (DSB_LDS_AS DsbDevIndex *)&sx, c, sms);
		if (c.n) { const DsbSms s0 = sms[0]; ring_put(w, 0, s0.t_pos, s0.q_pos, s0.len, s0.score); }
	}
	__syncthreads();
	NodeBlock nb; nb.base = 0; nb.valid = 0;
	uint32_t steps = 0, bi = 0;
	for (uint32_t n0 = 1; n0 < c.n; bi++) {
		uint32_t K = c.n_sizes ? sz[bi % c.n_sizes] : (uint32_t)DSB_DPB;
		K = K < 1u ? 1u : K > (uint32_t)DSB_DPB ? (uint32_t)DSB_DPB : K;
		if (K > c.n - n0) K = c.n - n0;
		if (wv == 0) {
			if (lane < DSB_DPB) { const DsbSms g = sms[n0 + ((uint32_t)lane < K ? lane : 0)]; mw.nd_t[lane] = g.t_pos; mw.nd_q[lane] = g.q_pos; mw.nd_l[lane] = g.len; }
			if (lane == 0) { mw.cmd = c.mode; mw.n0 = n0; mw.K = K; mw.sms = sms; }
		}
		__syncthreads();
		uint32_t preds = 0;
		if (c.mode == 1) sdp_batch_old_mw<1>(&mw, lds_ring, lds_red, lane, wv, W, &preds);
		else sdp_batch_old_mw<2>(&mw, lds_ring, lds_red, lane, wv, W, &preds);
		if (wv == 0) {
			DpBatchL &b = *w.dpb;
			if (lane == 0) {
				b.n0 = n0; b.K = K;
				for (uint32_t j = 0; j < DSB_DPB; j++) { int m = -2147483647 - 1; for (int u = 0; u < W; u++) m = MAXV(m, mw.best[u][j]); b.old_best[j] = j < K ? m : 0; }
			}
			w.dp_preds += preds;
			wave_sync();
			uint32_t bn0 = n0, bK = K;
			for (uint32_t cur = n0; cur < n0 + K; cur++) {
				DsbSms nd = sms[cur]; nd.score = 0;
				const int sc = c.mode == 1 ? sdp_best_pred_b<1>(w, b, nd, (int32_t)cur, nb, c.n, lds_ring, steps, bn0, bK) : sdp_best_pred_b<2>(w, b, nd, (int32_t)cur, nb, c.n, lds_ring, steps, bn0, bK);
				sms[cur].score = (uint32_t)sc;
				{ uint4 r_; r_.x = nd.t_pos; r_.y = nd.q_pos; r_.z = nd.len; r_.w = (uint32_t)sc; ring_st(lds_ring, cur & (DSB_RING - 1), r_); }
			}
			if (b.n0 != n0 || b.K != K || bn0 != n0 || bK != K) w.status |= DSB_ST_TIMEOUT;      // sdp_best_pred_b filled the batch anew: its own old pass ran, not the one under test (the test wants status 0)
		}
		__threadfence_block();
		__syncthreads();                                                // the scores and the ring: the next batch's old predecessors
		n0 += K;
	}
	if (threadIdx.x == 0) { cases[k].status = (uint32_t)w.status; cases[k].dp_preds = w.dp_preds; cases[k].scored = c.n; cases[k].defined = 1; }
}
extern "C" uint32_t stage_dev_sizes_dp(uint32_t *out)
{
	out[0] = sizeof(StageDp); out[1] = STAGE_DP_GUARD; out[2] = DSB_RING; out[3] = DSB_DPB; out[4] = DSB_DP_UNROLL; out[5] = 64; out[6] = DSB_MW_MAXW; out[7] = DSB_ST_HEAVY;
	return 8;
}
// all cases of one call take the same form, and for form (d) the same number of wavefronts (2, 4 or 8)
extern "C" int stage_dev_dp(StageDp *cases, uint32_t n, DsbSms *nodes, size_t node_entries, const uint32_t *sizes, size_t n_sizes)
{
	DevBuf dc, dn, dz, ds, dr;
	CK(stage_dp_check(cases, n, node_entries, n_sizes));
	if (!n) return 0;
	const uint32_t form = cases[0].form, W = cases[0].waves;
	for (uint32_t k = 0; k < n; k++) CK(cases[k].form != form || (form == DP_MW && (cases[k].waves != W || cases[k].mode == 0)));
	CK(form == DP_MW && W != 2 && W != 4 && W != 8);
	CK(stage_common(ds, dr));
	CK(dc.up(cases, (size_t)n * sizeof(StageDp))); CK(dn.up(nodes, node_entries * sizeof(DsbSms))); CK(dz.up(sizes, n_sizes * 4));
	for (uint32_t base = 0; base < n; base += STAGE_GRID) {
		const dim3 grid(n - base < STAGE_GRID ? n - base : STAGE_GRID);
		if (form != DP_MW) hipLaunchKernelGGL(k_stage_dp, grid, dim3(64), 0, 0, (StageDp *)dc.p, base, n, (DsbSms *)dn.p, (const uint32_t *)dz.p, (uint8_t *)ds.p, (const DsbRefInfo *)dr.p);
		else if (W == 2) hipLaunchKernelGGL(k_stage_dp_mw<2>, grid, dim3(128), 0, 0, (StageDp *)dc.p, base, n, (DsbSms *)dn.p, (const uint32_t *)dz.p);
		else if (W == 4) hipLaunchKernelGGL(k_stage_dp_mw<4>, grid, dim3(256), 0, 0, (StageDp *)dc.p, base, n, (DsbSms *)dn.p, (const uint32_t *)dz.p);
		else hipLaunchKernelGGL(k_stage_dp_mw<8>, grid, dim3(512), 0, 0, (StageDp *)dc.p, base, n, (DsbSms *)dn.p, (const uint32_t *)dz.p);
	}
	CK(hipGetLastError() != hipSuccess);
	CK(hipDeviceSynchronize() != hipSuccess);
	CK(dc.down(cases)); CK(dn.down(nodes));
	return 0;
}

// ---- one sdp_right_M2 / sdp_left_M2 per case (tests/test_stage_ext.py)
__global__ void __launch_bounds__(64) k_stage_ext(StageExt *cases, uint32_t base, uint32_t n, const uint8_t *bin, const uint64_t *pk, const uint8_t *ref, DsbChain *chains, const int32_t *anchors,
                                                  DsbSms *nodes, DsbScHash *scs, const DsbRefInfo *ris, uint8_t *slices, const DsbRefInfo *refinfo)
{
	const uint32_t k = base + blockIdx.x;
	if (k >= n) return;
	STAGE_KERNEL_CTX
	stage_ext(w, (DSB_LDS_AS DsbDevIndex *)&sx, cases + k, bin, pk, ref, chains, anchors, nodes, scs, ris);
}
extern "C" uint32_t stage_dev_sizes_ext(uint32_t *out) { out[0] = sizeof(StageExt); out[1] = sizeof(DsbChain); out[2] = sizeof(DsbScHash); out[3] = sizeof(DsbRefInfo); return 4; }
extern "C" int stage_dev_ext(StageExt *cases, uint32_t n, const uint8_t *bin, size_t bin_bytes, const uint64_t *pk, size_t pk_words, const uint8_t *ref, size_t ref_bytes,
                             DsbChain *chains, size_t n_chains, const int32_t *anchors, size_t n_rows, DsbSms *nodes, size_t node_entries, DsbScHash *scs, size_t n_sc,
                             const DsbRefInfo *ris, size_t n_ri)
{
	DevBuf dc, db, dp, dt, dh, da, dn, dz, di, ds, dr;
	CK(stage_ext_check(cases, n, n_chains, n_rows, anchors, chains, node_entries, n_sc, n_ri));
	if (!n) return 0;
	CK(stage_common(ds, dr));
	CK(dc.up(cases, (size_t)n * sizeof(StageExt))); CK(db.up(bin, bin_bytes)); CK(dp.up(pk, 8 * pk_words)); CK(dt.up(ref, ref_bytes)); CK(dh.up(chains, n_chains * sizeof(DsbChain)));
	CK(da.up(anchors, n_rows * 20)); CK(dn.up(nodes, node_entries * sizeof(DsbSms))); CK(dz.up(scs, n_sc * sizeof(DsbScHash))); CK(di.up(ris, n_ri * sizeof(DsbRefInfo)));
	for (uint32_t base = 0; base < n; base += STAGE_GRID)
		hipLaunchKernelGGL(k_stage_ext, dim3(n - base < STAGE_GRID ? n - base : STAGE_GRID), dim3(64), 0, 0, (StageExt *)dc.p, base, n, (const uint8_t *)db.p, (const uint64_t *)dp.p, (const uint8_t *)dt.p,
		                   (DsbChain *)dh.p, (const int32_t *)da.p, (DsbSms *)dn.p, (DsbScHash *)dz.p, (const DsbRefInfo *)di.p, (uint8_t *)ds.p, (const DsbRefInfo *)dr.p);
	CK(hipGetLastError() != hipSuccess);
	CK(hipDeviceSynchronize() != hipSuccess);
	CK(dc.down(cases)); CK(dh.down(chains)); CK(dn.down(nodes));
	return 0;
}

// ---- the chain stages (a-10, a-13, a-14, a-17): a slice layout of their own (STAGE2_SLICE), fewer workgroups per launch
#define STAGE2_GRID 128u
#define STAGE2_KERNEL_CTX                                                                                          \
	__shared__ DsbDevIndex sx;                                                                                     \
	__shared__ uint4 lds_ring[DSB_RING];                                                                           \
	__shared__ __attribute__((aligned(16))) uint32_t lds_wtab[DSB_WTAB_SLOTS];                                     \
	__shared__ uint32_t lds_red[2];                                                                                \
	__shared__ uint32_t lds_cnt[4];                                                                                \
	__shared__ DpBatch lds_dpb;                                                                                    \
	__shared__ WCtx s_w;                                                                                           \
	WCtxL &w = *(WCtxL *)&s_w;                                                                                     \
	if (threadIdx.x < 4) lds_cnt[threadIdx.x] = 0;                                                                 \
	__syncthreads();                                                                                               \
	w.dpb = (DpBatchL *)&lds_dpb;                                                                                  \
	uint8_t *const slice = slices + (size_t)blockIdx.x * STAGE2_SLICE;                                             \
	stage_ctx(w, (DSB_LDS_AS DsbDevIndex *)&sx, slice, lds_wtab, lds_ring, lds_red, lds_cnt, refinfo);             \
	__syncthreads();
static_assert(STAGE2_SLICE >= STAGE_SLICE, "stage_ctx points the a-12 arrays into the slice before stage2_ctx lays it out anew");

__global__ void __launch_bounds__(64) k_stage_resolve(StageRes *cases, uint32_t base, uint32_t n, const uint32_t *rows, uint32_t *order, int32_t *pre, DsbChain *hits, DsbChain *raw,
                                                      uint8_t *slices, const DsbRefInfo *refinfo)
{
	const uint32_t k = base + blockIdx.x;
	if (k >= n) return;
	STAGE2_KERNEL_CTX
	stage_resolve(w, cases + k, rows, order, pre, hits, raw, slice);
}
__global__ void __launch_bounds__(64) k_stage_finish(StageFin *cases, uint32_t base, uint32_t n, DsbChain *chains, DsbChain *tail, uint8_t *slices, const DsbRefInfo *refinfo)
{
	const uint32_t k = base + blockIdx.x;
	if (k >= n) return;
	STAGE2_KERNEL_CTX
	stage_finish(w, (DSB_LDS_AS DsbDevIndex *)&sx, cases + k, chains, tail, slice);
}
static int stage2_common(DevBuf &slices, DevBuf &ri)
{
	const DsbRefInfo r = {~0ULL, 0};
	CK(hipMalloc(&slices.p, (size_t)STAGE2_GRID * STAGE2_SLICE) != hipSuccess);
	slices.n = (size_t)STAGE2_GRID * STAGE2_SLICE;
	CK(ri.up(&r, sizeof r));
	return 0;
}
extern "C" uint32_t stage_dev_sizes2(uint32_t *out)
{
	out[0] = sizeof(StageRes); out[1] = sizeof(StageFin); out[2] = sizeof(DsbChain); out[3] = DSB_WTAB_SLOTS; out[4] = DSB_RANKSORT_MAX; out[5] = DSB_CHAINDP_LDS; out[6] = STAGE2_MAX_ANC; out[7] = STAGE2_MAX_HIT;
	out[8] = STAGE2_GUARD; out[9] = 64;
	return 10;
}
extern "C" int stage_dev_resolve(StageRes *cases, uint32_t n, const uint32_t *rows, size_t n_rows, uint32_t *order, int32_t *pre, DsbChain *hits, size_t n_hits, DsbChain *raw, size_t n_raw)
{
	DevBuf dc, da, dord, dpre, dh, dw, ds, dr;
	CK(stage_resolve_check(cases, n, rows, n_rows, n_hits, n_raw));
	CK(stage2_common(ds, dr));
	CK(dc.up(cases, (size_t)n * sizeof(StageRes))); CK(da.up(rows, n_rows * 32)); CK(dord.up(order, n_rows * 4)); CK(dpre.up(pre, n_rows * 4));
	CK(dh.up(hits, n_hits * sizeof(DsbChain))); CK(dw.up(raw, n_raw * sizeof(DsbChain)));
	for (uint32_t base = 0; base < n; base += STAGE2_GRID)
		hipLaunchKernelGGL(k_stage_resolve, dim3(n - base < STAGE2_GRID ? n - base : STAGE2_GRID), dim3(64), 0, 0, (StageRes *)dc.p, base, n, (const uint32_t *)da.p, (uint32_t *)dord.p, (int32_t *)dpre.p,
		                   (DsbChain *)dh.p, (DsbChain *)dw.p, (uint8_t *)ds.p, (const DsbRefInfo *)dr.p);
	CK(hipGetLastError() != hipSuccess);
	CK(hipDeviceSynchronize() != hipSuccess);
	if (n) { CK(dc.down(cases)); CK(dh.down(hits)); if (n_rows) { CK(dord.down(order)); CK(dpre.down(pre)); } if (n_raw) CK(dw.down(raw)); }
	return 0;
}
extern "C" int stage_dev_finish(StageFin *cases, uint32_t n, DsbChain *chains, DsbChain *tail, size_t n_chains)
{
	DevBuf dc, dh, dt, ds, dr;
	CK(stage_finish_check(cases, n, n_chains));
	CK(stage2_common(ds, dr));
	CK(dc.up(cases, (size_t)n * sizeof(StageFin))); CK(dh.up(chains, n_chains * sizeof(DsbChain))); CK(dt.up(tail, n_chains * sizeof(DsbChain)));
	for (uint32_t base = 0; base < n; base += STAGE2_GRID)
		hipLaunchKernelGGL(k_stage_finish, dim3(n - base < STAGE2_GRID ? n - base : STAGE2_GRID), dim3(64), 0, 0, (StageFin *)dc.p, base, n, (DsbChain *)dh.p, (DsbChain *)dt.p, (uint8_t *)ds.p, (const DsbRefInfo *)dr.p);
	CK(hipGetLastError() != hipSuccess);
	CK(hipDeviceSynchronize() != hipSuccess);
	if (n && n_chains) { CK(dc.down(cases)); CK(dh.down(chains)); CK(dt.down(tail)); } else if (n) CK(dc.down(cases));
	return 0;
}

// ---- the anchor stage (a-4 .. a-8): the FM search, fast_island, fast_classify, fast_classify_lane, slow_classify on a loaded index (tests/test_stage_anchor.py).
// The index comes from the host view of an opened index (dsb_index_host: the test passes the pointer): what the walk reads of it is uploaded once.
#include "dsb_host.h"
#define STAGE3_GRID 256u     /* workgroups and scratch slices (1.4 MB each) per launch */
#define STAGE3_KERNEL_CTX                                                                                          \
	__shared__ DsbDevIndex sx;                                                                                     \
	__shared__ uint4 lds_ring[DSB_RING];                                                                           \
	__shared__ __attribute__((aligned(16))) uint32_t lds_wtab[DSB_WTAB_SLOTS];                                     \
	__shared__ uint32_t lds_red[2];                                                                                \
	__shared__ uint32_t lds_cnt[4];                                                                                \
	__shared__ DpBatch lds_dpb;                                                                                    \
	__shared__ WCtx s_w;                                                                                           \
	WCtxL &w = *(WCtxL *)&s_w;                                                                                     \
	if (threadIdx.x < 4) lds_cnt[threadIdx.x] = 0;                                                                 \
	__syncthreads();                                                                                               \
	w.dpb = (DpBatchL *)&lds_dpb;                                                                                  \
	uint8_t *const slice = slices + (size_t)blockIdx.x * STAGE3_SLICE;                                             \
	stage_ctx(w, (DSB_LDS_AS DsbDevIndex *)&sx, slice, lds_wtab, lds_ring, lds_red, lds_cnt, dx->refinfo);         \
	__syncthreads();
static_assert(STAGE3_SLICE >= STAGE_SLICE, "stage_ctx points the a-12 arrays into the slice before stage3_ctx lays it out anew");

__global__ void __launch_bounds__(64) k_stage_anchor(const DsbDevIndex *dx, StageAnc *cases, uint32_t base, uint32_t n, const uint8_t *bin, DsbSeed *seeds, DsbAnchor *anchors, const int32_t *calls,
                                                     int64_t *mems, uint8_t *slices)
{
	const uint32_t k = base + blockIdx.x;
	if (k >= n) return;
	STAGE3_KERNEL_CTX
	stage_anchor(w, (DSB_LDS_AS DsbDevIndex *)&sx, dx, cases + k, bin, seeds, anchors, calls, mems, slice);
}
__global__ void __launch_bounds__(64) k_stage_anchor_lane(const DsbDevIndex *dx, StageAnc *cases, uint32_t base, uint32_t n, const uint8_t *bin, DsbSeed *seeds, DsbAnchor *anchors, uint8_t *slices)
{
	const uint32_t k0 = base + 64u * blockIdx.x;
	if (k0 >= n) return;
	STAGE3_KERNEL_CTX
	stage_anchor_lane(w, (DSB_LDS_AS DsbDevIndex *)&sx, dx, cases, k0, n, bin, seeds, anchors, slice);
}
struct Stage3DevIndex { DevBuf fm, fm_sb, hash, sa, uni, refpos, refbin, refinfo, qmem, qlv, dx; int ek_len; uint32_t info[3]; };
extern "C" void *stage_dev_anchor_index(const DsbHostIndex *h)
{
	Stage3DevIndex *s = new Stage3DevIndex();
	DsbDevIndex dx; memset(&dx, 0, sizeof dx);
	bool bad = false;
	bad |= s->fm.up(h->fm, h->n_fm * sizeof(DsbFmBlock)) != 0;
	if (h->fm_sb) bad |= s->fm_sb.up(h->fm_sb, h->n_fm_sb * 40) != 0;
	if (h->hash_c) bad |= s->hash.up(h->hash_c, (size_t)h->n_hash_c * sizeof(DsbHiLine)) != 0; else bad |= s->hash.up(h->hash_index, (((size_t)1 << 26) + 1) * 8) != 0;
	bad |= s->sa.up(h->sa, h->sa_size * 8) != 0; bad |= s->uni.up(h->uni, (h->n_uni + 1) * 8) != 0; bad |= s->refpos.up(h->refpos, (h->n_refpos + 1) * 8) != 0;
	bad |= s->refbin.up(h->refbin, h->n_refbin + 4096) != 0; bad |= s->refinfo.up(h->refinfo, h->n_ref * sizeof(DsbRefInfo)) != 0;
	bad |= s->qmem.up(h->Q_MEM, 2000 * sizeof(int)) != 0; bad |= s->qlv.up(&h->Q_LV[0][0], 400 * sizeof(int)) != 0;
	dx.ek_mask = h->ek_mask; dx.ek_len = h->ek_len; dx.single_base_max = h->single_base_max;          // (the filter tables are not uploaded: the walk does not read them)
	dx.fm = (const DsbFmBlock *)s->fm.p; dx.fm_sb = h->fm_sb ? (const uint64_t *)s->fm_sb.p : nullptr; dx.bwt_len = h->bwt_len; memcpy(dx.rank, h->rank, sizeof dx.rank);
	dx.dollar_pos = h->dollar_pos; dx.dollar_row = h->dollar_row;
	dx.hash_index = h->hash_c ? nullptr : (const uint64_t *)s->hash.p; dx.hash_c = h->hash_c ? (const DsbHiLine *)s->hash.p : nullptr;
	dx.sa = (const uint2 *)s->sa.p; dx.uni = (const uint2 *)s->uni.p; dx.refpos = (const uint64_t *)s->refpos.p; dx.refbin = (const uint8_t *)s->refbin.p; dx.ref_bases = h->n_refbin * 4;
	dx.refinfo = (const DsbRefInfo *)s->refinfo.p; dx.qmem = (const int *)s->qmem.p; dx.qlv = (const int *)s->qlv.p;
	bad |= s->dx.up(&dx, sizeof dx) != 0;
	s->ek_len = h->ek_len; s->info[0] = h->hash_c != nullptr; s->info[1] = h->fm_sb != nullptr; s->info[2] = (uint32_t)h->ek_len;
	if (bad) { fprintf(stderr, "dsb_stage: uploading the index failed (%s)\n", hipGetErrorString(hipGetLastError())); delete s; return nullptr; }
	return s;
}
extern "C" void stage_dev_anchor_index_free(void *p) { delete (Stage3DevIndex *)p; }
extern "C" void stage_dev_anchor_index_info(void *p, uint32_t *out) { memcpy(out, ((Stage3DevIndex *)p)->info, 12); }
extern "C" uint32_t stage_dev_sizes3(uint32_t *out)
{
	out[0] = sizeof(StageAnc); out[1] = sizeof(DsbAnchor); out[2] = sizeof(DsbSeed); out[3] = DSB_LANE_ANC_CAP; out[4] = DSB_LANE_STEPS; out[5] = STAGE3_GUARD; out[6] = STAGE3_MEM; out[7] = 64;
	out[8] = DSB_SPSET_CAP; out[9] = STAGE3_MAX_SEEDS;
	return 10;
}
// all cases of one call are ANC_LANE (64 reads per workgroup, one per lane) or none is
extern "C" int stage_dev_anchor(void *index, StageAnc *cases, uint32_t n, const uint8_t *bin, size_t bin_bytes, DsbSeed *seeds, size_t n_seeds, DsbAnchor *anchors, size_t n_anchors,
                                const int32_t *calls, size_t n_calls, int64_t *mems, size_t n_mems)
{
	Stage3DevIndex *si = (Stage3DevIndex *)index;
	DevBuf dc, db, dsd, da, dq, dm, ds;
	CK(!si);
	CK(stage_anchor_check(cases, n, bin_bytes, n_seeds, n_anchors, calls, n_calls, n_mems, seeds, si->ek_len));
	if (!n) return 0;
	const bool lanes = cases[0].form == ANC_LANE;
	for (uint32_t k = 0; k < n; k++) CK((cases[k].form == ANC_LANE) != lanes);
	CK(hipMalloc(&ds.p, (size_t)STAGE3_GRID * STAGE3_SLICE) != hipSuccess);
	ds.n = (size_t)STAGE3_GRID * STAGE3_SLICE;
	CK(hipMemset(ds.p, 0, ds.n) != hipSuccess);
	CK(dc.up(cases, (size_t)n * sizeof(StageAnc))); CK(db.up(bin, bin_bytes)); CK(dsd.up(seeds, n_seeds * sizeof(DsbSeed))); CK(da.up(anchors, n_anchors * sizeof(DsbAnchor)));
	CK(dq.up(calls, n_calls * 16)); CK(dm.up(mems, n_mems * STAGE3_MEM * 8));
	const uint32_t per = lanes ? 64u * STAGE3_GRID : STAGE3_GRID;
	for (uint32_t base = 0; base < n; base += per) {
		const uint32_t rest = n - base, grid = lanes ? ((rest < per ? rest : per) + 63u) / 64u : (rest < per ? rest : per);
		if (lanes) hipLaunchKernelGGL(k_stage_anchor_lane, dim3(grid), dim3(64), 0, 0, (const DsbDevIndex *)si->dx.p, (StageAnc *)dc.p, base, n, (const uint8_t *)db.p, (DsbSeed *)dsd.p, (DsbAnchor *)da.p, (uint8_t *)ds.p);
		else hipLaunchKernelGGL(k_stage_anchor, dim3(grid), dim3(64), 0, 0, (const DsbDevIndex *)si->dx.p, (StageAnc *)dc.p, base, n, (const uint8_t *)db.p, (DsbSeed *)dsd.p, (DsbAnchor *)da.p,
		                        (const int32_t *)dq.p, (int64_t *)dm.p, (uint8_t *)ds.p);
	}
	CK(hipGetLastError() != hipSuccess);
	CK(hipDeviceSynchronize() != hipSuccess);
	CK(dc.down(cases)); CK(da.down(anchors)); if (n_mems) CK(dm.down(mems));
	return 0;
}
