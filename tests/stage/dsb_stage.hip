// TEST INFRASTRUCTURE: stage a-12 of the device code (dsb_classify_dev.h: sdp_match in its five forms, gap_lane, sdp_middle_M2) and the
// chain stages a-10, a-13, a-14 and a-17 (resolve_tree in every form, the tail of delete_small_score_rst, detect_primary, glibc_sort_chains) on
// the GPU, form by form, with the real wavefront primitives of dsb_wave.h (tests/stage/dsb_stage_forms.h holds the forms; the
// host emulation runs the same text).  One wavefront per workgroup, one workgroup per case; the context is set up as
// classify_kernel_body (dsb_gpu.hip) sets it up.  Built into tests/stage/libdsbstage.so; nothing of it is in libdesamba_amd.so.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
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
