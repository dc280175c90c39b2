// Per-hit edit distance and per-reference identity (dsb_identity.h): the banded alignment of every counted record of a
// batch, one wavefront per record, after the batch's last classify launch; the run's per-reference table; the bare-pair entry
// dsb_ctx_edit_pairs, which runs the same device function on sequences of the caller's.  With dsb_ctx_enable_alignment the
// same pass also keeps the path: k_hit_align in place of k_hit_edits, ident_path behind the tracing form of ident_wave,
// dsb_ctx_align_pairs.  In checkpoint mode (dsb_ctx_alignment_mode) k_hit_align_ck runs instead: the trace of one segment
// of K generations, a checkpoint of every K-th generation, and a walk back that recomputes the earlier segments (ident_path_ck).
//
// The alignment is the diagonal-transition form of the banded unit-cost problem.  Diagonal k holds the cells (i, i + k), i bases of Q
// against i + k bases of T; FR_e[k] is the largest i on diagonal k that e edits reach.  The band is a set of whole diagonals
// [lo, hi] = [min(0, d) - B, max(0, d) + B] (d = m - n), so the recurrence over the diagonals of the band computes exactly the value
// of the banded DP: FR_e[k] = max(FR_{e-1}[k] + 1 (mismatch), FR_{e-1}[k - 1] (a base of T alone), FR_{e-1}[k + 1] + 1 (a base of Q
// alone)) over the candidates that lie in the rectangle, then the slide along the diagonal while Q[i] == T[i + k].  The distance is
// the first e with FR_e[d] >= n.
#include <algorithm>
#include "dsb_ctx.h"
#include "dsb_sam_fields.h"
#include "dsb_wave.h"

#define IDENT_NEG (-0x40000000)                        // a diagonal no path has reached
#define IDENT_BAD (DSB_IDENT_EMPTY | DSB_IDENT_SKEW | DSB_IDENT_OVER)
#define IDENT_MAX_LEN 0x40000000u                      // dsb_ctx_edit_pairs: longest sequence (the furthest-reaching points are ints)
#define IDENT_MAX_OFF (1ull << 40)                     // dsb_ctx_edit_pairs: furthest start of a pair in its blob
#define IDENT_MAX_RUN 0x10000000u                      // an operation's length has 28 bits (BAM's): longer sequences get no path
#define IDENT_T_PAD 16                                // bytes behind a packed text that a 32-base fetch may read (refbin has 4 KiB)

// Q: packed words, 32 bases each, the first in the top bits, base qbase of them the first of Q (a read strand of d_pk, or a blob of
// dsb_ctx_edit_pairs; one pad word behind).  T: packed bytes, 4 bases each, the first in the top bits, base tbase the first of T.
struct IdentSeq { const uint64_t *qw; uint64_t qbase; const uint8_t *tb; uint64_t tbase; uint32_t n, m; };

// 32 bases from base a on, the first in the top bits: two words funnel-shifted to the phase / nine bytes, byte-swapped, likewise
DV uint64_t ident_q32(const uint64_t *qw, uint64_t a)
{
	const uint64_t w = a >> 5; const uint32_t sh = (uint32_t)(a & 31u) * 2u;
	const uint64_t x = DSB_G64(qw, w), y = DSB_G64(qw, w + 1);
	return sh ? (x << sh) | (y >> (64u - sh)) : x;
}
DV uint64_t ident_t32(const uint8_t *tb, uint64_t a)
{
	const uint8_t *p = tb + (a >> 2); const uint32_t sh = (uint32_t)(a & 3u) * 2u;
	const uint64_t x = __builtin_bswap64(dsb_g64u(p)); const uint32_t y = p[8];
	return sh ? (x << sh) | (uint64_t)(y >> (8u - sh)) : x;
}

// from cell (i, i + k): the first i' >= i with Q[i'] != T[i' + k], or where the rectangle ends.  32 bases per step; what a fetch
// reads beyond n or m (the next bases, the pads) never counts: every step is clipped to the room left.
DV int ident_slide(const IdentSeq &s, int i, int k)
{
	int j = i + k;
	while (i < (int)s.n && j < (int)s.m) {
		const uint64_t d = ident_q32(s.qw, s.qbase + (uint64_t)i) ^ ident_t32(s.tb, s.tbase + (uint64_t)j);
		int eq = d ? (__builtin_clzll(d) >> 1) : 32;
		const int room = min((int)s.n - i, (int)s.m - j);
		if (eq > room) eq = room;
		i += eq; j += eq;
		if (eq < 32) break;
	}
	return i;
}

// The band of a pair of n x m bases, stated once for the forward pass, the walk back, the recomputation and ident_plan: d = m - n,
// the diagonals [lo, hi], W of them, and R, the 8-byte words of a generation's trace (two bit planes per round of 64 diagonals:
// 16 * ceil(W / 64) bytes, the R of DESIGN 2.13, are 8 * R).  Generation e writes the diagonals [klo(e), khi(e)] = [max(lo, -e),
// min(hi, e)].  All of it is wave-uniform.  (ints, as the furthest-reaching points are: right for n, m <= 2^30, which dsb_aln_plan
// and the pair entries check.)  Passed by value: behind a reference the loops that store ints would have to read its fields again,
// which costs two vector registers in every kernel.
struct IdentBand {
	int delta, lo, hi, W; uint32_t R;
	DSB_HD int klo(uint32_t e) const { return lo > -(int)e ? lo : -(int)e; }
	DSB_HD int khi(uint32_t e) const { return hi < (int)e ? hi : (int)e; }
};
DSB_HD IdentBand ident_band(uint32_t n, uint32_t m, uint32_t band)
{
	IdentBand b; const int delta = (int)m - (int)n;
	b.delta = delta; b.lo = (delta < 0 ? delta : 0) - (int)band; b.hi = (delta > 0 ? delta : 0) + (int)band; b.W = b.hi - b.lo + 1;
	b.R = 2u * (uint32_t)((b.W + 63) / 64);
	return b;
}

// The plan of a record in checkpoint mode, stated once for the device and for dsb_aln_plan: how a trace place of
// `room` bytes is divided for a pair of n x m bases.  A function of (n, m, band, permille, room) alone, never of the edits.  Sizes in
// bytes: Rb the trace of a generation (the band's 8 * R), C a checkpoint (a whole generation of FR, W + 2 ints), Mv a byte per move
// of the path; the place holds the segment trace (K x Rb), then the checkpoints (n_ck x C), then the moves.  All three are multiples
// of 16.
struct IdentPlan { uint32_t ok, K, n_ck, Rb, C, Mv; };
DSB_HD IdentPlan ident_plan(uint32_t n, uint32_t m, uint32_t band, uint32_t permille, uint64_t room)
{
	IdentPlan p; p.ok = p.K = p.n_ck = 0;
	const IdentBand b = ident_band(n, m, band);
	const uint64_t W = (uint64_t)b.W, Rb = 8ull * b.R;
	const uint64_t ecap = (uint64_t)(n > m ? n : m) * permille / 1000u;
	const uint64_t C = 16u * ((4u * (W + 2u) + 15u) / 16u), Mv = 16u * ((ecap + 15u) / 16u);
	p.Rb = (uint32_t)Rb; p.C = (uint32_t)C; p.Mv = (uint32_t)Mv;
	if (Mv > room) return p;
	const uint64_t A = room - Mv;
	if (ecap * Rb <= A) { p.K = (uint32_t)(ecap ? ecap : 1u); p.ok = 1; return p; }        // one pass, no checkpoint
	const uint64_t K = A / 2u / Rb;
	if (K < 1) return p;
	const uint64_t n_ck = (ecap - 1u) / K;                      // after generations K, 2K, .. < E_cap
	if (n_ck * C > A - K * Rb) return p;
	p.K = (uint32_t)K; p.n_ck = (uint32_t)n_ck; p.ok = 1;
	return p;
}

// Generation e of the recurrence, prev -> cur over the diagonals [klo, khi] of e: lane l takes diagonals klo + l + 64 r.  Returns
// whether diagonal delta reached n (wave-uniform).  TR with tracing (wave-uniform): every lane also holds the 2-bit code of the
// candidate it chose (0 mismatch, 1 a base of T alone, 2 a base of Q alone, 3 none moved; lanes beyond khi: 3), and each round's two
// bit planes (two ballots) go as 16 bytes to gen + 2 * round by one lane.
template <bool TR>
DV bool ident_gen(const IdentSeq &s, const IdentBand b, uint32_t e, const int *prev, int *cur, int lane, bool tracing, uint64_t *gen)
{
	const int n = (int)s.n, m = (int)s.m, delta = b.delta, klo = b.klo(e), khi = b.khi(e);
	bool mine = false;
	for (int k0 = klo; k0 <= khi; k0 += DSB_WAVE) {
		const int k = k0 + lane;
		uint32_t mv = 3;
		if (k <= khi) {
			const int x = k - b.lo + 1;
			const int p = prev[x], pl = prev[x - 1], pr = prev[x + 1];
			int c = p;
			if (p >= 0 && p + 1 <= n && p + 1 + k <= m) { c = p + 1; mv = 0; }
			if (pl >= 0 && pl + k <= m && pl > c) { c = pl; mv = 1; }
			if (pr >= 0 && pr + 1 <= n && pr + 1 > c) { c = pr + 1; mv = 2; }
			if (c >= 0) c = ident_slide(s, c, k);
			cur[x] = c;
			if (k == delta && c >= n) mine = true;
		}
		if constexpr (TR) {
			if (tracing) {                                         // (wave-uniform: all lanes give their bit to both planes)
				const uint64_t b0 = dsb_ballot64((mv & 1u) != 0), b1 = dsb_ballot64((mv & 2u) != 0);
				if (lane == 0) { ulonglong2 v; v.x = b0; v.y = b1; *reinterpret_cast<ulonglong2 *>(gen) = v; }
				gen += 2;
			}
		}
	}
	return dsb_ballot64(mine) != 0;
}

// The initial state, of the forward pass and of a recomputed segment 0: both generations unreached (each with its unreached entry on
// either side of the band), then lane 0 slides on diagonal 0.  Returns what that slide reached, in lane 0 alone.
DV int ident_start(const IdentSeq &s, const IdentBand b, int *prev, int *cur, int lane)
{
	for (int x = lane; x < b.W + 2; x += DSB_WAVE) { prev[x] = IDENT_NEG; cur[x] = IDENT_NEG; }
	wave_sync();
	int v0 = IDENT_NEG;
	if (lane == 0) { v0 = ident_slide(s, 0, 0); prev[1 - b.lo] = v0; }
	return v0;
}

// One wavefront, one pair (all 64 lanes, wave-uniform arguments).  fr: two generations of half ints each, entry k - lo + 1 for
// diagonal k with an unreached entry on either side of the band; both start unreached, and generation e writes the diagonals
// [max(lo, -e), min(hi, e)], a superset of what generation e - 2 wrote into the same half.
// The loops are bounded by E_cap (edits), the band width (rounds) and n, m (slides).  Three compile-time forms:
// IDENT_PLAIN (k_hit_edits / k_pair_edits): the distance alone.
// IDENT_TRACE (k_hit_align / k_pair_align): generation e is traced at trace + (e - 1) * R, R = 16 * ceil(W / 64) bytes --
// while e * R <= room, so that nothing is written beyond the place; after that the pass goes on as the plain form does.
// IDENT_CKPT (k_hit_align_ck / k_pair_align_ck), with a plan: generation e is traced at slot (e - 1) mod K of the
// segment trace, and after a generation with e mod K == 0 and e < E_cap all lanes copy the new generation's W + 2 ints into the next
// checkpoint, between two wave_syncs and before generation e + 1 overwrites slot 0.  Without a plan it runs as the plain form does.
// The plain and the tracing form compile to what they were.
enum { IDENT_PLAIN = 0, IDENT_TRACE = 1, IDENT_CKPT = 2 };
template <int F>
DV dsb_hit_identity ident_wave(const IdentSeq &s, const IdentBand b, uint32_t band, uint32_t permille, int *fr, uint32_t half, int lane, uint64_t *trace, uint64_t room,
                               const IdentPlan *plan)
{
	dsb_hit_identity o; o.edits = 0; o.q_len = s.n; o.t_len = s.m; o.flags = 0;
	const int n = (int)s.n, m = (int)s.m;
	if (!n || !m) { o.flags = DSB_IDENT_EMPTY; return o; }
	if (b.delta > DSB_IDENT_MAX_SKEW || b.delta < -DSB_IDENT_MAX_SKEW) { o.flags = DSB_IDENT_SKEW; return o; }
	const uint32_t ecap = (uint32_t)((uint64_t)(n > m ? n : m) * permille / 1000u);
	int *prev = fr, *cur = fr + half;
	const int v0 = ident_start(s, b, prev, cur, lane);
	bool hit = dsb_ballot64(lane == 0 && b.delta == 0 && v0 >= n) != 0;
	uint32_t e = 0;
	uint32_t slot = 0;                                                  // (IDENT_CKPT) (e - 1) mod K of the generation to come
	int *ck = nullptr;                                                  // (IDENT_CKPT) the next checkpoint
	if constexpr (F == IDENT_CKPT) ck = reinterpret_cast<int *>(trace + ((uint64_t)plan->K * plan->Rb >> 3));
	while (!hit && e < ecap) {
		e++;
		wave_sync();
		if constexpr (F == IDENT_CKPT) {
			const bool tracing = plan->ok != 0;
			hit = ident_gen<true>(s, b, e, prev, cur, lane, tracing, trace + (uint64_t)slot * b.R);
			if (tracing && ++slot == plan->K) {
				slot = 0;
				if (e < ecap) {
					wave_sync();
					for (int x = lane; x < b.W + 2; x += DSB_WAVE) ck[x] = cur[x];
					wave_sync();
					ck += plan->C >> 2;
				}
			}
		} else {
			const bool tracing = F == IDENT_TRACE && (uint64_t)e * b.R * 8u <= room;
			hit = ident_gen<F == IDENT_TRACE>(s, b, e, prev, cur, lane, tracing, F == IDENT_TRACE ? trace + (uint64_t)(e - 1) * b.R : nullptr);
		}
		int *t = prev; prev = cur; cur = t;
	}
	if (hit) { o.edits = e; if (e <= band) o.flags = DSB_IDENT_EXACT; }
	else { o.edits = ecap + 1; o.flags = DSB_IDENT_OVER; }
	return o;
}

// The next entry of a work list for this wavefront: one atomic by lane 0, that lane's value read by all (dsb_shfl, in wave-uniform
// control flow; dsb_wave.h keeps DSB_RFL for values every lane holds).  The loops that call this keep their control flow wave-uniform
// from end to start as well: the record is stored by every lane (the same 16 bytes), not under a second lane test.
DV uint32_t ident_take(unsigned int *work, int lane)
{
	uint32_t w = 0;
	if (lane == 0) w = atomicAdd(work, 1u);
	return dsb_shfl(w, 0);
}

// ---- the path of a record: walk back through the traced moves, replay forward, emit run-length operations ----
// Where a trace arena lies and where operations go (the tracing kernels): wavefront w owns trace[w * room / 8 .. + room / 8)
struct IdentAlnOut { uint64_t *trace; uint64_t room; dsb_hit_alignment *aln; uint32_t *ops; uint64_t ops_cap; unsigned long long *ops_used; };

// the record of a hit without operations, with the flag that says why
DV dsb_hit_alignment ident_no_path(uint32_t flags)
{
	dsb_hit_alignment a; a.ops_off = 0; a.n_ops = a.n_x = a.n_ins = a.n_del = a.pad = 0; a.flags = flags;
	return a;
}

// Appends to a record's operations, merging equal neighbours.  Every lane holds the same state and stores the same word.
struct IdentOps {
	uint32_t *out; uint32_t cnt, op, len;
	DV void put(uint32_t o, uint32_t l)
	{
		if (!l) return;
		if (o == op) { len += l; return; }
		flush(); op = o; len = l;
	}
	DV void flush() { if (len) out[cnt++] = len << 4 | op; len = 0; }
};

// The replay of a walked path, in wave-uniform control flow: the move of generation e is the byte at moves + (e - 1) * step.  The room
// of the record's operations is reserved with one atomic (its bound, 2 E + 1); a move is applied only where the rectangle has the room
// for it, and a replay that does not end on (n, m) gives a record without operations.
DV dsb_hit_alignment ident_replay(const IdentSeq &s, uint32_t E, const uint8_t *moves, uint64_t step, const IdentAlnOut &A, int lane)
{
	dsb_hit_alignment a = ident_no_path(0);
	const int n = (int)s.n, m = (int)s.m;
	const uint64_t need = 2ull * E + 1u;
	uint32_t off_lo = 0, off_hi = 0;
	if (lane == 0) { const unsigned long long at = atomicAdd(A.ops_used, (unsigned long long)need); off_lo = (uint32_t)at; off_hi = (uint32_t)(at >> 32); }
	const uint64_t off = (uint64_t)dsb_shfl(off_hi, 0) << 32 | dsb_shfl(off_lo, 0);
	if (off > A.ops_cap || need > A.ops_cap - off) { a.flags = DSB_ALN_NOROOM; return a; }
	IdentOps w; w.out = A.ops + off; w.cnt = 0; w.op = 0; w.len = 0;
	int i = 0, k = 0;
	bool good = true;
	for (uint32_t e = 1; e <= E && good; e++) {
		const int i2 = (int)DSB_RFL(ident_slide(s, i, k));
		w.put(DSB_ALN_OP_EQ, (uint32_t)(i2 - i)); i = i2;
		const uint32_t mv = DSB_RFL(moves[(uint64_t)(e - 1) * step]);
		if (mv == 1u && i + k < m) { w.put(DSB_ALN_OP_D, 1); k++; a.n_del++; }
		else if (mv == 2u && i < n) { w.put(DSB_ALN_OP_I, 1); i++; k--; a.n_ins++; }
		else if (mv == 0u && i < n && i + k < m) { w.put(DSB_ALN_OP_X, 1); i++; a.n_x++; }
		else good = false;
	}
	if (good) {
		const int i2 = (int)DSB_RFL(ident_slide(s, i, k));
		w.put(DSB_ALN_OP_EQ, (uint32_t)(i2 - i)); i = i2;
		w.flush();
	}
	if (!good || i != n || i + k != m) { a.n_x = a.n_ins = a.n_del = 0; a.flags = DSB_ALN_NOTRACE; return a; }
	a.ops_off = off; a.n_ops = w.cnt; a.flags = DSB_ALN_OPS;
	return a;
}

// The walk back, stated once: the moves of generations e_hi .. e_lo + 1, traced at slot e - 1 - e_lo of seg (R words each), from
// diagonal k on; the move of generation e goes to the byte moves + (e - 1) * step.  Returns the diagonal generation e_lo is left on.
// A step: the diagonal clamped to the generation's own [klo, khi], both planes read (two words), the move taken through DSB_RFL, then
// the byte stored, the same from every lane -- in this order, because in the full mode the byte lands in the 16 bytes just read.
DV int ident_walk_seg(const uint64_t *seg, uint8_t *moves, uint64_t step, const IdentBand b, uint32_t e_lo, uint32_t e_hi, int k)
{
	for (uint32_t e = e_hi; e > e_lo; e--) {
		const int klo = b.klo(e), khi = b.khi(e);
		int x = k - klo;
		if (x > khi - klo) x = khi - klo;
		if (x < 0) x = 0;
		const uint64_t *g = seg + (uint64_t)(e - 1u - e_lo) * b.R + 2u * ((uint32_t)x >> 6);
		const uint64_t b0 = g[0], b1 = g[1];
		const uint32_t mv = DSB_RFL((uint32_t)((b0 >> (x & 63)) & 1u) | (uint32_t)((b1 >> (x & 63)) & 1u) << 1);
		moves[(uint64_t)(e - 1u) * step] = (uint8_t)mv;
		k = klo + x + (mv == 2u ? 1 : 0) - (mv == 1u ? 1 : 0);
	}
	return k;
}

// After ident_wave<IDENT_TRACE> and a wave_sync, in wave-uniform control flow: all lanes run the same steps on the same values (what
// comes from memory goes through DSB_RFL, so the walk and the replay are scalar branches), and the stores are the same bytes from
// every lane.  The walk back reads generation e = edits .. 1 at diagonal k (from d to 0): the whole trace is its one segment, and
// the move area is the trace itself at a step of 8 * R bytes, so a move lies in the first byte of that generation's own 16 bytes --
// read already, and below every generation still to be read.  Index arithmetic alone keeps every access inside the place: e <= edits
// with edits * R <= room, and the diagonal is clamped to the generation's [klo, khi].  The replay applies a move only where the
// rectangle has the room for it and ends on (n, m); a trace that does not (none was seen: the model of tests/align_lib.py asserts it
// cannot happen) gives a record without operations.
// Loops: edits steps each, the slides bounded by n and m; at most 2 * edits + 1 operations, the room reserved with one atomic.
DV dsb_hit_alignment ident_path(const IdentSeq &s, const IdentBand b, const dsb_hit_identity &o, uint64_t *trace, const IdentAlnOut &A, int lane)
{
	if (o.flags & IDENT_BAD) return ident_no_path(DSB_ALN_UNALIGNED);
	const uint32_t E = o.edits;
	if ((uint64_t)E * b.R * 8u > A.room || s.n >= IDENT_MAX_RUN || s.m >= IDENT_MAX_RUN) return ident_no_path(DSB_ALN_NOTRACE);
	uint8_t *moves = reinterpret_cast<uint8_t *>(trace);
	ident_walk_seg(trace, moves, (uint64_t)b.R * 8u, b, 0, E, b.delta);
	wave_sync();
	return ident_replay(s, E, moves, (uint64_t)b.R * 8u, A, lane);
}

// ident_path in checkpoint mode, after ident_wave<IDENT_CKPT> and a wave_sync, in wave-uniform control flow.  At the
// hit the last segment, floor((edits - 1) / K), is still in the segment trace and is walked back as ident_path walks; each earlier
// segment s is recomputed first: prev restored from checkpoint s - 1 (the initial state for s = 0), cur filled with IDENT_NEG -- a
// generation reads up to two diagonals beyond what the one before wrote, which the forward pass has from the arrays' first fill and a
// restore has not --, generations sK + 1 .. (s + 1)K traced again without a hit test, then walked from the diagonal the later segment
// ended on.  The recurrence is deterministic, so these are the moves the forward pass chose.  Every index stays inside the place by
// arithmetic alone: e <= edits <= E_cap <= Mv, the slot is < K, the checkpoint s - 1 < floor((edits - 1) / K) <= n_ck, the diagonal
// is clamped.  The replay is ident_path's, the moves read at byte e - 1 of the move area.
DV dsb_hit_alignment ident_path_ck(const IdentSeq &s, const IdentBand b, const dsb_hit_identity &o, const IdentPlan &pl, int *fr, uint32_t half, uint64_t *trace,
                                   const IdentAlnOut &A, int lane)
{
	if (o.flags & IDENT_BAD) return ident_no_path(DSB_ALN_UNALIGNED);
	if (!pl.ok || s.n >= IDENT_MAX_RUN || s.m >= IDENT_MAX_RUN) return ident_no_path(DSB_ALN_NOTRACE);
	const uint32_t E = o.edits, K = pl.K;
	const int *ckpt = reinterpret_cast<const int *>(trace + ((uint64_t)K * pl.Rb >> 3));
	uint8_t *moves = reinterpret_cast<uint8_t *>(trace) + (uint64_t)K * pl.Rb + (uint64_t)pl.n_ck * pl.C;
	int k = b.delta;
	if (E) {
		uint32_t seg = (E - 1u) / K;
		k = ident_walk_seg(trace, moves, 1u, b, seg * K, E, k);
		while (seg) {
			seg--;
			wave_sync();
			int *prev = fr, *cur = fr + half;
			if (seg) {
				const int *from = ckpt + (uint64_t)(seg - 1u) * (pl.C >> 2);
				for (int x = lane; x < b.W + 2; x += DSB_WAVE) { prev[x] = from[x]; cur[x] = IDENT_NEG; }
			} else
				ident_start(s, b, prev, cur, lane);
			for (uint32_t e = seg * K + 1u; e <= (seg + 1u) * K; e++) {
				wave_sync();
				ident_gen<true>(s, b, e, prev, cur, lane, true, trace + (uint64_t)(e - 1u - seg * K) * b.R);
				int *t = prev; prev = cur; cur = t;
			}
			wave_sync();
			k = ident_walk_seg(trace, moves, 1u, b, seg * K, (seg + 1u) * K, k);
		}
	}
	wave_sync();
	return ident_replay(s, E, moves, 1u, A, lane);
}

// One lane per read, after the batch's last classify work: the records dsb_ref_coverage counts (dsb_sam_counted, among the hits
// dsb_batch_fetch hands out) go into the work list as {hit, read}, in any order -- each record's result depends on itself alone.
__global__ void __launch_bounds__(256) k_ident_list(const DsbReadOut *__restrict__ rout, const DsbHitOut *__restrict__ hout, const DsbCounters *__restrict__ counters,
                                                    uint32_t cap_hout, uint32_t n, uint2 *__restrict__ list, unsigned int *cnt)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const uint32_t nh = dsb_hits_out(counters->hits, cap_hout);
	const DsbReadOut r = rout[i];
	const uint32_t nrec = dsb_hits_cut(r.first, r.n, nh) ? 0u : r.n;
	const dsb_hit *h = reinterpret_cast<const dsb_hit *>(hout + r.first);
	for (uint32_t k = 0; k < nrec; k++)
		if (dsb_sam_counted(h + k, k)) { uint2 w; w.x = r.first + k; w.y = i; list[atomicAdd(cnt, 1u)] = w; }
}

// ---- the record loop, stated once: three forms x two sources ----
// Where the wavefronts work, and with what: wavefront w owns arena[w * stride .. + stride), two generations of stride / 2 ints
struct IdentRun { uint32_t band, permille; int *arena; uint32_t stride; };

// A source says how many entries there are (total), where the work counter is (work), how entry w becomes an IdentSeq and which
// output slot it writes (seq).  The batch's hit list: cnt[0] entries {hit, read} of k_ident_list, the counter in cnt[1]; the interval
// of the hit clamped to its read and its reference, Q on the hit's strand (the reverse strand of a read lies one pad word behind the
// forward one in pk), T in refbin; the slot is the hit's.
struct IdentHits {
	const DsbHitOut *hout; const DsbReadDesc *rd; const uint64_t *pk; const uint8_t *refbin; const DsbRefInfo *refinfo; uint32_t n_ref; const uint2 *list; unsigned int *cnt;
	DV uint32_t total() const { return cnt[0]; }
	DV unsigned int *work() const { return cnt + 1; }
	DV uint32_t seq(uint32_t w, IdentSeq &s) const
	{
		const uint2 it = list[w];
		const DsbHitOut h = hout[it.x];
		const DsbReadDesc d = rd[it.y];
		uint64_t ln = 0, off = 0;
		if (h.ref_ID < n_ref) { const DsbRefInfo ri = refinfo[h.ref_ID]; ln = ri.seq_l; off = ri.seq_offset; }
		const uint32_t qs = h.q_st < d.len ? h.q_st : d.len, qe = h.q_ed < d.len ? h.q_ed : d.len;
		const uint64_t ts = h.t_st < ln ? h.t_st : ln, te = h.t_ed < ln ? h.t_ed : ln;
		s.qw = pk + d.pk_off + (h.direction ? 0u : (d.len + 31u) / 32u + 1u); s.qbase = qs; s.n = qe > qs ? qe - qs : 0u;
		s.tb = refbin; s.tbase = off + ts; s.m = te > ts ? (uint32_t)(te - ts) : 0u;
		return it.x;
	}
};
// The caller's pairs (dsb_ctx_edit_pairs, dsb_ctx_align_pairs): pair w as it was given, into slot w
struct IdentPairs {
	const uint64_t *qw; const uint8_t *tb; const uint64_t *q_off; const uint32_t *q_len; const uint64_t *t_off; const uint32_t *t_len; uint32_t n_pairs; unsigned int *cnt;
	DV uint32_t total() const { return n_pairs; }
	DV unsigned int *work() const { return cnt; }
	DV uint32_t seq(uint32_t w, IdentSeq &s) const
	{
		s.qw = qw; s.qbase = q_off[w]; s.n = q_len[w]; s.tb = tb; s.tbase = t_off[w]; s.m = t_len[w];
		return w;
	}
};

// One wavefront per entry of the source, taken by the work counter until the source is empty.  The grid is as many wavefronts as
// the arena (and with a tracing form the trace arena) has places for.  IDENT_PLAIN: one forward pass, the identity record.
// IDENT_TRACE: the forward pass in the tracing form, then the same wavefront walks back and replays (ident_path); IDENT_CKPT: the
// record's plan divides the wavefront's trace place, the forward pass keeps one segment's trace and the checkpoints, ident_path_ck
// recomputes the earlier segments in the wavefront's own arena place, and a record without a plan runs as the plain form runs it.
// The identity record is the same in all three.  Control flow is wave-uniform from end to start (ident_take): the records are
// stored by every lane, the same bytes.
template <int F, class Src>
DV void ident_records(const Src &src, const IdentRun &r, dsb_hit_identity *rec, const IdentAlnOut &A)
{
	const int lane = (int)(threadIdx.x & 63u);
	const size_t wave = blockIdx.x * 4u + (threadIdx.x >> 6);
	int *fr = r.arena + wave * r.stride;
	uint64_t *trace = nullptr;
	if constexpr (F != IDENT_PLAIN) trace = A.trace + wave * (A.room / 8u);
	const uint32_t total = src.total();
	for (;;) {
		const uint32_t w = ident_take(src.work(), lane);
		if (w >= total) break;
		IdentSeq s;
		const uint32_t at = src.seq(w, s);
		const IdentBand b = ident_band(s.n, s.m, r.band);
		if constexpr (F == IDENT_PLAIN) {
			rec[at] = ident_wave<F>(s, b, r.band, r.permille, fr, r.stride / 2u, lane, nullptr, 0, nullptr);
		} else {
			IdentPlan pl = {};                                      // (IDENT_CKPT alone reads it)
			if constexpr (F == IDENT_CKPT) pl = ident_plan(s.n, s.m, r.band, r.permille, A.room);
			const dsb_hit_identity o = ident_wave<F>(s, b, r.band, r.permille, fr, r.stride / 2u, lane, trace, A.room, &pl);
			wave_sync();
			dsb_hit_alignment a;
			if constexpr (F == IDENT_CKPT) a = ident_path_ck(s, b, o, pl, fr, r.stride / 2u, trace, A, lane);
			else a = ident_path(s, b, o, trace, A, lane);
			rec[at] = o; A.aln[at] = a;
		}
	}
}

// The three kernels of a batch's records (identity_run): --identity alone, with the path kept (dsb_ctx_enable_alignment), and that in
// checkpoint mode (dsb_ctx_alignment_mode).  One parameter list, so that they launch alike; k_hit_edits does not read A.
// The source's pointers are parameters of the kernel, not an IdentHits by value: as members they lose __restrict__, and without it
// the hit kernels take four more vector registers each (32 / 38 / 50).
#define IDENT_HIT_PARAMS const DsbHitOut *__restrict__ hout, const DsbReadDesc *__restrict__ rd, const uint64_t *__restrict__ pk, const uint8_t *__restrict__ refbin, \
	const DsbRefInfo *__restrict__ refinfo, uint32_t n_ref, const uint2 *__restrict__ list, unsigned int *cnt, IdentRun r, dsb_hit_identity *__restrict__ rec, IdentAlnOut A
#define IDENT_HIT_SRC IdentHits{hout, rd, pk, refbin, refinfo, n_ref, list, cnt}
__global__ void __launch_bounds__(256) k_hit_edits(IDENT_HIT_PARAMS) { ident_records<IDENT_PLAIN>(IDENT_HIT_SRC, r, rec, A); }
__global__ void __launch_bounds__(256) k_hit_align(IDENT_HIT_PARAMS) { ident_records<IDENT_TRACE>(IDENT_HIT_SRC, r, rec, A); }
__global__ void __launch_bounds__(256) k_hit_align_ck(IDENT_HIT_PARAMS) { ident_records<IDENT_CKPT>(IDENT_HIT_SRC, r, rec, A); }

// The batch's records into the run's table, behind k_hit_edits on the same stream: one lane per listed record, equal ref_IDs grouped
// inside the wavefront first (as k_lca_count groups taxids), the first lane of a group adding the group's sums.  Integer adds only.
__global__ void __launch_bounds__(256) k_ident_ref(const DsbHitOut *__restrict__ hout, const uint2 *__restrict__ list, const unsigned int *__restrict__ cnt,
                                                   const dsb_hit_identity *__restrict__ rec, uint32_t n_ref, dsb_ref_identity *tab)
{
	const uint32_t lane = threadIdx.x & 63u, total = cnt[0];
	for (uint32_t base = (blockIdx.x * 4u + (threadIdx.x >> 6)) * 64u; base < total; base += gridDim.x * 256u) {
		const uint32_t i = base + lane;
		bool live = i < total;
		uint32_t ref = 0xffffffffu, v[6] = {0, 0, 0, 0, 0, 0};
		if (live) {
			const uint32_t hit = list[i].x;
			ref = hout[hit].ref_ID;
			const dsb_hit_identity r = rec[hit];
			const bool bad = (r.flags & IDENT_BAD) != 0;
			v[0] = bad ? 0u : 1u; v[1] = bad ? 0u : r.q_len; v[2] = bad ? 0u : r.t_len; v[3] = bad ? 0u : r.edits;
			v[4] = (!bad && (r.flags & DSB_IDENT_EXACT)) ? 1u : 0u; v[5] = bad ? 1u : 0u;
			live = ref < n_ref;
		}
		uint64_t left = dsb_ballot64(live);
		while (left) {
			const int src = __builtin_ctzll(left);
			const uint32_t t = dsb_shfl(ref, src);
			const uint64_t grp = dsb_ballot64(live && ref == t);
			unsigned long long sum[6] = {0, 0, 0, 0, 0, 0};
			for (uint64_t g = grp; g; g &= g - 1) {
				const int l = __builtin_ctzll(g);
				for (int f = 0; f < 6; f++) sum[f] += dsb_shfl(v[f], l);
			}
			if ((int)lane == src) {
				unsigned long long *o = reinterpret_cast<unsigned long long *>(tab + t);
				for (int f = 0; f < 6; f++) if (sum[f]) atomicAdd(o + f, sum[f]);
			}
			left &= ~grp;
		}
	}
}

// ---- dsb_ctx_edit_pairs: the caller's codes packed as reads and reference text are, then ident_wave per pair ----
__global__ void __launch_bounds__(256) k_ident_pack_q(const uint8_t *__restrict__ codes, uint64_t n_bases, uint64_t *__restrict__ words, uint64_t n_words)
{
	const uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (w >= n_words) return;
	uint64_t v = 0;
	for (uint32_t b = 0; b < 32; b++) { const uint64_t p = w * 32 + b; v = (v << 2) | (p < n_bases ? codes[p] & 3u : 0u); }
	words[w] = v;
}
__global__ void __launch_bounds__(256) k_ident_pack_t(const uint8_t *__restrict__ codes, uint64_t n_bases, uint8_t *__restrict__ bytes, uint64_t n_bytes)
{
	const uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (w >= n_bytes) return;
	uint32_t v = 0;
	for (uint32_t b = 0; b < 4; b++) { const uint64_t p = w * 4 + b; v = (v << 2) | (p < n_bases ? codes[p] & 3u : 0u); }
	bytes[w] = (uint8_t)v;
}
// the three kernels of the caller's pairs (ident_pairs): what k_hit_edits, k_hit_align and k_hit_align_ck do to a record, on pair w
#define IDENT_PAIR_PARAMS const uint64_t *__restrict__ qw, const uint8_t *__restrict__ tb, const uint64_t *__restrict__ q_off, const uint32_t *__restrict__ q_len, \
	const uint64_t *__restrict__ t_off, const uint32_t *__restrict__ t_len, uint32_t n_pairs, unsigned int *work, IdentRun r, dsb_hit_identity *__restrict__ out, IdentAlnOut A
#define IDENT_PAIR_SRC IdentPairs{qw, tb, q_off, q_len, t_off, t_len, n_pairs, work}
__global__ void __launch_bounds__(256) k_pair_edits(IDENT_PAIR_PARAMS) { ident_records<IDENT_PLAIN>(IDENT_PAIR_SRC, r, out, A); }
__global__ void __launch_bounds__(256) k_pair_align(IDENT_PAIR_PARAMS) { ident_records<IDENT_TRACE>(IDENT_PAIR_SRC, r, out, A); }
__global__ void __launch_bounds__(256) k_pair_align_ck(IDENT_PAIR_PARAMS) { ident_records<IDENT_CKPT>(IDENT_PAIR_SRC, r, out, A); }

// ================================== host side ====================================================
// ints of a wavefront's arena place: two generations of the widest band (|d| <= DSB_IDENT_MAX_SKEW) with its two unreached ends
static uint32_t ident_stride(uint32_t band) { return 2u * (DSB_IDENT_MAX_SKEW + 2u * band + 3u); }
// wavefronts of the grid: eight per compute unit (the kernel waits on dependent loads; 8 x 36 KiB of arena per CU stay in L2)
static int ident_waves(int device, uint32_t *n_waves)
{
	int cus = 0;
	HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
	*n_waves = (uint32_t)(cus > 0 ? cus : 1) * 8u;
	return DSB_OK;
}
// the kernel of a launch site: the plain form, with alignment on the tracing form, and in checkpoint mode the checkpointed one
template <class K> static K ident_kernel(K plain, K trace, K ckpt, bool aln, uint32_t mode) { return !aln ? plain : mode == DSB_ALN_MODE_CHECKPOINT ? ckpt : trace; }
// the ranges of the options, wherever a caller gives them
static bool ident_opts_ok(uint32_t band, uint32_t max_permille) { return band <= DSB_IDENT_MAX_BAND && max_permille >= 1 && max_permille <= 1000; }
static bool trace_kib_ok(uint32_t trace_kib) { return trace_kib >= 1 && trace_kib <= DSB_ALN_TRACE_KIB_MAX; }
static bool aln_mode_ok(uint32_t mode) { return mode == DSB_ALN_MODE_FULL || mode == DSB_ALN_MODE_CHECKPOINT; }

// alignment off: the trace arena, the records and the operation array freed (identity stays as it is)
static void alignment_release(dsb_ctx *c)
{
	DsbIdent &d = c->ident;
	hipFree(d.d_trace); hipFree(d.d_aln); hipFree(d.d_ops); hipFree(d.d_ops_used);
	d.d_trace = nullptr; d.d_aln = nullptr; d.d_ops = nullptr; d.d_ops_used = nullptr;
	d.cap_aln = d.cap_ops = 0; d.trace_kib = 0; d.aln_mode = DSB_ALN_MODE_FULL; d.ops_fixed = d.ops_room = 0; d.aln_run = false;
	std::vector<dsb_hit_alignment>().swap(d.h_aln); std::vector<uint32_t>().swap(d.h_ops);
}

void identity_release(dsb_ctx *c)
{
	alignment_release(c);
	hipFree(c->ident.d_rec); hipFree(c->ident.d_list); hipFree(c->ident.d_cnt); hipFree(c->ident.d_arena); hipFree(c->ident.d_tab);
	c->ident = DsbIdent();
}

extern "C" int dsb_ctx_reset_identity(dsb_ctx *c)
{
	if (!c || !c->ident.d_tab) return DSB_EINVAL;
	HIPCHK(hipSetDevice(c->device));
	HIPCHK(hipMemsetAsync(c->ident.d_tab, 0, (size_t)dsb_index_n_ref(c->idx) * sizeof(dsb_ref_identity) + 8, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return DSB_OK;
}

extern "C" int dsb_ctx_enable_identity(dsb_ctx *c, int on, uint32_t band, uint32_t max_permille)
{
	if (!c) return DSB_EINVAL;
	if (on && band == 0 && max_permille == 0) { band = DSB_IDENT_BAND_DEFAULT; max_permille = DSB_IDENT_PERMILLE_DEFAULT; }
	if (on && !ident_opts_ok(band, max_permille)) return DSB_EINVAL;
	HIPCHK(hipSetDevice(c->device));
	HIPCHK(hipStreamSynchronize(c->stream));
	if (on && c->ident.d_tab && c->ident.band == band) { c->ident.permille = max_permille; return dsb_ctx_reset_identity(c); }
	identity_release(c);
	if (!on) return DSB_OK;
	DsbIdent &d = c->ident;
	if (int rc = ident_waves(c->device, &d.n_waves)) return rc;
	d.stride = ident_stride(band);
	const size_t n_ref = (size_t)dsb_index_n_ref(c->idx);
	if (hipMalloc((void **)&d.d_tab, n_ref * sizeof(dsb_ref_identity) + 8) != hipSuccess || hipMalloc((void **)&d.d_cnt, 2 * sizeof(unsigned int)) != hipSuccess ||
	    hipMalloc((void **)&d.d_arena, (size_t)d.n_waves * d.stride * sizeof(int)) != hipSuccess ||
	    grow(&d.d_rec, &d.cap_rec, c->cap_hout) || grow(&d.d_list, &d.cap_list, c->cap_hout)) {
		identity_release(c); (void)hipGetLastError(); return DSB_ENOMEM;
	}
	d.band = band; d.permille = max_permille;
	return dsb_ctx_reset_identity(c);
}

extern "C" int dsb_ctx_enable_alignment(dsb_ctx *c, int on, uint32_t trace_kib, uint64_t ops_cap)
{
	if (!c) return DSB_EINVAL;
	if (on && !c->ident.d_tab) return DSB_EINVAL;
	if (on && trace_kib == 0) trace_kib = DSB_ALN_TRACE_KIB_DEFAULT;
	if (on && !trace_kib_ok(trace_kib)) return DSB_EINVAL;
	HIPCHK(hipSetDevice(c->device));
	HIPCHK(hipStreamSynchronize(c->stream));
	alignment_release(c);
	if (!on) return DSB_OK;
	DsbIdent &d = c->ident;
	if (hipMalloc((void **)&d.d_trace, (size_t)d.n_waves * trace_kib * 1024u) != hipSuccess || hipMalloc((void **)&d.d_ops_used, sizeof(unsigned long long)) != hipSuccess ||
	    grow(&d.d_aln, &d.cap_aln, c->cap_hout)) {
		alignment_release(c); (void)hipGetLastError(); return DSB_ENOMEM;
	}
	d.trace_kib = trace_kib; d.ops_fixed = ops_cap;               // (the mode: alignment_release left it at FULL)
	return DSB_OK;
}

extern "C" int dsb_ctx_alignment_mode(dsb_ctx *c, uint32_t mode)
{
	if (!c || !c->ident.d_trace || !aln_mode_ok(mode)) return DSB_EINVAL;
	c->ident.aln_mode = mode;                                    // (host state alone: the next batch's launch reads it)
	return DSB_OK;
}

extern "C" int dsb_aln_plan(uint32_t n, uint32_t m, uint32_t band, uint32_t max_permille, uint32_t trace_kib, uint32_t *K, uint32_t *n_ckpt)
{
	if (!K || !n_ckpt || n >= IDENT_MAX_RUN || m >= IDENT_MAX_RUN || !ident_opts_ok(band, max_permille) || !trace_kib_ok(trace_kib)) return DSB_EINVAL;
	const IdentPlan p = ident_plan(n, m, band, max_permille, (uint64_t)trace_kib * 1024u);
	*K = p.K; *n_ckpt = p.n_ck;
	return p.ok ? 1 : 0;
}

int identity_run(dsb_ctx *c, const DsbBatchView &b)
{
	DsbIdent &d = c->ident;
	// one record and one list entry per place of the hit buffer (it may have been regrown by this batch)
	if (grow(&d.d_rec, &d.cap_rec, b.cap_hout) || grow(&d.d_list, &d.cap_list, b.cap_hout)) return DSB_ENOMEM;
	HIPCHK(hipMemsetAsync(d.d_rec, 0, b.cap_hout * sizeof(dsb_hit_identity), b.st));
	HIPCHK(hipMemsetAsync(d.d_cnt, 0, 2 * sizeof(unsigned int), b.st));
	hipLaunchKernelGGL(k_ident_list, dim3((b.n + 255) / 256), dim3(256), 0, b.st, b.rout, b.hout, b.counters, (uint32_t)b.cap_hout, b.n, d.d_list, d.d_cnt);
	IdentAlnOut A = {};
	if (d.d_trace) {
		// alignment on: the records' room and the batch's operation array (automatic: an operation per base and four per hit place)
		d.ops_room = d.ops_fixed ? d.ops_fixed : c->in[c->cur].total_bases + 4ull * b.cap_hout;
		if (grow(&d.d_aln, &d.cap_aln, b.cap_hout) || grow(&d.d_ops, &d.cap_ops, (size_t)d.ops_room)) return DSB_ENOMEM;
		HIPCHK(hipMemsetAsync(d.d_aln, 0, b.cap_hout * sizeof(dsb_hit_alignment), b.st));
		HIPCHK(hipMemsetAsync(d.d_ops_used, 0, sizeof(unsigned long long), b.st));
		A.trace = d.d_trace; A.room = (uint64_t)d.trace_kib * 1024u; A.aln = d.d_aln; A.ops = d.d_ops; A.ops_cap = d.ops_room; A.ops_used = d.d_ops_used;
		d.aln_run = true;
	}
	const IdentRun r = {d.band, d.permille, d.d_arena, d.stride};
	hipLaunchKernelGGL(ident_kernel(k_hit_edits, k_hit_align, k_hit_align_ck, d.d_trace != nullptr, d.aln_mode), dim3(d.n_waves / 4), dim3(256), 0, b.st, b.hout, b.rd, b.pk,
	                   c->dx.refbin, c->dx.refinfo, (uint32_t)dsb_index_n_ref(c->idx), (const uint2 *)d.d_list, d.d_cnt, r, d.d_rec, A);
	const size_t ref_blocks = std::min<size_t>((b.cap_hout + 255) / 256, 1024);
	hipLaunchKernelGGL(k_ident_ref, dim3((unsigned)(ref_blocks ? ref_blocks : 1)), dim3(256), 0, b.st, b.hout, (const uint2 *)d.d_list, (const unsigned int *)d.d_cnt,
	                   (const dsb_hit_identity *)d.d_rec, (uint32_t)dsb_index_n_ref(c->idx), d.d_tab);
	d.run = true;
	return DSB_OK;
}

// The used part of an operation array of `room` operations, queued on st: its length has to be known before the copy is queued, so
// it is read first (8 bytes and one wait on the stream).  to(used) gives the place the operations go to.
template <class To>
static int ident_fetch_ops(hipStream_t st, const uint32_t *d_ops, const unsigned long long *d_used, uint64_t room, uint64_t *n_used, To to)
{
	unsigned long long used = 0;
	HIPCHK(hipMemcpyAsync(&used, d_used, sizeof used, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	if (used > room) used = room;                            // (reservations that did not fit moved the counter too)
	uint32_t *h_ops = to((size_t)used);
	if (used) HIPCHK(hipMemcpyAsync(h_ops, d_ops, (size_t)used * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
	*n_used = used;
	return DSB_OK;
}

int identity_fetch_queue(dsb_ctx *c, size_t n_hits)
{
	c->ident.h_rec.resize(n_hits);
	if (n_hits) HIPCHK(hipMemcpyAsync(c->ident.h_rec.data(), c->ident.d_rec, n_hits * sizeof(dsb_hit_identity), hipMemcpyDeviceToHost, c->stream));
	if (!c->ident.aln_run) return DSB_OK;
	// alignment: the records, and the used part of the operation array alone (the stream's one more wait comes after the batch's
	// counters have already been waited for on it)
	DsbIdent &d = c->ident;
	d.h_aln.resize(n_hits); d.h_ops.clear();
	if (!n_hits) return DSB_OK;
	uint64_t used = 0;
	HIPCHK(hipMemcpyAsync(d.h_aln.data(), d.d_aln, n_hits * sizeof(dsb_hit_alignment), hipMemcpyDeviceToHost, c->stream));
	return ident_fetch_ops(c->stream, d.d_ops, d.d_ops_used, d.ops_room, &used, [&d](size_t n) { d.h_ops.resize(n); return d.h_ops.data(); });
}

extern "C" int dsb_batch_alignment(dsb_ctx *c, const dsb_hit_alignment **recs, const uint32_t **ops, uint64_t *n_ops)
{
	if (!c || !recs || !ops || !n_ops || !c->ident.d_trace || !c->ident.aln_run) return DSB_EINVAL;
	if (!c->ident.done) { dsb_result r; int rc = dsb_batch_fetch(c, &r); if (rc && rc != DSB_ECAP) return rc; }
	*recs = c->ident.h_aln.data(); *ops = c->ident.h_ops.data(); *n_ops = c->ident.h_ops.size();
	return DSB_OK;
}

extern "C" int dsb_batch_identity(dsb_ctx *c, const dsb_hit_identity **out)
{
	if (!c || !out || !c->ident.d_tab || !c->ident.run) return DSB_EINVAL;
	if (!c->ident.done) { dsb_result r; int rc = dsb_batch_fetch(c, &r); if (rc && rc != DSB_ECAP) return rc; }
	*out = c->ident.h_rec.data();
	return DSB_OK;
}

extern "C" int dsb_ctx_identity(dsb_ctx *c, dsb_ref_identity *out)
{
	if (!c || !out || !c->ident.d_tab) return DSB_EINVAL;
	HIPCHK(hipSetDevice(c->device));
	const size_t n_ref = (size_t)dsb_index_n_ref(c->idx);
	if (n_ref) HIPCHK(hipMemcpyAsync(out, c->ident.d_tab, n_ref * sizeof(dsb_ref_identity), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	return DSB_OK;
}

extern "C" int dsb_multi_enable_identity(dsb_multi *m, int on, uint32_t band, uint32_t max_permille)
{
	if (!m) return DSB_EINVAL;
	m->ident_on = m->ident_ok = false;
	for (dsb_ctx *c : m->ctx) {
		int rc = dsb_ctx_enable_identity(c, on, band, max_permille);
		if (rc) { for (dsb_ctx *d : m->ctx) dsb_ctx_enable_identity(d, 0, 0, 0); return rc; }
	}
	m->ident_on = on != 0;
	for (dsb_ctx *c : m->ctx) if (!c->ident.d_trace) m->aln_on = false;      // (identity off, or on with another band: alignment went with it)
	m->aln_ok = false;
	return DSB_OK;
}

extern "C" int dsb_multi_enable_alignment(dsb_multi *m, int on, uint32_t trace_kib, uint64_t ops_cap)
{
	if (!m) return DSB_EINVAL;
	m->aln_on = m->aln_ok = false;
	for (dsb_ctx *c : m->ctx) {
		int rc = dsb_ctx_enable_alignment(c, on, trace_kib, ops_cap);
		if (rc) { for (dsb_ctx *d : m->ctx) dsb_ctx_enable_alignment(d, 0, 0, 0); return rc; }
	}
	m->aln_on = on != 0;
	return DSB_OK;
}

extern "C" int dsb_multi_alignment_mode(dsb_multi *m, uint32_t mode)
{
	if (!m || !m->aln_on || !aln_mode_ok(mode)) return DSB_EINVAL;
	for (dsb_ctx *c : m->ctx) if (int rc = dsb_ctx_alignment_mode(c, mode)) return rc;
	return DSB_OK;
}

extern "C" int dsb_multi_alignment(dsb_multi *m, const dsb_hit_alignment **recs, const uint32_t **ops, uint64_t *n_ops)
{
	if (!m || !recs || !ops || !n_ops || !m->aln_on || !m->aln_ok) return DSB_EINVAL;
	*recs = m->aln.data(); *ops = m->aln_ops.data(); *n_ops = m->aln_ops.size();
	return DSB_OK;
}

extern "C" int dsb_multi_identity(dsb_multi *m, const dsb_hit_identity **out)
{
	if (!m || !out || !m->ident_on || !m->ident_ok) return DSB_EINVAL;
	*out = m->ident.data();
	return DSB_OK;
}

// the contexts' tables added on the host (48 bytes per reference and context)
extern "C" int dsb_multi_ref_identity(dsb_multi *m, dsb_ref_identity *out)
{
	if (!m || !out || m->ctx.empty()) return DSB_EINVAL;
	const size_t n_ref = (size_t)dsb_index_n_ref(m->idx);
	std::vector<dsb_ref_identity> t(n_ref);
	memset(out, 0, n_ref * sizeof *out);
	for (dsb_ctx *c : m->ctx) {
		if (int rc = dsb_ctx_identity(c, t.data())) return rc;
		for (size_t r = 0; r < n_ref; r++) {
			out[r].records += t[r].records; out[r].q_bases += t[r].q_bases; out[r].t_bases += t[r].t_bases;
			out[r].edits += t[r].edits; out[r].exact += t[r].exact; out[r].unaligned += t[r].unaligned;
		}
	}
	return DSB_OK;
}

// dsb_ctx_edit_pairs, and with al dsb_ctx_align_pairs(_mode): the same packing and the same phases, k_pair_edits or a tracing twin
struct IdentPairsAln { uint32_t trace_kib, mode; dsb_hit_alignment *aln_out; uint32_t *ops_out; uint64_t ops_cap; uint64_t *ops_used; };
static int ident_pairs(dsb_ctx *c, const uint8_t *q_codes, const uint64_t *q_off, const uint32_t *q_len, const uint8_t *t_codes, const uint64_t *t_off,
                       const uint32_t *t_len, size_t n_pairs, uint32_t band, uint32_t max_permille, dsb_hit_identity *out, const IdentPairsAln *al)
{
	if (!c || !ident_opts_ok(band, max_permille) || n_pairs > 0xffffffffu) return DSB_EINVAL;
	if (al && (!al->ops_used || !trace_kib_ok(al->trace_kib) || !aln_mode_ok(al->mode))) return DSB_EINVAL;
	if (al) *al->ops_used = 0;
	if (!n_pairs) return DSB_OK;
	if (!q_codes || !q_off || !q_len || !t_codes || !t_off || !t_len || !out || (al && (!al->aln_out || (!al->ops_out && al->ops_cap)))) return DSB_EINVAL;
	const uint32_t max_len = al ? IDENT_MAX_RUN - 1u : IDENT_MAX_LEN;
	uint64_t nq = 0, nt = 0;
	for (size_t p = 0; p < n_pairs; p++) {
		if (q_len[p] > max_len || t_len[p] > max_len || q_off[p] > IDENT_MAX_OFF || t_off[p] > IDENT_MAX_OFF) return DSB_EINVAL;   // (the sums below cannot wrap)
		nq = std::max(nq, q_off[p] + q_len[p]); nt = std::max(nt, t_off[p] + t_len[p]);
	}
	HIPCHK(hipSetDevice(c->device));
	uint32_t n_waves = 0;
	if (int rc = ident_waves(c->device, &n_waves)) return rc;
	n_waves = (uint32_t)std::min<size_t>(n_waves, (n_pairs + 3) / 4 * 4);
	const uint32_t stride = ident_stride(band);
	const uint64_t n_words = (nq + 31) / 32 + 1, n_bytes = (nt + 3) / 4 + IDENT_T_PAD;
	struct Bufs { std::vector<void *> p; ~Bufs() { for (void *q : p) hipFree(q); }
	              void *get(size_t bytes) { void *q = nullptr; if (hipMalloc(&q, bytes ? bytes : 1) != hipSuccess) { (void)hipGetLastError(); return nullptr; } p.push_back(q); return q; } } T;
	uint8_t *d_qc = (uint8_t *)T.get(nq), *d_tc = (uint8_t *)T.get(nt), *d_tb = (uint8_t *)T.get(n_bytes);
	uint64_t *d_qw = (uint64_t *)T.get(n_words * 8), *d_qo = (uint64_t *)T.get(n_pairs * 8), *d_to = (uint64_t *)T.get(n_pairs * 8);
	uint32_t *d_ql = (uint32_t *)T.get(n_pairs * 4), *d_tl = (uint32_t *)T.get(n_pairs * 4);
	unsigned int *d_work = (unsigned int *)T.get(sizeof(unsigned int));
	int *d_arena = (int *)T.get((size_t)n_waves * stride * sizeof(int));
	dsb_hit_identity *d_out = (dsb_hit_identity *)T.get(n_pairs * sizeof(dsb_hit_identity));
	if (!d_qc || !d_tc || !d_tb || !d_qw || !d_qo || !d_to || !d_ql || !d_tl || !d_work || !d_arena || !d_out) return DSB_ENOMEM;
	IdentAlnOut A; memset(&A, 0, sizeof A);
	if (al) {
		A.room = (uint64_t)al->trace_kib * 1024u; A.ops_cap = al->ops_cap;
		A.trace = (uint64_t *)T.get((size_t)n_waves * A.room); A.aln = (dsb_hit_alignment *)T.get(n_pairs * sizeof(dsb_hit_alignment));
		A.ops = (uint32_t *)T.get((size_t)al->ops_cap * sizeof(uint32_t)); A.ops_used = (unsigned long long *)T.get(sizeof(unsigned long long));
		if (!A.trace || !A.aln || !A.ops || !A.ops_used) return DSB_ENOMEM;
	}
	hipStream_t st = c->stream;
	if (nq) HIPCHK(hipMemcpyAsync(d_qc, q_codes, nq, hipMemcpyHostToDevice, st));
	if (nt) HIPCHK(hipMemcpyAsync(d_tc, t_codes, nt, hipMemcpyHostToDevice, st));
	HIPCHK(hipMemcpyAsync(d_qo, q_off, n_pairs * 8, hipMemcpyHostToDevice, st));
	HIPCHK(hipMemcpyAsync(d_to, t_off, n_pairs * 8, hipMemcpyHostToDevice, st));
	HIPCHK(hipMemcpyAsync(d_ql, q_len, n_pairs * 4, hipMemcpyHostToDevice, st));
	HIPCHK(hipMemcpyAsync(d_tl, t_len, n_pairs * 4, hipMemcpyHostToDevice, st));
	HIPCHK(hipMemsetAsync(d_work, 0, sizeof(unsigned int), st));
	hipLaunchKernelGGL(k_ident_pack_q, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, st, (const uint8_t *)d_qc, nq, d_qw, n_words);
	hipLaunchKernelGGL(k_ident_pack_t, dim3((unsigned)((n_bytes + 255) / 256)), dim3(256), 0, st, (const uint8_t *)d_tc, nt, d_tb, n_bytes);
	if (al) HIPCHK(hipMemsetAsync(A.ops_used, 0, sizeof(unsigned long long), st));
	const IdentRun r = {band, max_permille, d_arena, stride};
	hipLaunchKernelGGL(ident_kernel(k_pair_edits, k_pair_align, k_pair_align_ck, al != nullptr, al ? al->mode : 0u), dim3(n_waves / 4), dim3(256), 0, st, (const uint64_t *)d_qw,
	                   (const uint8_t *)d_tb, (const uint64_t *)d_qo, (const uint32_t *)d_ql, (const uint64_t *)d_to, (const uint32_t *)d_tl, (uint32_t)n_pairs, d_work, r, d_out, A);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(out, d_out, n_pairs * sizeof(dsb_hit_identity), hipMemcpyDeviceToHost, st));
	if (al) {
		HIPCHK(hipMemcpyAsync(al->aln_out, A.aln, n_pairs * sizeof(dsb_hit_alignment), hipMemcpyDeviceToHost, st));
		if (int rc = ident_fetch_ops(st, A.ops, A.ops_used, al->ops_cap, al->ops_used, [al](size_t) { return al->ops_out; })) return rc;
	}
	HIPCHK(hipStreamSynchronize(st));
	return DSB_OK;
}

extern "C" int dsb_ctx_edit_pairs(dsb_ctx *c, const uint8_t *q_codes, const uint64_t *q_off, const uint32_t *q_len, const uint8_t *t_codes, const uint64_t *t_off,
                                  const uint32_t *t_len, size_t n_pairs, uint32_t band, uint32_t max_permille, dsb_hit_identity *out)
{
	return ident_pairs(c, q_codes, q_off, q_len, t_codes, t_off, t_len, n_pairs, band, max_permille, out, nullptr);
}

extern "C" int dsb_ctx_align_pairs(dsb_ctx *c, const uint8_t *q_codes, const uint64_t *q_off, const uint32_t *q_len, const uint8_t *t_codes, const uint64_t *t_off,
                                   const uint32_t *t_len, size_t n_pairs, uint32_t band, uint32_t max_permille, uint32_t trace_kib,
                                   dsb_hit_identity *ident_out, dsb_hit_alignment *aln_out, uint32_t *ops_out, uint64_t ops_cap, uint64_t *ops_used)
{
	return dsb_ctx_align_pairs_mode(c, q_codes, q_off, q_len, t_codes, t_off, t_len, n_pairs, band, max_permille, trace_kib, DSB_ALN_MODE_FULL, ident_out, aln_out, ops_out,
	                                ops_cap, ops_used);
}

extern "C" int dsb_ctx_align_pairs_mode(dsb_ctx *c, const uint8_t *q_codes, const uint64_t *q_off, const uint32_t *q_len, const uint8_t *t_codes, const uint64_t *t_off,
                                        const uint32_t *t_len, size_t n_pairs, uint32_t band, uint32_t max_permille, uint32_t trace_kib, uint32_t mode,
                                        dsb_hit_identity *ident_out, dsb_hit_alignment *aln_out, uint32_t *ops_out, uint64_t ops_cap, uint64_t *ops_used)
{
	if (trace_kib == 0) trace_kib = DSB_ALN_TRACE_KIB_DEFAULT;
	IdentPairsAln al; al.trace_kib = trace_kib; al.mode = mode; al.aln_out = aln_out; al.ops_out = ops_out; al.ops_cap = ops_cap; al.ops_used = ops_used;
	return ident_pairs(c, q_codes, q_off, q_len, t_codes, t_off, t_len, n_pairs, band, max_permille, ident_out, &al);
}
