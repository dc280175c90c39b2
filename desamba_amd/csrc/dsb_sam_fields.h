// The fields of output_one_result_sam (src/cly_mt.c:245-344) that the taxonomy report reads back: which records are
// printed, the MAPQ of each, and the read length `deSAMBA analysis` takes from a printed CIGAR.  One definition for the
// SAM writer (dsb_format_sam, dsb_index.cpp) and for k_read_taxon (dsb_reductions.hip), so that the two cannot drift apart.
#pragma once
#include <stdint.h>
#include "../../include/desamba_amd.h"

#if defined(__HIPCC__)
#define DSB_HD __host__ __device__ __forceinline__
#else
#define DSB_HD static inline
#endif

// The records dsb_batch_fetch hands out: the first nh = dsb_hits_out(hits counted, the hit buffer's capacity) of the buffer, and
// of a read only records that lie among them -- a read whose records reach further (dsb_hits_cut) gets none.  One rule for the
// fetch and for the kernels that read a batch's hits after its last classify launch (dsb_reductions.hip).
DSB_HD uint32_t dsb_hits_out(uint32_t counted, uint64_t cap) { return counted < cap ? counted : (uint32_t)cap; }
DSB_HD bool dsb_hits_cut(uint32_t first, uint32_t n, uint64_t nh) { return (uint64_t)first + n > nh; }

// MAPQ of the primary record; supplementary records print min(it, 30), secondary ones 0.  (Unsigned difference, as
// the reference computes it: the hits are in score order, so it does not wrap.)
DSB_HD int dsb_sam_mapq_pri(const dsb_hit *h, uint32_t n)
{
	if (n == 1 || (h[0].sum_score - h[1].sum_score > 5)) return 30;
	return (int)((h[0].sum_score - h[1].sum_score) << 2);
}

// record i >= 1 of a read: printed in pass 0 (supplementary: pri_index 0) or pass 1 (secondary: pri_index 1..max_sec)
DSB_HD bool dsb_sam_shown(const dsb_hit *c, int pass, int max_sec)
{
	return pass == 0 ? c->pri_index == 0 : (c->pri_index > 0 && c->pri_index <= max_sec);
}

// MAPQ of a supplementary record (pass 0, FLAG 0x800), from the primary's
DSB_HD int dsb_sam_mapq_sup(int mapq_pri) { return mapq_pri < 30 ? mapq_pri : 30; }

// record i of a read is printed without FLAG 0x100: the primary (i = 0) or a supplementary record.  The records the
// per-reference coverage counts (k_ref_cover), whatever max_sec is.
DSB_HD bool dsb_sam_counted(const dsb_hit *c, uint32_t i) { return i == 0 || dsb_sam_shown(c, 0, 0); }

// the three numbers of a record's CIGAR as the writer prints them with %d: "<v0>S<v1>M<v2>S" (primary, secondary) or
// "<v0>H<v1>M<v2>H" (supplementary)
DSB_HD void dsb_sam_cigar(const dsb_hit *c, uint32_t read_l, int v[3])
{
	v[0] = (int)c->q_st; v[1] = (int)(c->q_ed - c->q_st); v[2] = (int)(read_l - c->q_ed);
}

// a CIGAR number counted back the way analysis reads it: digits accumulate, a '-' starts the number over
DSB_HD uint32_t dsb_cigar_num(int v) { return v < 0 ? 0u - (uint32_t)v : (uint32_t)v; }

// read length of a record as analysis counts its CIGAR (M/I/S/X): all three numbers of an S-clipped CIGAR, only the M
// of an H-clipped one.  So "0S8154M-1S" counts 8155.
DSB_HD uint32_t dsb_sam_cigar_len(const dsb_hit *c, uint32_t read_l, bool hard_clips)
{
	int v[3]; dsb_sam_cigar(c, read_l, v);
	return hard_clips ? dsb_cigar_num(v[1]) : dsb_cigar_num(v[0]) + dsb_cigar_num(v[1]) + dsb_cigar_num(v[2]);
}
