/* TEST INFRASTRUCTURE -- CPU restatement ("oracle") of deSAMBA's classify hot path.
 *
 * This is the checker, not the product: only tests/, __graft_entry__.smoke() and
 * bench.py's cpu_baseline leg may load it.  Nothing under desamba_amd/ links it.
 *
 * Parity status: PINNED.  The restatement reproduces the reference's own demo
 * run byte for byte (SAM md5 1da908b61be240c40334b58d3c12ba2a) and
 * is cross-checked against the compiled reference (oracle/_ref/deSAMBA) on
 * synthetic reads (tests/test_oracle_golden.py::test_against_live_reference).
 *
 * Canonical semantics at the reference's undefined-behaviour sites (SURVEY.md
 * section 8 a-UB), chosen so the result of a read never depends on earlier reads:
 *   U1  query bytes left of the forward strand read as 0 ('A'); the forward
 *       strand is followed by the reverse strand (as in the reference buffer);
 *       bytes right of the reverse strand never match (value 5).
 *   U2  bytes of a reference window that the reference did not load (stale
 *       stack in src/cly.c:2472,2542,2688) hold the value 4: they match nothing and
 *       enter 9-mer arithmetic as the literal 4.
 *   U3  2-bit reference text beyond its end reads as 0.
 *   U5  lv_extd (src/cly.c:594) can read the byte in front of either string: for a
 *       string inside the read buffer that is the previous base (defined); for
 *       the local 13-byte buffers of map_seed/get_new_ed it never matches.
 *   U6  a reference window whose start offset lies beyond the 2-bit text reads as all 0 ('A').  The reference computes
 *       window offsets in unsigned 32-bit arithmetic (src/cly.c:2727,2742: c_t_offset - max_search_ref wraps when a
 *       hit hangs over the start of a reference) and then reads up to 1 GB behind the text: a segmentation fault on
 *       small indexes, arbitrary bytes on large ones (found with a read running over the start of its reference).
 *   U4  max_read_l (src/cly.c:2958) is the prefix maximum of read length in
 *       input order (= the reference's `-t 1` behaviour).
 *   U7  the per-thread 9-mer table of build_hash_table_M2 has room for every read: the reference allocates 2^20 nodes
 *       (src/cly_mt.c:540-541), a read of L bases takes 2^18 heads + L nodes (src/cly.c:2173-2224), so the stock binary
 *       writes behind the table for reads longer than 786432 bases.  2^24 nodes here and in the UB-pinned build
 *       (tests/golden/synth/ultralong.fq.gz: one read of 0.87 Mbp).
 */
#ifndef DSB_ORACLE_H
#define DSB_ORACLE_H
#include <stdint.h>
#include <stdio.h>

typedef struct { uint32_t unitig_ID, offset; } ora_sa_t;          /* src/bwt.h:10-13 */
typedef struct { uint32_t ref_list, length; } ora_unitig_t;       /* src/idx.h:21-25 */
typedef struct { char name[128]; uint64_t seq_l, seq_offset; } ora_refinfo_t; /* src/idx.h:15-19 */

typedef struct {
	/* FM index, src/bwt.c:68-104 */
	uint64_t byteLen; uint8_t *bwt_occ; uint64_t rank[6]; uint64_t *hash_index;
	uint8_t *acgt[5]; ora_sa_t *sa; uint64_t sa_size; uint64_t dollar_pos;
	/* exist-kmer filter, src/idx.c:966-982,1112-1118 */
	uint64_t ek_size, ek_mask; int ek_len, single_base_max; uint8_t *ek0, *ek1;
	/* unitigs / references, src/idx.c:1123-1159 */
	uint64_t n_uni; ora_unitig_t *uni;
	uint64_t n_refbin; uint8_t *refbin;
	uint64_t n_ref; ora_refinfo_t *ref;
	uint64_t n_refpos; uint64_t *refpos;   /* bit-field {global_offset:40, ref_ID:23, direction:1} */
	/* MAPQ tables, src/cly_mt.c:413-437 */
	int Q_MEM[2000]; int Q_LV[20][20];
	int filter_min_length, filter_min_score, filter_min_score_LV3;
} ora_idx_t;

/* one output hit == the fields of chain_item the SAM writer consumes (src/cly.h:69-89) */
typedef struct {
	uint32_t ref_ID; uint32_t t_st, t_ed, q_st, q_ed; uint32_t sum_score; uint32_t indel;
	uint8_t direction, primary, pri_index, pad;
} ora_hit_t;

typedef struct ora_ctx ora_ctx_t;

/* stage dump of one strand's seed list (a-3), for stage-level parity of the seed-lookup kernel */
typedef struct { uint32_t offset, len; uint8_t top; } ora_seed_t;

typedef struct { uint32_t index_in_read, ref_ID, ref_offset; int16_t score; uint16_t mtch_len, seed_ID; uint8_t direction, useless, left_len, left_ED, rigt_len, rigt_ED; } ora_anchor_t;

#ifdef __cplusplus
extern "C" {
#endif
int  ora_idx_load(ora_idx_t *idx, const char *dir, int min_len, int min_score);
void ora_idx_free(ora_idx_t *idx);
ora_ctx_t *ora_ctx_new(void);
void ora_ctx_free(ora_ctx_t *c);
/* classify one read (ASCII, length len).  Returns number of hits; *hits points into ctx storage
 * valid until the next call.  max_read_l is carried in the ctx (U4). */
int  ora_classify(ora_ctx_t *c, const ora_idx_t *idx, const char *seq, uint32_t len, const ora_hit_t **hits);
void ora_ctx_reset_history(ora_ctx_t *c);
void ora_ctx_set_history(ora_ctx_t *c, int max_read_l);
/* stage dumps from the last ora_classify call */
int  ora_last_seeds(const ora_ctx_t *c, int strand /*1=F,0=R*/, const ora_seed_t **seeds, uint32_t *total_score);
/* exist-kmer hit bit of every window of a strand (1 byte per window), for the probe kernel's parity */
void ora_exist_bits(const ora_idx_t *idx, const char *seq, uint32_t len, int strand, uint8_t *out);
/* a-3 behind the table probes (tests/test_stage_seed.py): search_exist_kmer_M2 and the top marking of get_seed_vector_M2 as ora_classify runs
 * them, on one hit byte per window of a strand (1 = forward, 0 = reverse); returns the number of seeds (sv: room for n / 3 + 2), or -1 */
int  ora_seed_stage(const uint8_t *hit, uint32_t n, int direction, ora_seed_t *sv, uint32_t max_sv, uint32_t *total_score);
/* work counters of the last call: P0,P1,OCC,SA,RW,MEMS */
int  ora_last_anchors(const ora_ctx_t *c, ora_anchor_t *out, int max);
void ora_last_counters(const ora_ctx_t *c, uint64_t out[8]);
/* SAM record(s) of one read, exactly src/cly_mt.c:245-344 */
void ora_write_sam(FILE *f, const ora_idx_t *idx, const char *name, const char *seq, const char *qual,
                   uint32_t len, const ora_hit_t *hits, int n_hits, int max_sec, int full);
/* whole-file driver: FASTQ/FASTA (plain text) -> SAM; returns number of reads, or <0 */
long ora_classify_file(const ora_idx_t *idx, const char *reads_path, const char *out_path,
                       int max_sec, int full, int n_threads, uint64_t *bases);
uint64_t ora_occ(const ora_idx_t *idx, uint64_t r, uint8_t *c);
/* a-9 on its own (tests/test_stage_lv_extd.py): the strings with the 8 bytes in front of them that the callers' buffers hold */
int32_t ora_lv_extd(const uint8_t *ref_padded, int32_t ref_length, const uint8_t *query_padded, int32_t query_length);
/* a-11 on its own (tests/test_stage_combine_chain.py) */
void ora_combine_stage(uint32_t *chains, uint32_t n, const int32_t *queries, uint32_t n_q, int32_t *out);
/* a-12 on its own (tests/test_stage_sdp.py): sdp_match on one window, sdp_middle_M2 on one chain over a synthetic text (oracle/classify.c) */
int ora_sdp_match_stage(ora_ctx_t *c, const char *seq, uint32_t len, int strand, uint32_t q_bg, uint32_t q_ed,
                        const uint8_t *t_str, uint32_t t_len, uint32_t t_st, int is_forward, uint32_t *out, int max_out);
int ora_gap_stage(ora_ctx_t *c, const char *seq, uint32_t len, int strand, const uint8_t *refbin, uint64_t ref_bases,
                  const int32_t *anchors, uint32_t n_anchors, int32_t c_a, uint32_t *gap_nodes, uint32_t *n_gaps);
/* the sparse DP of a-12 on a bare node list (tests/test_stage_dp.py): rows of 4 (t_pos, q_pos, len, score), node 0 carries its score;
 * mode 0 middle, 1 right, 2 left -> the score of every node */
void ora_sdp_dp_stage(int mode, const uint32_t *nodes, uint32_t n, int32_t *scores);
/* a chain as the stage entries below take and give it: the layout of chain_item as oracle/classify.c and the device code hold it */
typedef struct {
	uint32_t ref_ID; int32_t q_t_dis; uint32_t sum_score, anchor_number;
	uint8_t direction, with_top_anchor, primary, pri_index;
	uint32_t t_st, t_ed, q_st, q_ed, indel, chain_id; int32_t cur;
} ora_chain_t;
/* one sdp_right_M2 (left == 0) or sdp_left_M2 on its own (tests/test_stage_ext.py): see oracle/classify.c */
int ora_ext_stage(ora_ctx_t *c, const char *seq, uint32_t L, int strand, int left, const uint8_t *refbin, uint64_t ref_bases,
                  const uint64_t *refinfo, uint32_t n_ref, ora_chain_t *chains, uint32_t n_chains, const int32_t *anchors, uint32_t n_anchors,
                  int chain_ID, int score_ori, uint32_t *info, uint32_t *win_n, uint32_t max_win, uint32_t *seg, uint32_t max_seg,
                  uint32_t *nodes, uint32_t max_nodes);
/* a-10 on its own (tests/test_stage_chain.py): chain_insert_M2 / chain_insert_M3 and the end of resolve_tree on a list of anchors */
int ora_resolve_stage(ora_ctx_t *c, const uint32_t *anchors, uint32_t n, int m3, uint32_t *order, int32_t *pre,
                      ora_chain_t *raw, uint32_t max_raw, uint32_t *n_raw, ora_chain_t *fin, uint32_t max_fin);
/* a-13 without the extensions and a-14 (tests/test_stage_finish.py); a-17: glibc's qsort with one of the three chain comparators */
int ora_finish_stage(ora_ctx_t *c, ora_chain_t *chains, uint32_t n, uint32_t read_len, int *max_read_l, int min_length, int min_score,
                     int min_score_LV3, ora_chain_t *tail, uint32_t *n_cut);
void ora_sort_stage(ora_ctx_t *c, ora_chain_t *chains, uint32_t n, int which);
/* a-4 .. a-8 on their own (tests/test_stage_anchor.py): fast_classify (what 0) or slow_classify (what 1) on one strand (1 = F, 0 = R), or
 * (what 2) fast_classify on the read as ora_classify calls it, with the strand swap and the both-direction rule.  The caller owns the
 * arrays of the trace and states their sizes (max_*); a count (n_*) beyond its size says that the array was too small.
 *   isl  one row per walked island (fast) or searched seed (slow): seed index, searches, skip flag (the next seed is jumped over), first
 *        anchor, last anchor + 1, largest map_seed score of a search, strand, MEMs collected (slow), 8th and 9th MEM of equal length (slow), 0
 *   mem  one row per bwt_MEM_search: row of isl, string index (= l_max), 13-mer prefix, max_rst, l_min, number of MEMs, set hits (a row
 *        seen before ended a walk), set restarts (the 500-entry set started over), then per MEM (at most 8) sp, match_len, sa_sp, sa_sp_l
 *   map  one row per map_seed: row of isl, reason (ORA_MS_*), return value, length of the reference-position list (0: not reached),
 *        anchors pushed, flags (ORA_MS_* bits), read_offset, match_len of the MEM */
#define ORA_AT_ISL 10
#define ORA_AT_MEM 40
#define ORA_AT_MAP 8
enum { ORA_MS_UNI_EARLY = 1, ORA_MS_UNI_LATE = 2, ORA_MS_PRE12 = 3, ORA_MS_SUF12 = 4, ORA_MS_LIST_1000 = 5, ORA_MS_LIST_51 = 6, ORA_MS_PUSHED = 7,
       ORA_MS_ALL_DROPPED = 8, ORA_MS_NO_SCORE = 9 };   /* unitig < 35 met early / late; s < 12 && l_pre == 12 without a unitig; s <= 20 && l_suf == 12; a list
       of >= 1000 positions (returns 50); a list of 51 .. 999 (anchors pushed or not: see the count); anchors pushed from a list of <= 50; every position of
       such a list dropped by score < 20; the score before the list was not positive */
enum { ORA_MS_SA_SP = 1, ORA_MS_SEARCH_L = 2, ORA_MS_SEARCH_R = 4, ORA_MS_EXT_L = 8, ORA_MS_Q_MINUS1 = 16, ORA_MS_NO_SUF = 32, ORA_MS_SHORT_PRE = 64 };
       /* sa_sp set; ref_search_l; ref_search_r; l_m_ext_l > 0 at a pushed anchor; the MEM reaches base 0 (q_off = -1); l_max_suf == 0; l_pre < 12 from the read */
typedef struct { ora_anchor_t a; uint64_t global_offset; } ora_anchor_full_t;
typedef struct {
	ora_seed_t *seeds[2]; uint32_t n_seed[2], total[2], max_seed;     /* [0] forward strand, [1] reverse strand */
	uint32_t both, first;                                             /* the both-direction rule; the strand with the larger total (walked first) */
	ora_anchor_full_t *anc; uint32_t n_anc, max_anc;
	int64_t *isl; uint32_t n_isl, max_isl;
	int64_t *mem; uint32_t n_mem, max_mem;
	int64_t *map; uint32_t n_map, max_map;
} ora_anchor_trace_t;
int ora_anchor_stage(ora_ctx_t *c, const ora_idx_t *idx, const char *seq, uint32_t len, int what, int strand, ora_anchor_trace_t *t);
#ifdef __cplusplus
}
#endif
#endif
