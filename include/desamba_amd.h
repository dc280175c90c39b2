/* desamba_amd -- C-ABI of the MI355X-native `deSAMBA classify` hot path.
 *
 * The reference has no plugin/FFI interface; its in-process seam for this path is the
 * kt_for call in classify_pipeline (src/cly_mt.c:389): a batch of kseq_t in, a batch of
 * cly_r out, of which the SAM writer consumes only cly_r.hit (chain_item, src/cly.h:69-89).
 * This header is that seam as a C ABI: plain pointers and sizes, no torch / HIP types.
 * Every entry point returns 0 on success or a negative DSB_E* code; nothing here calls
 * exit() (the reference's print-and-exit convention, src/lib/utils.c:144-176, lives only
 * in the CLI).  One dsb_ctx per host thread and GPU; batches run in submission order;
 * dsb_ctx_create_multi / dsb_multi_classify_batch spread one batch over a list of GPUs.
 *
 * There is NO CPU fallback: every compute stage runs as a HIP kernel on gfx950, and
 * dsb_ctx_create fails with DSB_ENODEV when no such device is present.
 */
#ifndef DESAMBA_AMD_H
#define DESAMBA_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSB_OK        0
#define DSB_EIO      -1   /* index file missing / short (reference: xread/xopen abort, src/lib/utils.h:112) */
#define DSB_ENODEV   -2   /* no gfx950 device, or HIP runtime error */
#define DSB_ENOMEM   -3
#define DSB_EINVAL   -4
#define DSB_ECAP     -5   /* a per-read device arena overflowed; the read's status says which */

typedef struct dsb_index dsb_index;   /* replaces DA_IDX (src/idx.h:68-91) */
typedef struct dsb_ctx dsb_ctx;       /* replaces Classify_buff_pool + MAP_opt (src/cly.h:139-158,17-26) */
typedef struct dsb_multi dsb_multi;   /* one dsb_ctx per GPU of a device list: the T worker threads of kt_for (src/cly_mt.c:389) with GPUs for threads */

/* replaces MAP_opt's classify-relevant fields, defaults {170, 64, 5} (src/cly_mt.c:486) */
typedef struct {
	int L_min_matching;   /* -l, idx.filter_min_length   (src/cly_mt.c:521) */
	int min_score;        /* -s, idx.filter_min_score    (src/cly_mt.c:522) */
	int max_sec_N;        /* -r, used by the SAM writer only */
	int n_slots;          /* 0 = default: reads in flight on the device (one wavefront each) */
	uint32_t max_read_len;     /* hints, 0 = none: with both set, arenas and batch buffers are allocated by dsb_ctx_create */
	uint32_t max_batch_reads;  /*   for batches of that many reads of up to that length, instead of inside the first batch */
	int input_slots;      /* batches a ctx can hold staged in HBM at once (dsb_ctx_select_slot); 0 or 1 = one */
	int reserved;         /* 0 */
	uint64_t max_batch_bases;  /* with the two hints above: bases of the largest batch (0 = max_batch_reads x max_read_len: all reads of full length) */
} dsb_opts;

/* replaces kseq_t as consumed by classify_seq (src/cly.c:3064): only seq/len reach the kernel */
typedef struct {
	const char *name;
	const char *seq;
	const char *qual;
	uint32_t len;
} dsb_read;

/* replaces chain_item as consumed by output_one_result_sam (src/cly_mt.c:245-344) */
typedef struct {
	uint32_t ref_ID, t_st, t_ed, q_st, q_ed, sum_score, indel;
	uint8_t direction, primary, pri_index, pad;
} dsb_hit;

/* replaces cly_r.hit (src/cly.h:93-100): hits of read i are hits[first .. first+n) in final order */
typedef struct {
	uint32_t first, n;
	int32_t status;       /* 0, or DSB_ECAP * 256 - bits: a capacity the read exceeded even in the second run (bits: 1 anchors,
	                         2 chains, 4 match nodes, 8 hit buffer, 16 loop budget) */
	uint32_t fast;        /* cly_r.fast_classify */
	uint32_t device_us;   /* time the read occupied its wavefront (100 MHz wall clock), diagnostics */
	uint32_t n_anc;       /* cly_r.anchor_v.n when classify_seq returns (printed by the DES writers) */
} dsb_read_result;

typedef struct {
	const dsb_read_result *reads;   /* n entries */
	const dsb_hit *hits;            /* owned by the ctx, valid until the next batch on it */
	size_t n_hits;
} dsb_result;

/* stage dump of the seed-lookup kernels (src/cly.c:1071-1234), used by the parity tests */
typedef struct { uint32_t offset, len; uint8_t top; uint8_t pad[3]; } dsb_seed;

/* per-batch device timings (HIP events on the ctx's stream), milliseconds */
typedef struct {
	float encode_ms, seed_probe_ms, classify_ms, total_ms;   /* classify_ms: the main k_classify launch */
	uint64_t windows;      /* exist-kmer windows probed (= P0 of SURVEY.md 8d): all of both strands, or what k_seed_scan asked for */
	uint64_t probes_t1;    /* probes that continued to table 1 (= P1) */
	uint64_t bases;
	float order_ms;        /* scoring + ordering of the reads (longest first) + the probes of the early launch */
	float tail_ms;         /* after the main launch: waiting for the early launch (heaviest reads, second stream) + the second run */
	uint32_t n_early;      /* reads that went through the early launch */
	uint32_t n_retry;      /* reads run a second time (32x match nodes, 8x anchors, 4x chains, 16x loop budget): theirs ran out */
	uint32_t n_regrow;     /* reads run again after the hit buffer had to be regrown */
	uint32_t seed_scan;    /* 1: the seed lookup ran as k_seed_scan (one lane per strand, windows = probes it issued); 0: all windows probed */
	/* work counters of the classify kernels, counted on the device (the terms of the algorithmic bytes) */
	uint64_t n_occ;        /* occ() evaluations (src/bwt.c:43) */
	uint64_t n_mem;        /* bwt_MEM_search calls = hash_index pairs read (src/cly.c:1388) */
	uint64_t n_sa;         /* get_uni calls = SA sample + unitig + ref-position lookups (src/cly.c:471) */
	uint64_t ref_bases;    /* reference bases fetched by get_ref (src/cly.c:435) */
	uint64_t main_occ, main_mem, main_sa, main_ref_bases;   /* the same for the main k_classify launch alone (what classify_ms times) */
	uint32_t n_heavy_mw;   /* reads of the early launch that ran on several wavefronts each (k_classify_heavy) */
	uint32_t n_requeue;    /* reads given up by their wavefront as heavy (quadratic sparse DP) and run again by a workgroup of wavefronts */
	uint64_t upload_bytes; /* bytes the sequences of the batch took over PCIe: bases / 4 from dsb_batch_upload (packed by the gather threads), the text from dsb_batch_upload_text */
	uint64_t anc_pool_asked;   /* anchors k_anchor asked its pool for: 0 when k_anchor did not run (the anchor stage ran inside k_classify) or no read of the
	                              batch had anchors; above anc_pool_cap, the reads that found the pool full walked their islands again in k_classify */
	uint64_t anc_pool_cap;     /* anchors the pool of k_anchor holds */
} dsb_timing;

/* load_idx (src/idx.c:1103-1160, src/bwt.c:68-104): read <dir>/deSAMBA.* into host memory */
/* Index construction on the GPU -- replaces build_index_main (src/idx.c:1254-1282: `deSAMBA index [SortedKmer]
 * [Reference] [IndexDir]`, i.e. build_UNITIG src/idx.c:884, build_BWT src/bwt.c:269, bwt_cal_SA src/idx.c:1163,
 * get_EXIST_kmer src/idx.c:986, write_idx src/idx.c:1046) and, with kmer_srt = NULL, the Jellyfish + kmersort steps in
 * front of it (src/idx_sort.c:298-401): the 31-mers are then enumerated from the reference text itself.
 * fasta: plain or gzip FASTA read with the reference's reader rules; out_dir is created; the ten deSAMBA.* files
 * written are byte-identical to the reference's (.ref_i: the reference leaves the padding behind each name
 * uninitialised; zeros here).  Limits: < 2^32 / 30 unitigs (the file format holds unitig numbers in 32 bits); k-mer ranks and BWT rows
 * are 64-bit (an index of > 2^32 BWT rows is built and classified on: tests/tools/huge_index.sh).  The build runs in one piece when
 * its working set (~60 bytes per reference base) fits the free device memory, and otherwise -- or when the environment says
 * DSB_BUILD_BUDGET=<bytes>[k|m|g] -- in passes over ranges of 13-mer prefixes (dsb_build_parts.h; the reference's bucket-by-bucket
 * construction, src/idx_sort.c:298-401, src/idx.c:884-1026): the device then holds the text (1 byte per base), ~12 bytes per unitig
 * occurrence and unitig, and one range; host memory holds the k-mer list (8 bytes per k-mer; with DSB_BUILD_SPILL=1 a temporary file in
 * out_dir holds it instead) and the files.  Same files either way.
 * DSB_ENOMEM: the budget does not hold what stays resident.  DSB_EINVAL: reference shorter than 31 bases, a k-mer of the text missing from kmer_srt or a
 * k-mer of kmer_srt missing from the text, or a unitig cycle the reference's builder does not handle either. */
typedef struct {
	uint64_t n_bases, n_refs, n_kmer, n_unitig, n_rows;
	double parse_s, sort_s, graph_s, walk_s, rows_s, tables_s, write_s, total_s;
	uint64_t budget_bytes;        /* 0: built in one piece; else the device memory the passes were planned for */
	uint64_t peak_device_bytes;   /* the most the build held at once (every allocation of the build is counted) */
	uint32_t ranges_kmers, ranges_unitig_numbers, ranges_rows, ranges_exist;   /* passes of the k-mer / unitig-number / BWT-row / filter-table stages */
	uint64_t spilled_bytes;       /* DSB_BUILD_SPILL=1: bytes of the k-mer list that went through <out_dir>/deSAMBA.kmers.tmp instead of host memory */
} dsb_build_stats;
int  dsb_index_build(const char *kmer_srt, const char *fasta, const char *out_dir, int device, dsb_build_stats *stats);

int  dsb_index_open(const char *dir, dsb_index **idx);
void dsb_index_close(dsb_index *idx);
/* reference names / lengths for the SAM writer (REF_INFO, src/idx.h:15-19) */
uint64_t    dsb_index_n_ref(const dsb_index *idx);
const char *dsb_index_ref_name(const dsb_index *idx, uint32_t ref_ID);
uint64_t    dsb_index_ref_len(const dsb_index *idx, uint32_t ref_ID);
int         dsb_index_ek_len(const dsb_index *idx);
/* host mirror of the device's prefix-interval lookup (hash_index[p], hash_index[p+1] of bwt_MEM_search, src/cly.c:1396-1399):
 * form 1 = from the compressed 64-byte lines staged on the device (returns -1 if this index keeps the raw table), 0 = raw */
int dsb_index_prefix_interval(const dsb_index *idx, uint32_t prefix, int form, uint64_t *sp, uint64_t *ep);
/* host mirror of the device rank structure, for layout tests without a GPU (occ, src/bwt.c:43-65) */
uint64_t dsb_index_occ_host(const dsb_index *idx, uint64_t r, uint8_t *c);

/* classify_main's set-up (src/cly_mt.c:518-550): stage the index into HBM, allocate arenas.  The staged index is shared
 * by all contexts of one (index, device) pair: a second context on a device costs only its arenas and buffers. */
int  dsb_device_count(void);           /* gfx950 or not: HIP devices visible to the process */
int  dsb_ctx_create(dsb_index *idx, int device_id, const dsb_opts *opts, dsb_ctx **ctx);
void dsb_ctx_destroy(dsb_ctx *ctx);
/* reset the running max_read_l (src/cly.c:2958).  The reference never resets it during a run -- its per-thread buffers
 * are allocated once, before the loop over the input files (src/cly_mt.c:538-556) -- so a drop-in caller calls this only
 * where a new `deSAMBA classify` process would start */
void dsb_ctx_reset_history(dsb_ctx *ctx);
/* The DSB_* diagnostic switches of the environment are read once, by dsb_ctx_create; this reads them again (tests and experiments
 * that change them on a living context).  No counterpart in the reference. */
void dsb_ctx_reload_env(dsb_ctx *ctx);
/* set it explicitly: the longest read of the run before the next batch (for callers that deal batches to several
 * contexts and therefore carry the prefix maximum themselves) */
void dsb_ctx_set_history(dsb_ctx *ctx, uint32_t max_len_before);
/* measurement hook for the seed-lookup kernels on tables far larger than the caches: the two exist-kmer tables
 * of this ctx become synthetic ones of table_bytes each (2^27 .. 2^34; k-mer length and mask as set_ekmer_par,
 * src/idx.c:966-982), each bit set with probability fill; dsb_batch_run then ends behind the seed lookup.  Upload the
 * batch AFTER this call (the window count of a read depends on k).  dsb_synthetic_filter_bit recomputes a table bit. */
int  dsb_ctx_use_synthetic_filter(dsb_ctx *ctx, uint64_t table_bytes, double fill);
int  dsb_synthetic_filter_bit(int which, uint64_t bit, double fill);
/* input slots (dsb_opts.input_slots > 1): the upload / run / fetch / timing calls below work on the selected slot, so a
 * ctx can keep several batches staged in HBM and run them in any order */
int  dsb_ctx_select_slot(dsb_ctx *ctx, int slot);

/* several GPUs of one node: reads sharded, index replicated, no collective.  One dsb_ctx per entry of
 * device_ids (a device listed twice gets two contexts that overlap each other's copies and kernels). */
int  dsb_ctx_create_multi(dsb_index *idx, const int *device_ids, int n_dev, const dsb_opts *opts, dsb_multi **m);
void dsb_multi_destroy(dsb_multi *m);
int  dsb_multi_n(const dsb_multi *m);
dsb_ctx *dsb_multi_ctx(dsb_multi *m, int i);          /* for callers that drive the contexts themselves (the CLI) */
void dsb_multi_reset_history(dsb_multi *m);
/* how the last dsb_multi_classify_batch was cut: the dsb_classify_batch calls context i made (a batch is cut into n / n_ctx reads per
 * call, not less than 32768, bounded by dsb_opts.max_batch_reads / max_batch_bases: a call fills the device from ~64 k long reads on) */
uint32_t dsb_multi_last_calls(const dsb_multi *m, int i);
/* the kt_for seam over all contexts: the batch is cut by dsb_shard_plan, results in input order, valid until the next call */
int  dsb_multi_classify_batch(dsb_multi *m, const dsb_read *reads, size_t n, dsb_result *out);
/* the sharding rule: contiguous chunks of the input order (a chunk ends after chunk_bases bases or chunk_reads reads;
 * 0 = 64 Mbases / 4096 reads) dealt round-robin over `world` ranks; hist_max_before = longest read before the chunk,
 * the only cross-read state (max_read_l, src/cly.c:2958).  out may be NULL to count (n_out). */
typedef struct { uint64_t start, end; uint32_t hist_max_before; int32_t rank; } dsb_chunk;
int  dsb_shard_plan(const uint32_t *lengths, size_t n, int world, uint64_t chunk_bases, uint32_t chunk_reads, dsb_chunk *out, size_t cap, size_t *n_out);

/* the kt_for seam (src/cly_mt.c:389): classify n reads; results valid until the next call */
int  dsb_classify_batch(dsb_ctx *ctx, const dsb_read *reads, size_t n, dsb_result *out);

/* the same, split so that a benchmark can time the device part with inputs resident in HBM */
/* (the sequences are gathered out of the caller's buffers by a few host threads through pinned chunks, each chunk
 * travelling as soon as it is full: reads may lie anywhere, e.g. in a mapped input file) */
int  dsb_batch_upload(dsb_ctx *ctx, const dsb_read *reads, size_t n);
/* the same for sequences that already lie in one host blob (a parsed FASTQ buffer): read i = text[seq_off[i] .. +seq_len[i]);
 * the blob goes to the device in one copy, at PCIe speed if it came from dsb_host_alloc (pinned memory) */
int  dsb_batch_upload_text(dsb_ctx *ctx, const char *text, size_t text_len, const uint64_t *seq_off, const uint32_t *seq_len, size_t n);
void *dsb_host_alloc(size_t bytes);
void  dsb_host_free(void *p);
/* host threads worth starting (the T of kt_for, src/cly_mt.c:389, for the host-side stages): CPUs the process may run on,
 * capped by the CPU quota of its control group */
int   dsb_host_cpus(void);
/* read_reads (src/cly_mt.c:42-56) for a plain-text FASTQ/FASTA file: stage records [skip, skip+max_reads) of the
 * file into HBM without per-read host copies; returns the number of reads staged, or a negative DSB_E* code */
long dsb_batch_upload_fastq(dsb_ctx *ctx, const char *path, size_t skip, size_t max_reads);
int  dsb_batch_run(dsb_ctx *ctx);                       /* all kernels, synchronous */
int  dsb_batch_fetch(dsb_ctx *ctx, dsb_result *out);
int  dsb_batch_timing(const dsb_ctx *ctx, dsb_timing *t);
/* stage dumps of the last run: seeds of one read strand (1 = forward, 0 = reverse) */
int  dsb_batch_seeds(dsb_ctx *ctx, size_t read, int strand, dsb_seed *out, size_t cap, uint32_t *n, uint32_t *total_score);
/* exist-kmer hit bits of one read strand, one byte per window */
int  dsb_batch_exist_bits(dsb_ctx *ctx, size_t read, int strand, uint8_t *out, size_t cap, uint32_t *n);

/* output_one_result_sam (src/cly_mt.c:245-344): format the records of one read into buf;
 * returns the number of bytes written (excluding the NUL), or -1 if cap is too small */
long dsb_format_sam(const dsb_index *idx, const dsb_read *read, const dsb_hit *hits, uint32_t n_hits,
                    int max_sec_N, int full, char *buf, size_t cap);

/* output_one_result_des / output_one_result_full (src/cly_mt.c:158-243): the DES (full = 0: secondaries up to max_sec_N)
 * or DES_FULL (full = 1: all) record of one read; same return convention as dsb_format_sam */
long dsb_format_des(const dsb_index *idx, const dsb_read *read, const dsb_read_result *rr, const dsb_hit *hits,
                    int max_sec_N, int full, char *buf, size_t cap);

/* ---- taxonomy: per-read taxa on the GPU and the abundance report of `deSAMBA analysis ana_meta[_base]` in the run itself.
 * The report a run accumulates equals what `deSAMBA analysis ana_meta` (by_base = 0) or `ana_meta_base` (by_base = 1) prints
 * for the SAM dsb_format_sam writes for the same reads, hits and max_sec_N (src/analysis.c:1271-1330,1831-1855), without its
 * leading "Current read <SAM>.temp\t<SAM>.temp\t"; a report that saw no read is empty. */
typedef struct dsb_taxonomy dsb_taxonomy;   /* nodes.dmp: the parent of every taxid up to max_tid */
typedef struct dsb_report dsb_report;       /* read counts / bases per taxid of a run, in input order */

/* load nodes.dmp as analysis does: the table ends at max_tid = (taxid of the LAST line) + 1 000 000.  DSB_EIO: cannot be
 * read; DSB_EINVAL: a chain of parent links runs in a cycle (the walks on the device are bounded by the deepest chain, which
 * the loader records).  dsb_taxonomy_load_any accepts cycles, as analysis always has: such a taxonomy serves a report
 * (whose walks then loop where analysis loops) but not dsb_ctx_set_taxonomy. */
int      dsb_taxonomy_load(const char *nodes_dmp, dsb_taxonomy **tx);
int      dsb_taxonomy_load_any(const char *nodes_dmp, dsb_taxonomy **tx);
void     dsb_taxonomy_close(dsb_taxonomy *tx);
uint32_t dsb_taxonomy_max_tid(const dsb_taxonomy *tx);
uint32_t dsb_taxonomy_parent(const dsb_taxonomy *tx, uint32_t taxid);   /* 0xffffffff: not in the file (or above max_tid) */

/* one read's taxon as k_read_taxon finds it.  taxid is the walk over THIS read's own records alone, in SAM order
 * (primary, supplementary, secondary up to max_sec_N): the primary's taxid (the second '|' field of the reference name),
 * moved to a later record's taxid when that record has the same AS and its taxid descends from the one held; 0 =
 * unclassified or not in the taxonomy.  The rules that join reads -- adjacent reads of one name are one read, a read
 * whose first AS is 0 ends at once, the last read of a run counts only in total_read_number -- belong to dsb_report. */
typedef struct {
	uint32_t taxid;
	uint32_t score;       /* AS of the first record */
	uint32_t len;         /* read length as analysis counts the first record's CIGAR */
	uint8_t  mapq;        /* MAPQ of the first record */
	uint8_t  flags;       /* DSB_TAXON_* */
	uint16_t pad;
} dsb_read_taxon;
#define DSB_TAXON_CLASSIFIED 1   /* the read has records (hits) */
#define DSB_TAXON_HOST       2   /* the device left the read to the host: first AS 0 or taxid above max_tid, an odd reference
                                    name, or a walk deeper than the bound.  taxid is final all the same (completed on the host). */

/* attach a taxonomy to a ctx (NULL detaches): its parent table and each reference's taxid are staged in HBM, and every batch
 * from then on ends with k_read_taxon.  The taxonomy must outlive the attachment.  Without one nothing is launched. */
int  dsb_ctx_set_taxonomy(dsb_ctx *ctx, const dsb_taxonomy *tx);
int  dsb_multi_set_taxonomy(dsb_multi *m, const dsb_taxonomy *tx);
/* the taxa of the last batch (n reads, valid until the next batch); DSB_EINVAL when no taxonomy is attached */
int  dsb_batch_taxa(dsb_ctx *ctx, const dsb_read_taxon **out);
/* the same for the last dsb_multi_classify_batch, in input order */
int  dsb_multi_taxa(dsb_multi *m, const dsb_read_taxon **out);

/* The report.  dsb_report_add feeds n reads in input order (res->reads[i], its hits res->hits + first): a read with a
 * device record (taxa[i], DSB_TAXON_HOST clear) is counted from it; the others, and a read whose name is that of the read
 * before it, are walked on the host over the records dsb_format_sam prints for it.  taxa may be NULL: every read is then
 * walked on the host.  A classified read stays open until a read of another name arrives.
 * dsb_report_add_sam feeds SAM text (the `@` lines at the top skipped), as `analysis` reads it.
 * dsb_report_format: same return convention as dsb_format_sam.  by_base = 0: ana_meta, 1: ana_meta_base. */
int  dsb_report_create(const dsb_taxonomy *tx, dsb_report **rep);
int  dsb_report_add(dsb_report *rep, const dsb_index *idx, const dsb_read *reads, const dsb_result *res, const dsb_read_taxon *taxa,
                    size_t n, int max_sec_N);
int  dsb_report_add_sam(dsb_report *rep, const char *text, size_t len);
long dsb_report_format(const dsb_report *rep, int by_base, char *buf, size_t cap);
void dsb_report_destroy(dsb_report *rep);

/* ---- per-reference coverage of a run (breadth and depth), accumulated on the GPU after every batch.
 * Counted are the records dsb_format_sam prints without FLAG 0x100: the primary and the supplementary ones (pri_index 0);
 * secondary records never count, so the numbers do not depend on max_sec_N.  A record's interval is
 * [min(t_st, LN), min(t_ed, LN)) of its reference (LN = dsb_index_ref_len), empty when t_ed <= t_st. */
typedef struct {
	uint64_t numreads;        /* counted records */
	uint64_t covbases;        /* size of the union of their intervals */
	uint64_t aligned_bases;   /* sum of their interval lengths */
	uint64_t mapq_sum;        /* sum of the MAPQ each prints */
} dsb_ref_coverage;
/* on: allocate a bitmap of one bit per reference base (plus 4 counters per reference) and zero it; DSB_ENOMEM if it does
 * not fit.  off: free it.  While it is on, every batch ends with k_ref_cover; while it is off nothing is allocated or launched. */
int  dsb_ctx_enable_coverage(dsb_ctx *ctx, int on);
int  dsb_ctx_reset_coverage(dsb_ctx *ctx);                    /* zero, keep the allocation */
/* dsb_index_n_ref entries: everything since enable / reset (fetching changes nothing); DSB_EINVAL when coverage is off */
int  dsb_ctx_coverage(dsb_ctx *ctx, dsb_ref_coverage *out);
int  dsb_multi_enable_coverage(dsb_multi *m, int on);
int  dsb_multi_coverage(dsb_multi *m, dsb_ref_coverage *out);  /* merged over the contexts: what one context would count */
/* the table of `samtools coverage` without its base-quality column: a header line, then one row per reference with
 * numreads > 0, in ref_ID order.  Same return convention as dsb_format_sam. */
long dsb_coverage_format(const dsb_index *idx, const dsb_ref_coverage *cov, char *buf, size_t cap);

/* ---- per-window coverage: where on each reference the counted records lie.
 * Window size W >= 1 bases.  Window j of reference r (LN = dsb_index_ref_len(r)) is [jW, min((j + 1)W, LN)), 0-based half-open, in the
 * coordinates POS prints; r has ceil(LN / W) windows (none for LN 0), and the windows of all references form one array in which r's
 * begin at first_r, the prefix sum of ceil(LN / W) in ref_ID order.  Counted are exactly the records of dsb_ref_coverage, each with
 * its clipped interval [s, e) = [min(t_st, LN), min(t_ed, LN)); a record with e <= s adds to no window (it still counts in its
 * reference's numreads).  Over the windows of a reference, aligned_bases and covbases sum to the reference's, and starts to its
 * numreads minus its records with an empty interval.  Integers that do not depend on how the reads are split into batches, slots
 * or contexts. */
typedef struct {
	uint64_t starts;          /* counted records with e > s whose s lies in the window */
	uint64_t aligned_bases;   /* sum over the counted records of the length of [s, e) within the window */
	uint64_t covbases;        /* bases of the window in the union of those intervals */
} dsb_cov_window;
uint64_t dsb_coverage_n_windows(const dsb_index *idx, uint32_t window);   /* the array's length; 0 for window 0 */
/* Windows are part of the coverage state (one bitmap, shared with dsb_ctx_coverage): coverage must be on, else DSB_EINVAL.
 * window > 0: allocate 24 bytes per window (DSB_ENOMEM if it does not fit; coverage stays on, windows off) and zero the WHOLE
 * coverage state as dsb_ctx_reset_coverage does -- also when windows were on already, with this or another size -- so bitmap,
 * per-reference counters and windows always describe the same reads.  window 0: off, freed; the rest of the state stays.
 * dsb_ctx_reset_coverage zeroes the windows too, dsb_ctx_enable_coverage(ctx, 0) frees them.  While windows are on, every batch
 * ends with k_ref_windows behind k_ref_cover; while they are off nothing is allocated or launched. */
int  dsb_ctx_enable_coverage_windows(dsb_ctx *ctx, uint32_t window);
/* *n = the number of windows; out NULL: that only; cap < *n: DSB_ECAP; windows off: DSB_EINVAL.  Everything since enable / reset.
 * Fetching changes nothing on the device but the covbases slots it recomputes and does not disturb a batch in flight. */
int  dsb_ctx_coverage_windows(dsb_ctx *ctx, dsb_cov_window *out, size_t cap, size_t *n);
int  dsb_multi_enable_coverage_windows(dsb_multi *m, uint32_t window);
int  dsb_multi_coverage_windows(dsb_multi *m, dsb_cov_window *out, size_t cap, size_t *n);   /* merged over the contexts: what one context would count */
/* a header line "#rname start end numreads covbases coverage meandepth" (tabs), then for every reference with cov[r].numreads > 0,
 * in ref_ID order, all its windows in order, those with all zeros included: start / end the window's bounds (BED convention),
 * numreads = starts, coverage = 100 covbases / (end - start) and meandepth = aligned_bases / (end - start), both as %g.  win: the
 * dsb_coverage_n_windows(idx, window) windows.  Same return convention as dsb_format_sam. */
long dsb_coverage_windows_format(const dsb_index *idx, const dsb_ref_coverage *cov, const dsb_cov_window *win, uint32_t window, char *buf, size_t cap);

/* ---- per-reference abundance of a run by expectation-maximisation on the GPU.
 * Every read with hits (those dsb_batch_fetch hands out, whatever max_sec_N is) has a candidate set: the references r < n_ref
 * whose best AS S_r has S_r * 1000 >= S_max * min_permille (S_max: the read's best AS), ascending, each once.  Reads are not
 * joined by name.  A distinct set is a class k with c_k reads.  With L_r = dsb_index_ref_len(r) and N classified reads, the
 * read shares a_r start at 1 / R on the R references that occur in some class, and one iteration is
 *     a'_r = (a_r / L_r) * (sum over the classes k holding r of c_k / sum_{s in k} a_s / L_s) / N,
 * until the first iteration with max_r N |a'_r - a_r| < tol or max_iter iterations.  The doubles do not depend on how the reads
 * were split into batches, input slots or contexts, nor on the run: every sum has a fixed order. */
typedef struct {
	uint64_t numreads;     /* classified reads whose set holds the reference */
	uint64_t uniqreads;    /* ... whose set is that reference alone */
	double   est_reads;    /* N * a_r */
	double   read_share;   /* a_r */
	double   copy_share;   /* (a_r / L_r) / sum_s (a_s / L_s) */
} dsb_ref_abundance;
typedef struct {
	uint32_t max_iter;     /* >= 1; default 10000 */
	uint32_t reserved;     /* 0 */
	double   tol;          /* >= 0, in reads; default 0.01 */
} dsb_em_opts;
typedef struct {
	uint64_t reads;        /* reads the batches held */
	uint64_t classified;   /* N: reads with a candidate set */
	uint64_t classes;      /* distinct candidate sets */
	uint32_t iterations;   /* iterations run (the state returned is the one after the last) */
	uint32_t converged;    /* 1: the last iteration met tol (also for a run without classified reads); 0: max_iter ran out */
	double   max_change;   /* max_r N |a'_r - a_r| of the last iteration (0 when none ran) */
	uint32_t min_permille; /* the threshold the sets were formed with */
	uint32_t reserved;
} dsb_abundance_summary;
/* on: every batch from now on ends with k_em_collect, which appends each read's set to a store in HBM (16 bytes per read + 4 per
 * hit; grown between batches, DSB_ENOMEM rather than a lost read); min_permille in 1 .. 1000 (1000: ties
 * only), else DSB_EINVAL.  On again: new threshold, store emptied.  off: freed; nothing is allocated or launched while off. */
int  dsb_ctx_enable_abundance(dsb_ctx *ctx, int on, uint32_t min_permille);
int  dsb_ctx_reset_abundance(dsb_ctx *ctx);                   /* empty the store, keep the allocation */
/* the estimate over everything since enable / reset (the store is left as it is): out has dsb_index_n_ref entries.  opts NULL:
 * the defaults.  DSB_EINVAL when abundance is off or an option is out of range. */
int  dsb_ctx_abundance(dsb_ctx *ctx, const dsb_em_opts *opts, dsb_ref_abundance *out, dsb_abundance_summary *summary);
int  dsb_multi_enable_abundance(dsb_multi *m, int on, uint32_t min_permille);
/* the contexts' stores together, solved on the first context's device: bitwise what one context would give */
int  dsb_multi_abundance(dsb_multi *m, const dsb_em_opts *opts, dsb_ref_abundance *out, dsb_abundance_summary *summary);
/* a '#' summary line, a header line, then one row per reference with numreads > 0, in ref_ID order (DESIGN 2.10 has the
 * formats).  Same return convention as dsb_format_sam. */
long dsb_abundance_format(const dsb_index *idx, const dsb_ref_abundance *ab, const dsb_abundance_summary *summary, char *buf, size_t cap);

/* ---- each read assigned to one reference by its EM posterior.  With a_r the read_share of the solve, L_r the
 * reference lengths as doubles (1 for an empty reference) and C a read's candidate set in ascending ref_ID: w_s = a_s / L_s,
 * d = the sum of w_s over C in that order from 0.0, ref_ID = the s of C with the largest w_s (equal weights: the smallest ref_ID),
 * posterior = w_ref / d (d == 0, every share underflowed: the smallest ref_ID of C and 0), n_cand = |C|.  A read without a
 * candidate set: ref_ID DSB_ASSIGN_NONE, n_cand 0, posterior 0.  The record is a function of the read's class alone: reads of one
 * class get bitwise-equal records, whatever the batch split, input slot, context or run. */
typedef struct { uint32_t ref_ID;   /* DSB_ASSIGN_NONE: unclassified */
                 uint32_t n_cand; double posterior; } dsb_read_assign;
#define DSB_ASSIGN_NONE 0xffffffffu
/* read i of the batch staged in the selected input slot has ordinal first + i in the records below.  Taken by that slot's next
 * dsb_batch_run / dsb_classify_batch and forgotten after it.  Not set: the reads this context has collected since
 * dsb_ctx_enable_abundance / dsb_ctx_reset_abundance, so that a context driven plainly numbers its reads in run order.
 * dsb_multi_classify_batch numbers each piece by its input index, counted over all calls since enable / reset. */
int  dsb_ctx_set_batch_ordinal(dsb_ctx *ctx, uint64_t first);
/* dsb_ctx_abundance, and reads[ordinal] = the record of every read since enable / reset.  *n = 1 + the largest ordinal a batch
 * covered (0: none); an ordinal below *n that no batch covered gets the "none" record.  reads NULL: *n is set and nothing else is
 * done (out and summary may be NULL); cap < *n: DSB_ECAP.  out and summary are what dsb_ctx_abundance gives for the same state. */
int  dsb_ctx_abundance_assign(dsb_ctx *ctx, const dsb_em_opts *opts, dsb_ref_abundance *out, dsb_abundance_summary *summary,
                              dsb_read_assign *reads, size_t cap, size_t *n);
int  dsb_multi_abundance_assign(dsb_multi *m, const dsb_em_opts *opts, dsb_ref_abundance *out, dsb_abundance_summary *summary,
                                dsb_read_assign *reads, size_t cap, size_t *n);
/* one line per read: QNAME \t rname \t taxid \t n_cand \t posterior (%.6f) \n -- QNAME as dsb_format_sam prints it, taxid the second
 * '|' field of the reference name (0: none); an unclassified read: QNAME \t * \t 0 \t 0 \t 0.000000.  Return as dsb_format_sam
 * (-1 also for a ref_ID that is neither DSB_ASSIGN_NONE nor a reference of the index). */
long dsb_format_assign(const dsb_index *idx, const dsb_read *read, const dsb_read_assign *a, char *buf, size_t cap);

/* ---- per-read classification by the lowest common ancestor (LCA) of the near-best hits, on the GPU.
 * Per read (reads are not joined by name): its hits are those dsb_batch_fetch hands out, whatever max_sec_N is; hits with
 * ref_ID >= n_ref are skipped, and a read with no hit left is unclassified (record all zero).  S_max is the largest AS; a hit
 * passes when AS * 1000 >= S_max * min_permille (64-bit); n_pass counts passing hits, not references.  A taxid is rooted when it
 * lies in 1 .. max_tid and its parent links reach taxid 1; depth = links to taxid 1.  A passing hit whose reference's taxid (the
 * second '|' field of its name) is not rooted is left out.  taxid = the deepest node that is an ancestor-or-self of every
 * remaining passing hit's taxid; none remaining: taxid 0 and DSB_LCA_NO_TAXON; more than one distinct taxid among them:
 * DSB_LCA_AMBIGUOUS.  The result does not depend on hit order, duplicates, batch split, input slot or context. */
typedef struct { uint32_t taxid, score, n_pass; uint16_t depth; uint8_t flags, pad; } dsb_read_lca;   /* score = S_max */
#define DSB_LCA_CLASSIFIED 1   /* the read has hits */
#define DSB_LCA_NO_TAXON   2   /* ... but no passing hit with a rooted taxid: taxid 0 */
#define DSB_LCA_AMBIGUOUS  4   /* passing hits of more than one taxid */
/* run-wide: direct_reads = reads whose taxid is this one, clade_reads = the same summed over the taxon and its descendants */
typedef struct { uint32_t taxid, pad; uint64_t clade_reads, direct_reads; } dsb_taxon_count;
typedef struct { uint64_t reads, classified /* taxid != 0 */, no_taxon, ambiguous; uint32_t min_permille, reserved; } dsb_lca_summary;
/* on: every batch from now on ends with k_read_lca and k_lca_count (a depth table beside the parent table, one u64 per taxid for
 * the run's counts); needs a taxonomy from dsb_taxonomy_load attached (dsb_ctx_set_taxonomy), else DSB_EINVAL; min_permille outside
 * 1 .. 1000: DSB_EINVAL.  On again: new threshold, counts zeroed.  off: freed; nothing is allocated or launched while off.
 * dsb_ctx_set_taxonomy on a ctx whose LCA is on turns it off. */
int  dsb_ctx_enable_lca(dsb_ctx *ctx, int on, uint32_t min_permille);
int  dsb_ctx_reset_lca(dsb_ctx *ctx);                          /* zero the counts, keep the allocation */
int  dsb_batch_lca(dsb_ctx *ctx, const dsb_read_lca **out);    /* the records of the last batch (n reads), valid until the next */
/* everything since enable / reset (fetching changes nothing): the taxa with clade_reads > 0 in ascending taxid, rolled up on the
 * device; only these rows are copied.  *n = the number of rows; out gets the first min(cap, *n) of them (out NULL: count only);
 * DSB_ECAP when out is given and cap < *n.  summary may be NULL. */
int  dsb_ctx_lca_counts(dsb_ctx *ctx, dsb_taxon_count *out, size_t cap, size_t *n, dsb_lca_summary *summary);
int  dsb_multi_enable_lca(dsb_multi *m, int on, uint32_t min_permille);
int  dsb_multi_lca(dsb_multi *m, const dsb_read_lca **out);    /* the last dsb_multi_classify_batch, in input order */
/* the contexts' counts added on the first context's device, then the same roll-up: what one context would give */
int  dsb_multi_lca_counts(dsb_multi *m, dsb_taxon_count *out, size_t cap, size_t *n, dsb_lca_summary *summary);
typedef struct dsb_taxnames dsb_taxnames;                       /* names.dmp: the "scientific name" of each taxid */
int  dsb_taxnames_load(const char *names_dmp, dsb_taxnames **names);   /* DSB_EIO: cannot be read */
void dsb_taxnames_close(dsb_taxnames *names);
/* Kraken's per-read line: C|U \t QNAME \t taxid \t read length \t S_max:n_pass \n -- C iff taxid != 0, QNAME as dsb_format_sam
 * prints it; columns 1 to 4 are Kraken's, column 5 stands where Kraken puts its k-mer string.  Return as dsb_format_sam. */
long dsb_format_kraken(const dsb_read *read, const dsb_read_lca *lca, char *buf, size_t cap);
/* Kraken's report (`kraken2 --report`) of the rows of dsb_*_lca_counts: a line for the reads - classified unclassified reads (code
 * U, taxid 0) when there are any, then the tree from taxid 1 depth first, children by clade_reads descending then taxid
 * ascending; each line  %6.2f \t clade \t direct \t code \t taxid \t  + two spaces per depth + name (names NULL or without the
 * taxid: the decimal taxid).  Code: R for taxid 1, D K P C O F G S for superkingdom / domain, kingdom, phylum, class, order, family,
 * genus, species; any other rank takes its parent's letter and the parent's number plus one (S, S1, S2; R1 under the root).
 * Zero reads: empty.  Return as dsb_format_sam. */
long dsb_lca_report_format(const dsb_taxonomy *tx, const dsb_taxnames *names, const dsb_taxon_count *rows, size_t n,
                           const dsb_lca_summary *summary, char *buf, size_t cap);

/* ---- per-hit edit distance and per-reference identity, by banded alignment on the GPU.
 * Counted are the records of dsb_ref_coverage: record i of a read with i == 0 or pri_index == 0, among the hits dsb_batch_fetch hands
 * out; every other hit gets an all-zero record.  With L the read length and LN = dsb_index_ref_len(ref_ID) (0 for ref_ID >= n_ref):
 * qs = min(q_st, L), qe = min(q_ed, L), ts = min(t_st, LN), te = min(t_ed, LN), n = qe - qs, m = te - ts (0 when the end is not above
 * the start).  Q = bases [qs, qe) of the strand the chain was built on (direction 1: the read as given; 0: its reverse complement;
 * q_st and q_ed count on that strand), T = bases [ts, te) of the reference.  n == 0 or m == 0: DSB_IDENT_EMPTY.  d = m - n,
 * |d| > DSB_IDENT_MAX_SKEW: DSB_IDENT_SKEW.  Else edits = the unit-cost global edit distance (mismatches and indels) of Q and T over
 * the cells (i, j) with min(0, d) - band <= j - i <= max(0, d) + band: never below the unbanded distance, and equal to it when
 * edits <= band (DSB_IDENT_EXACT).  E_cap = floor(max(n, m) * max_permille / 1000): a distance above it is reported as E_cap + 1
 * with DSB_IDENT_OVER, and the search stops there.  EMPTY and SKEW records have edits 0.  The identity of a record is
 * 1 - edits / max(n, m), and 0 for an EMPTY, SKEW or OVER record.
 * The intervals are taken as the hit gives them, and the hit's two starts are not always a matched pair: where an end of the chain
 * is still its first or last anchor's (map_seed: index_in_read = read_offset + 1 - left extension with the reference's read_offset =
 * k_idx + l_ek - 1 - match_len; chain_insert_meta copies it), q lies one base below the base that t_st matched, and only an end the
 * left or right extension moved (sdp_left / sdp_right set q_st, t_st from a match node) is a matched pair.  A hit does not say which
 * kind its ends are.  Seen on reads that match over their whole length: q_st 0 with t_st one above the read's 0-based start, 2 edits
 * (one base alone at either end) where there are none.  So edits may be high by up to 2, identity low by up to 2 / max(n, m). */
typedef struct { uint32_t edits, q_len /* n */, t_len /* m */, flags; } dsb_hit_identity;
#define DSB_IDENT_EXACT 1      /* edits <= band: the band did not matter */
#define DSB_IDENT_OVER  2      /* more than E_cap edits: edits = E_cap + 1 */
#define DSB_IDENT_SKEW  4      /* |m - n| > DSB_IDENT_MAX_SKEW: not aligned */
#define DSB_IDENT_EMPTY 8      /* n == 0, m == 0 or ref_ID >= n_ref: not aligned */
#define DSB_IDENT_MAX_SKEW 4096
#define DSB_IDENT_MAX_BAND 1024
#define DSB_IDENT_BAND_DEFAULT 256
#define DSB_IDENT_PERMILLE_DEFAULT 300
/* per reference, everything since enable / reset: integer sums that do not depend on batch split, input slot, context or run.
 * records, q_bases, t_bases, edits and exact count the records without EMPTY, SKEW and OVER; unaligned those with one of the three
 * (a record with ref_ID >= n_ref belongs to no reference and is counted nowhere). */
typedef struct { uint64_t records, q_bases, t_bases, edits, exact, unaligned; } dsb_ref_identity;
/* on: every batch from now on ends with k_ident_list, k_hit_edits and k_ident_ref (16 bytes per hit of the hit buffer, 48 bytes per
 * reference, and the wavefronts' diagonal arena: 8 bytes x (DSB_IDENT_MAX_SKEW + 2 band + 3) each).  band 0 .. DSB_IDENT_MAX_BAND and
 * max_permille 1 .. 1000, else DSB_EINVAL; band == 0 && max_permille == 0: the defaults (a band of 0 is asked for with its cap
 * spelled out, e.g. 0, 300).  On again: new options, table zeroed.  off: freed; nothing is allocated or launched while off. */
int  dsb_ctx_enable_identity(dsb_ctx *ctx, int on, uint32_t band, uint32_t max_permille);
int  dsb_ctx_reset_identity(dsb_ctx *ctx);                               /* zero the table, keep the allocation */
/* the records of the last batch, one per hit of dsb_batch_fetch's hits (n_hits entries), valid until the next batch */
int  dsb_batch_identity(dsb_ctx *ctx, const dsb_hit_identity **out);
int  dsb_ctx_identity(dsb_ctx *ctx, dsb_ref_identity *out);              /* dsb_index_n_ref entries since enable / reset */
int  dsb_multi_enable_identity(dsb_multi *m, int on, uint32_t band, uint32_t max_permille);
int  dsb_multi_identity(dsb_multi *m, const dsb_hit_identity **out);     /* the last dsb_multi_classify_batch: one per hit of its result */
int  dsb_multi_ref_identity(dsb_multi *m, dsb_ref_identity *out);        /* the contexts' tables added */
/* one line per counted record of a read, in record order (hits and ident: the read's own, rr->n of each):
 * QNAME \t rname \t +|- \t qs \t qe \t ts \t te \t AS \t edits \t identity (%.4f) \t flags (decimal) \n; a read without hits:
 * QNAME \t * \t * \t 0 \t 0 \t 0 \t 0 \t 0 \t 0 \t 0.0000 \t 0 \n.  Return as dsb_format_sam. */
long dsb_format_identity(const dsb_index *idx, const dsb_read *read, const dsb_read_result *rr, const dsb_hit *hits, const dsb_hit_identity *ident,
                         char *buf, size_t cap);
/* "#rname records q_bases t_bases edits identity exact unaligned" (tabs), then one row per reference with records + unaligned > 0 in
 * ref_ID order; identity = 1 - edits / max(q_bases, t_bases) as %.4f (0.0000 without bases).  Return as dsb_format_sam. */
long dsb_identity_format(const dsb_index *idx, const dsb_ref_identity *tab, char *buf, size_t cap);
/* host mirror of the 2-bit reference text: codes[i] = base start + i of reference ref_ID (0 A, 1 C, 2 G, 3 T; the index holds
 * every other letter of the FASTA as A, where a read's other letters count as C), len codes;
 * DSB_EINVAL for a reference the index does not have or a window that reaches beyond its length */
int  dsb_index_ref_bases(const dsb_index *idx, uint32_t ref_ID, uint64_t start, uint32_t len, uint8_t *codes);
/* n_pairs bare alignments by the device function of k_hit_edits: Q of pair p = q_codes[q_off[p] .. + q_len[p]), T likewise, one code
 * (0 .. 3) per byte.  The two blobs are packed on the device as reads and reference text are laid out (32 bases per 64-bit word and 4
 * per byte, first base in the top bits), base b of a blob at base b of its packed form: a pair starts at word phase q_off & 31 and
 * byte phase t_off & 3.  band 0 .. DSB_IDENT_MAX_BAND, max_permille 1 .. 1000, a length up to 2^30 and an offset up to 2^40, else DSB_EINVAL
 * (no defaults here).  out: n_pairs records. */
int  dsb_ctx_edit_pairs(dsb_ctx *ctx, const uint8_t *q_codes, const uint64_t *q_off, const uint32_t *q_len,
                        const uint8_t *t_codes, const uint64_t *t_off, const uint32_t *t_len, size_t n_pairs,
                        uint32_t band, uint32_t max_permille, dsb_hit_identity *out);

/* ---- base-level alignment of every counted record on the GPU: CIGAR operations and NM.
 * Everything of the identity records above stands: which records are counted, qs, qe, ts, te, n, m, Q, T, the band [lo, hi] =
 * [min(0, d) - band, max(0, d) + band], W = hi - lo + 1, E_cap and the flags EMPTY / SKEW / OVER / EXACT.  The intervals are taken as
 * they come, so the one-base offset of a chain end that is still its anchor's (above) shows as a leading or trailing 1I / 1D / 1X;
 * classify is not changed.
 * The alignment of a record is the path that the distance's own recurrence takes.  FR_e[k] is the furthest i on diagonal k (cells
 * (i, i + k)) after e edits; generation e holds the diagonals [max(lo, -e), min(hi, e)].  On diagonal k of generation e the candidate
 * chosen is: the mismatch from FR_{e-1}[k] (+1, if the cell lies in the rectangle) -- it wins ties; then a base of T alone from
 * FR_{e-1}[k - 1], if strictly further; then a base of Q alone from FR_{e-1}[k + 1] (+1), if strictly further.  Move codes: 0 mismatch,
 * 1 T alone, 2 Q alone, 3 no candidate moved (unreached, or the value carried).  The path runs back from generation `edits` on diagonal
 * d = m - n to generation 0 on diagonal 0 by the moves alone (0 keeps k, 1 goes to k - 1, 2 goes to k + 1) and is then replayed from
 * (0, 0): slide while Q[i] == T[i + k] (=), apply the move (X: i + 1; D: j + 1, k + 1; I: i + 1, k - 1), slide, and so on; the last slide
 * ends on (n, m).  X + I + D == edits.
 * An operation is len << 4 | op with BAM's codes (len below 2^28, as in BAM); adjacent equal operations are merged, none has length
 * 0, and a record has at most 2 edits + 1 of them.  Equality is equality of the 2-bit codes the device holds: a letter of a read
 * that is not A, G or T is C, a letter of the reference that is not C, G or T is A -- so an N can stand under =.
 * Trace room: a wavefront's trace place holds trace_kib x 1024 bytes and a generation takes R = 16 x ceil(W / 64) of them (two bit
 * planes of the move codes, 64 diagonals per 16 bytes).  A record has a path iff it is aligned (not EMPTY / SKEW / OVER) and
 * edits x R <= trace_kib x 1024: a rule of (n, m, band, edits, trace_kib) alone, whatever wavefront takes the record.  Where the room
 * ends the forward pass goes on without tracing: edits and the identity record are what they are without alignment, and the record
 * gets DSB_ALN_NOTRACE. */
typedef struct { uint64_t ops_off; uint32_t n_ops, n_x, n_ins, n_del, flags, pad; } dsb_hit_alignment;   /* n_x, n_ins, n_del: bases */
#define DSB_ALN_OPS       1    /* n_ops operations at ops_off of the batch's operation array */
#define DSB_ALN_NOTRACE   2    /* aligned, but edits x R is above the trace room, or, in checkpoint mode, no plan: no path */
#define DSB_ALN_NOROOM    4    /* the batch's operation array was full: n_ops = 0.  Records take their room in the order their wavefronts
                                  finish, so WHICH records lose is not deterministic (that none loses is: see ops_cap) */
#define DSB_ALN_UNALIGNED 8    /* the identity record is EMPTY, SKEW or OVER */
#define DSB_ALN_OP_I 1
#define DSB_ALN_OP_D 2
#define DSB_ALN_OP_EQ 7
#define DSB_ALN_OP_X 8
#define DSB_ALN_TRACE_KIB_DEFAULT 2048
#define DSB_ALN_TRACE_KIB_MAX 65536
/* on: needs identity on (DSB_EINVAL otherwise) and uses its band and cap; from the next batch on k_hit_align runs in place of
 * k_hit_edits -- one forward pass, so the identity records and the per-reference table are what they are without it.  Allocates the
 * trace arena, trace_kib KiB for each wavefront of the grid (8 per compute unit: 2048 wavefronts x 2048 KiB = 4 GiB on an MI355X at the
 * default), 32 bytes per place of the hit buffer and, per batch, the operation array.  trace_kib 0: the default; 1 .. 65536 else
 * DSB_EINVAL.  ops_cap 0: the array is sized per batch, one operation per base of the batch's reads plus 4 per place of the hit buffer
 * (a record reserves its bound 2 edits + 1, so this is enough whenever 2 edits + 1 <= n for every record); otherwise it holds ops_cap
 * operations.  An allocation that fails: DSB_ENOMEM, and alignment stays off.  off: freed; nothing is allocated or launched while off.
 * Turning identity off, or on again with another band, turns alignment off too. */
int  dsb_ctx_enable_alignment(dsb_ctx *ctx, int on, uint32_t trace_kib, uint64_t ops_cap);
/* Checkpoint mode: the same alignment -- every record that gets a path gets exactly the operations defined above --
 * held in a fixed trace room.  The forward pass keeps the trace of one segment of K generations and the furthest-reaching values of
 * every K-th generation (a checkpoint); after the hit the earlier segments are computed again from their checkpoints, one at a time,
 * and walked back.  The price is a second forward pass.  WHICH records get a path follows the record's plan, known before the pass and
 * a function of (n, m, band, max_permille, trace_kib) alone, never of the edits.  With W, E_cap as above, in bytes:
 *   Rb = 16 ceil(W / 64) a generation's trace, C = 16 ceil(4 (W + 2) / 16) a checkpoint, Mv = 16 ceil(E_cap / 16) a byte per move,
 *   room = trace_kib x 1024, A = room - Mv.
 *   1. A < 0: no plan.  2. E_cap x Rb <= A: K = max(E_cap, 1), no checkpoint (one pass).  3. Otherwise K = floor(A / 2 / Rb); K < 1: no
 *   plan.  4. n_ckpt = floor((E_cap - 1) / K) checkpoints, after generations K, 2K, .. < E_cap.  5. A plan iff n_ckpt x C <= A - K x Rb.
 * An aligned record with a plan always gets a path (DSB_ALN_NOROOM and the 2^28 limit apply as ever); one without a plan gets
 * DSB_ALN_NOTRACE, its forward pass running as it does without alignment.  The two modes are NOT nested: the full mode's rule looks at
 * edits, the plan at E_cap, so a short record whose E_cap is far above its edits can have a path in full mode and no plan here (at
 * trace_kib 1 and band 32, a 200 x 200 pair with 3 edits under a cap of 310 permille).  There is no fallback from one to the other.
 * 50000 x 50750 bases at band 256 and 300 permille: K = 3253 with 4 checkpoints in the default 2048 KiB, where the full mode needs
 * edits x 336 bytes. */
#define DSB_ALN_MODE_FULL       0
#define DSB_ALN_MODE_CHECKPOINT 1
/* the plan of a pair of n x m bases: 1 with *K and *n_ckpt set, 0 for no plan; DSB_EINVAL for a length of 2^28 or more, band above
 * DSB_IDENT_MAX_BAND, max_permille outside 1 .. 1000, trace_kib outside 1 .. DSB_ALN_TRACE_KIB_MAX or a null pointer.  Host only, no
 * context: the function the kernels call. */
int  dsb_aln_plan(uint32_t n, uint32_t m, uint32_t band, uint32_t max_permille, uint32_t trace_kib, uint32_t *K, uint32_t *n_ckpt);
/* from the next batch on k_hit_align_ck (checkpoint) or k_hit_align (full) runs, in the trace arena dsb_ctx_enable_alignment made.
 * DSB_EINVAL unless alignment is on and mode is one of the two.  dsb_ctx_enable_alignment always leaves the mode at FULL. */
int  dsb_ctx_alignment_mode(dsb_ctx *ctx, uint32_t mode);
/* the last batch: one record per hit of dsb_batch_fetch's hits (all zero for a hit that is not counted) and the operation array they
 * index (records lie there in any order, with gaps); valid until the next batch.  DSB_EINVAL before a batch ran with alignment on. */
int  dsb_batch_alignment(dsb_ctx *ctx, const dsb_hit_alignment **recs, const uint32_t **ops, uint64_t *n_ops);
int  dsb_multi_enable_alignment(dsb_multi *m, int on, uint32_t trace_kib, uint64_t ops_cap);
int  dsb_multi_alignment_mode(dsb_multi *m, uint32_t mode);
/* the last dsb_multi_classify_batch: records concatenated as dsb_multi_identity's, ops_off rebased into the one array */
int  dsb_multi_alignment(dsb_multi *m, const dsb_hit_alignment **recs, const uint32_t **ops, uint64_t *n_ops);
/* n_pairs bare alignments by the device functions of k_hit_align, beside dsb_ctx_edit_pairs: same packing, same phases, lengths
 * below 2^28 here.  ident_out and aln_out: n_pairs records each; ops_out: room for ops_cap operations (no automatic size here), of
 * which *ops_used were taken -- the sum of the bounds 2 edits + 1 of the records that have a path and found room. */
int  dsb_ctx_align_pairs(dsb_ctx *ctx, const uint8_t *q_codes, const uint64_t *q_off, const uint32_t *q_len,
                         const uint8_t *t_codes, const uint64_t *t_off, const uint32_t *t_len, size_t n_pairs,
                         uint32_t band, uint32_t max_permille, uint32_t trace_kib,
                         dsb_hit_identity *ident_out, dsb_hit_alignment *aln_out, uint32_t *ops_out, uint64_t ops_cap, uint64_t *ops_used);
/* dsb_ctx_align_pairs (which means DSB_ALN_MODE_FULL) with the mode: DSB_ALN_MODE_CHECKPOINT runs k_pair_align_ck */
int  dsb_ctx_align_pairs_mode(dsb_ctx *ctx, const uint8_t *q_codes, const uint64_t *q_off, const uint32_t *q_len,
                              const uint8_t *t_codes, const uint64_t *t_off, const uint32_t *t_len, size_t n_pairs,
                              uint32_t band, uint32_t max_permille, uint32_t trace_kib, uint32_t mode,
                              dsb_hit_identity *ident_out, dsb_hit_alignment *aln_out, uint32_t *ops_out, uint64_t ops_cap, uint64_t *ops_used);
/* SAM with base-level CIGARs.  Header: @HD VN:1.6 SO:unknown, one @SQ SN LN per reference in ref_ID order, @PG ID:desamba_amd.
 * A read: one line per counted record, in record order (secondaries are not printed; hits, ident and aln: the read's own, rr->n of
 * each; ops: the batch's array):  QNAME FLAG RNAME POS MAPQ CIGAR * 0 0 SEQ QUAL NM:i:edits AS:i:sum_score  -- FLAG and MAPQ as
 * dsb_format_sam prints them, POS = ts + 1, CIGAR = clip, operations, clip with the clips qs and L - qe (left out when 0; S on the
 * primary, H on a supplementary record).  SEQ of the primary is the whole read on the strand the chain was built on (direction 0:
 * the reverse complement, any letter that is not ACGT as N, upper case; QUAL reversed; QUAL * without qualities); of a supplementary
 * record that strand's bases [qs, qe) and their QUAL.  A record without DSB_ALN_OPS: CIGAR *, and xa:i:<alignment flags> where NM
 * stands.  A record whose ref_ID the index does not have: RNAME *, POS 0.  A read without hits:
 * QNAME 4 * 0 0 * * 0 0 SEQ QUAL.  Tabs between the fields, none trailing.  Return as dsb_format_sam. */
long dsb_format_aligned_sam(const dsb_index *idx, const dsb_read *read, const dsb_read_result *rr, const dsb_hit *hits, const dsb_hit_identity *ident,
                            const dsb_hit_alignment *aln, const uint32_t *ops, char *buf, size_t cap);
long dsb_aligned_sam_header(const dsb_index *idx, char *buf, size_t cap);

const char *dsb_strerror(int code);
const char *dsb_version(void);

#ifdef __cplusplus
}
#endif
#endif
