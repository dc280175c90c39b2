"""desamba_amd -- MI355X-native `deSAMBA classify` hot path.

Thin ctypes binding over the C-ABI in include/desamba_amd.h (libdesamba_amd.so, built in-tree by
__graft_entry__.build()).  All compute runs in HIP kernels on gfx950; there is no CPU fallback:
loading fails loudly when the library is missing and Ctx() fails when no gfx950 device is present.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DSB_LIB_PATH", os.path.join(_HERE, "libdesamba_amd.so"))   # override: A/B builds in experiments

DSB_OK, DSB_EIO, DSB_ENODEV, DSB_ENOMEM, DSB_EINVAL, DSB_ECAP = 0, -1, -2, -3, -4, -5


class DsbOpts(C.Structure):
    _fields_ = [("L_min_matching", C.c_int), ("min_score", C.c_int), ("max_sec_N", C.c_int), ("n_slots", C.c_int),
                ("max_read_len", C.c_uint32), ("max_batch_reads", C.c_uint32), ("input_slots", C.c_int), ("reserved", C.c_int), ("max_batch_bases", C.c_uint64)]


class DsbRead(C.Structure):
    _fields_ = [("name", C.c_char_p), ("seq", C.c_char_p), ("qual", C.c_char_p), ("len", C.c_uint32)]


class DsbHit(C.Structure):
    _fields_ = [("ref_ID", C.c_uint32), ("t_st", C.c_uint32), ("t_ed", C.c_uint32), ("q_st", C.c_uint32), ("q_ed", C.c_uint32),
                ("sum_score", C.c_uint32), ("indel", C.c_uint32), ("direction", C.c_uint8), ("primary", C.c_uint8),
                ("pri_index", C.c_uint8), ("pad", C.c_uint8)]

    def key(self):
        return (self.ref_ID, self.t_st, self.t_ed, self.q_st, self.q_ed, self.sum_score, self.direction, self.primary, self.pri_index)


class DsbReadResult(C.Structure):
    _fields_ = [("first", C.c_uint32), ("n", C.c_uint32), ("status", C.c_int32), ("fast", C.c_uint32), ("device_us", C.c_uint32), ("n_anc", C.c_uint32)]


class DsbResult(C.Structure):
    _fields_ = [("reads", C.POINTER(DsbReadResult)), ("hits", C.POINTER(DsbHit)), ("n_hits", C.c_size_t)]


class DsbSeed(C.Structure):
    _fields_ = [("offset", C.c_uint32), ("len", C.c_uint32), ("top", C.c_uint8), ("pad", C.c_uint8 * 3)]


class DsbTiming(C.Structure):
    _fields_ = [("encode_ms", C.c_float), ("seed_probe_ms", C.c_float), ("classify_ms", C.c_float), ("total_ms", C.c_float),
                ("windows", C.c_uint64), ("probes_t1", C.c_uint64), ("bases", C.c_uint64),
                ("order_ms", C.c_float), ("tail_ms", C.c_float), ("n_early", C.c_uint32), ("n_retry", C.c_uint32),
                ("n_regrow", C.c_uint32), ("seed_scan", C.c_uint32),
                ("n_occ", C.c_uint64), ("n_mem", C.c_uint64), ("n_sa", C.c_uint64), ("ref_bases", C.c_uint64),
                ("main_occ", C.c_uint64), ("main_mem", C.c_uint64), ("main_sa", C.c_uint64), ("main_ref_bases", C.c_uint64),
                ("n_heavy_mw", C.c_uint32), ("n_requeue", C.c_uint32), ("upload_bytes", C.c_uint64),
                ("anc_pool_asked", C.c_uint64), ("anc_pool_cap", C.c_uint64)]


class DsbBuildStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_bases", "n_refs", "n_kmer", "n_unitig", "n_rows")] + \
               [(n, C.c_double) for n in ("parse_s", "sort_s", "graph_s", "walk_s", "rows_s", "tables_s", "write_s", "total_s")] + \
               [(n, C.c_uint64) for n in ("budget_bytes", "peak_device_bytes")] + \
               [(n, C.c_uint32) for n in ("ranges_kmers", "ranges_unitig_numbers", "ranges_rows", "ranges_exist")] + \
               [("spilled_bytes", C.c_uint64)]


class DsbReadTaxon(C.Structure):
    _fields_ = [("taxid", C.c_uint32), ("score", C.c_uint32), ("len", C.c_uint32), ("mapq", C.c_uint8), ("flags", C.c_uint8), ("pad", C.c_uint16)]


DSB_TAXON_CLASSIFIED, DSB_TAXON_HOST = 1, 2


class DsbRefCoverage(C.Structure):
    _fields_ = [("numreads", C.c_uint64), ("covbases", C.c_uint64), ("aligned_bases", C.c_uint64), ("mapq_sum", C.c_uint64)]


COVERAGE_FIELDS = ("numreads", "covbases", "aligned_bases", "mapq_sum")
WINDOW_FIELDS = ("starts", "aligned_bases", "covbases")


class DsbEmOpts(C.Structure):
    _fields_ = [("max_iter", C.c_uint32), ("reserved", C.c_uint32), ("tol", C.c_double)]


class DsbAbundanceSummary(C.Structure):
    _fields_ = [("reads", C.c_uint64), ("classified", C.c_uint64), ("classes", C.c_uint64), ("iterations", C.c_uint32),
                ("converged", C.c_uint32), ("max_change", C.c_double), ("min_permille", C.c_uint32), ("reserved", C.c_uint32)]


ABUNDANCE_DTYPE = [("numreads", "<u8"), ("uniqreads", "<u8"), ("est_reads", "<f8"), ("read_share", "<f8"), ("copy_share", "<f8")]


class DsbReadAssign(C.Structure):
    _fields_ = [("ref_ID", C.c_uint32), ("n_cand", C.c_uint32), ("posterior", C.c_double)]


DSB_ASSIGN_NONE = 0xffffffff
ASSIGN_DTYPE = [("ref_ID", "<u4"), ("n_cand", "<u4"), ("posterior", "<f8")]


class DsbReadLca(C.Structure):
    _fields_ = [("taxid", C.c_uint32), ("score", C.c_uint32), ("n_pass", C.c_uint32), ("depth", C.c_uint16), ("flags", C.c_uint8), ("pad", C.c_uint8)]


DSB_LCA_CLASSIFIED, DSB_LCA_NO_TAXON, DSB_LCA_AMBIGUOUS = 1, 2, 4
LCA_DTYPE = [("taxid", "<u4"), ("score", "<u4"), ("n_pass", "<u4"), ("depth", "<u2"), ("flags", "u1"), ("pad", "u1")]
TAXON_COUNT_DTYPE = [("taxid", "<u4"), ("pad", "<u4"), ("clade_reads", "<u8"), ("direct_reads", "<u8")]


class DsbLcaSummary(C.Structure):
    _fields_ = [("reads", C.c_uint64), ("classified", C.c_uint64), ("no_taxon", C.c_uint64), ("ambiguous", C.c_uint64),
                ("min_permille", C.c_uint32), ("reserved", C.c_uint32)]


LCA_SUMMARY_FIELDS = ("reads", "classified", "no_taxon", "ambiguous", "min_permille")


class DsbHitIdentity(C.Structure):
    _fields_ = [("edits", C.c_uint32), ("q_len", C.c_uint32), ("t_len", C.c_uint32), ("flags", C.c_uint32)]


DSB_IDENT_EXACT, DSB_IDENT_OVER, DSB_IDENT_SKEW, DSB_IDENT_EMPTY = 1, 2, 4, 8
DSB_IDENT_MAX_SKEW, DSB_IDENT_MAX_BAND, DSB_IDENT_BAND_DEFAULT, DSB_IDENT_PERMILLE_DEFAULT = 4096, 1024, 256, 300
HIT_IDENTITY_DTYPE = [("edits", "<u4"), ("q_len", "<u4"), ("t_len", "<u4"), ("flags", "<u4")]
REF_IDENTITY_FIELDS = ("records", "q_bases", "t_bases", "edits", "exact", "unaligned")
REF_IDENTITY_DTYPE = [(f, "<u8") for f in REF_IDENTITY_FIELDS]


class DsbHitAlignment(C.Structure):
    _fields_ = [("ops_off", C.c_uint64), ("n_ops", C.c_uint32), ("n_x", C.c_uint32), ("n_ins", C.c_uint32), ("n_del", C.c_uint32),
                ("flags", C.c_uint32), ("pad", C.c_uint32)]


DSB_ALN_OPS, DSB_ALN_NOTRACE, DSB_ALN_NOROOM, DSB_ALN_UNALIGNED = 1, 2, 4, 8
DSB_ALN_OP_I, DSB_ALN_OP_D, DSB_ALN_OP_EQ, DSB_ALN_OP_X = 1, 2, 7, 8
DSB_ALN_TRACE_KIB_DEFAULT, DSB_ALN_TRACE_KIB_MAX = 2048, 65536
DSB_ALN_MODE_FULL, DSB_ALN_MODE_CHECKPOINT = 0, 1
HIT_ALIGNMENT_DTYPE = [("ops_off", "<u8"), ("n_ops", "<u4"), ("n_x", "<u4"), ("n_ins", "<u4"), ("n_del", "<u4"), ("flags", "<u4"), ("pad", "<u4")]


class DsbChunk(C.Structure):
    _fields_ = [("start", C.c_uint64), ("end", C.c_uint64), ("hist_max_before", C.c_uint32), ("rank", C.c_int32)]


EXPORTS = ["dsb_index_open", "dsb_index_close", "dsb_index_n_ref", "dsb_index_ref_name", "dsb_index_ref_len", "dsb_index_ek_len",
           "dsb_index_occ_host", "dsb_ctx_create", "dsb_ctx_destroy", "dsb_ctx_reset_history", "dsb_ctx_reload_env", "dsb_classify_batch",
           "dsb_batch_upload", "dsb_batch_upload_fastq", "dsb_batch_upload_text", "dsb_ctx_set_history", "dsb_host_alloc", "dsb_host_free", "dsb_host_cpus", "dsb_batch_run", "dsb_batch_fetch", "dsb_batch_timing", "dsb_batch_seeds", "dsb_batch_exist_bits",
           "dsb_format_sam", "dsb_format_des", "dsb_strerror", "dsb_version",
           "dsb_device_count", "dsb_ctx_select_slot", "dsb_ctx_create_multi", "dsb_multi_destroy", "dsb_multi_n", "dsb_multi_ctx",
           "dsb_multi_reset_history", "dsb_multi_last_calls", "dsb_multi_classify_batch", "dsb_shard_plan", "dsb_ctx_use_synthetic_filter", "dsb_synthetic_filter_bit", "dsb_index_prefix_interval", "dsb_index_build",
           "dsb_taxonomy_load", "dsb_taxonomy_load_any", "dsb_taxonomy_close", "dsb_taxonomy_max_tid", "dsb_taxonomy_parent",
           "dsb_ctx_set_taxonomy", "dsb_multi_set_taxonomy", "dsb_batch_taxa", "dsb_multi_taxa",
           "dsb_report_create", "dsb_report_add", "dsb_report_add_sam", "dsb_report_format", "dsb_report_destroy",
           "dsb_ctx_enable_coverage", "dsb_ctx_reset_coverage", "dsb_ctx_coverage", "dsb_multi_enable_coverage", "dsb_multi_coverage",
           "dsb_coverage_format", "dsb_coverage_n_windows", "dsb_ctx_enable_coverage_windows", "dsb_ctx_coverage_windows",
           "dsb_multi_enable_coverage_windows", "dsb_multi_coverage_windows", "dsb_coverage_windows_format", "dsb_ctx_enable_abundance", "dsb_ctx_reset_abundance", "dsb_ctx_abundance", "dsb_multi_enable_abundance",
           "dsb_multi_abundance", "dsb_abundance_format",
           "dsb_ctx_set_batch_ordinal", "dsb_ctx_abundance_assign", "dsb_multi_abundance_assign", "dsb_format_assign",
           "dsb_ctx_enable_lca", "dsb_ctx_reset_lca", "dsb_batch_lca", "dsb_ctx_lca_counts", "dsb_multi_enable_lca", "dsb_multi_lca",
           "dsb_multi_lca_counts", "dsb_taxnames_load", "dsb_taxnames_close", "dsb_format_kraken", "dsb_lca_report_format",
           "dsb_ctx_enable_identity", "dsb_ctx_reset_identity", "dsb_batch_identity", "dsb_ctx_identity", "dsb_multi_enable_identity",
           "dsb_multi_identity", "dsb_multi_ref_identity", "dsb_format_identity", "dsb_identity_format", "dsb_index_ref_bases", "dsb_ctx_edit_pairs",
           "dsb_ctx_enable_alignment", "dsb_batch_alignment", "dsb_multi_enable_alignment", "dsb_multi_alignment", "dsb_ctx_align_pairs",
           "dsb_aln_plan", "dsb_ctx_alignment_mode", "dsb_multi_alignment_mode", "dsb_ctx_align_pairs_mode",
           "dsb_format_aligned_sam", "dsb_aligned_sam_header"]

_lib = None


def lib():
    """Load the HIP library; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("desamba_amd: %s is missing -- run __graft_entry__.build(); there is no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    L.dsb_index_open.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
    L.dsb_index_close.argtypes = [C.c_void_p]
    L.dsb_index_n_ref.argtypes = [C.c_void_p]; L.dsb_index_n_ref.restype = C.c_uint64
    L.dsb_index_ref_name.argtypes = [C.c_void_p, C.c_uint32]; L.dsb_index_ref_name.restype = C.c_char_p
    L.dsb_index_ref_len.argtypes = [C.c_void_p, C.c_uint32]; L.dsb_index_ref_len.restype = C.c_uint64
    L.dsb_index_ek_len.argtypes = [C.c_void_p]
    L.dsb_index_occ_host.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint8)]; L.dsb_index_occ_host.restype = C.c_uint64
    L.dsb_ctx_create.argtypes = [C.c_void_p, C.c_int, C.POINTER(DsbOpts), C.POINTER(C.c_void_p)]
    L.dsb_ctx_destroy.argtypes = [C.c_void_p]
    L.dsb_ctx_reset_history.argtypes = [C.c_void_p]
    L.dsb_ctx_reload_env.argtypes = [C.c_void_p]; L.dsb_ctx_reload_env.restype = None
    L.dsb_classify_batch.argtypes = [C.c_void_p, C.POINTER(DsbRead), C.c_size_t, C.POINTER(DsbResult)]
    L.dsb_batch_upload.argtypes = [C.c_void_p, C.POINTER(DsbRead), C.c_size_t]
    L.dsb_batch_upload_fastq.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_size_t]; L.dsb_batch_upload_fastq.restype = C.c_long
    L.dsb_batch_run.argtypes = [C.c_void_p]
    L.dsb_batch_fetch.argtypes = [C.c_void_p, C.POINTER(DsbResult)]
    L.dsb_batch_timing.argtypes = [C.c_void_p, C.POINTER(DsbTiming)]
    L.dsb_batch_seeds.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(DsbSeed), C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.dsb_batch_exist_bits.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_uint32)]
    L.dsb_format_sam.argtypes = [C.c_void_p, C.POINTER(DsbRead), C.POINTER(DsbHit), C.c_uint32, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    L.dsb_format_sam.restype = C.c_long
    L.dsb_format_des.argtypes = [C.c_void_p, C.POINTER(DsbRead), C.POINTER(DsbReadResult), C.POINTER(DsbHit), C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    L.dsb_format_des.restype = C.c_long
    L.dsb_batch_upload_text.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_size_t]
    L.dsb_ctx_set_history.argtypes = [C.c_void_p, C.c_uint32]; L.dsb_ctx_set_history.restype = None
    L.dsb_host_alloc.argtypes = [C.c_size_t]; L.dsb_host_alloc.restype = C.c_void_p
    L.dsb_host_free.argtypes = [C.c_void_p]; L.dsb_host_free.restype = None
    L.dsb_device_count.argtypes = []; L.dsb_device_count.restype = C.c_int
    L.dsb_ctx_select_slot.argtypes = [C.c_void_p, C.c_int]
    L.dsb_ctx_create_multi.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.POINTER(DsbOpts), C.POINTER(C.c_void_p)]
    L.dsb_multi_destroy.argtypes = [C.c_void_p]; L.dsb_multi_destroy.restype = None
    L.dsb_multi_n.argtypes = [C.c_void_p]
    L.dsb_multi_ctx.argtypes = [C.c_void_p, C.c_int]; L.dsb_multi_ctx.restype = C.c_void_p
    L.dsb_multi_reset_history.argtypes = [C.c_void_p]; L.dsb_multi_reset_history.restype = None
    L.dsb_multi_last_calls.argtypes = [C.c_void_p, C.c_int]; L.dsb_multi_last_calls.restype = C.c_uint32
    L.dsb_multi_classify_batch.argtypes = [C.c_void_p, C.POINTER(DsbRead), C.c_size_t, C.POINTER(DsbResult)]
    L.dsb_shard_plan.argtypes = [C.POINTER(C.c_uint32), C.c_size_t, C.c_int, C.c_uint64, C.c_uint32, C.POINTER(DsbChunk), C.c_size_t, C.POINTER(C.c_size_t)]
    L.dsb_ctx_use_synthetic_filter.argtypes = [C.c_void_p, C.c_uint64, C.c_double]
    L.dsb_synthetic_filter_bit.argtypes = [C.c_int, C.c_uint64, C.c_double]
    L.dsb_index_prefix_interval.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.dsb_index_build.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(DsbBuildStats)]
    L.dsb_index_close.restype = None; L.dsb_ctx_destroy.restype = None; L.dsb_ctx_reset_history.restype = None
    L.dsb_taxonomy_load.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
    L.dsb_taxonomy_load_any.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
    L.dsb_taxonomy_close.argtypes = [C.c_void_p]; L.dsb_taxonomy_close.restype = None
    L.dsb_taxonomy_max_tid.argtypes = [C.c_void_p]; L.dsb_taxonomy_max_tid.restype = C.c_uint32
    L.dsb_taxonomy_parent.argtypes = [C.c_void_p, C.c_uint32]; L.dsb_taxonomy_parent.restype = C.c_uint32
    L.dsb_ctx_set_taxonomy.argtypes = [C.c_void_p, C.c_void_p]
    L.dsb_multi_set_taxonomy.argtypes = [C.c_void_p, C.c_void_p]
    L.dsb_batch_taxa.argtypes = [C.c_void_p, C.POINTER(C.POINTER(DsbReadTaxon))]
    L.dsb_multi_taxa.argtypes = [C.c_void_p, C.POINTER(C.POINTER(DsbReadTaxon))]
    L.dsb_report_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.dsb_report_add.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(DsbRead), C.POINTER(DsbResult), C.POINTER(DsbReadTaxon), C.c_size_t, C.c_int]
    L.dsb_report_add_sam.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.dsb_report_format.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t]; L.dsb_report_format.restype = C.c_long
    L.dsb_report_destroy.argtypes = [C.c_void_p]; L.dsb_report_destroy.restype = None
    L.dsb_ctx_enable_coverage.argtypes = [C.c_void_p, C.c_int]
    L.dsb_ctx_reset_coverage.argtypes = [C.c_void_p]
    L.dsb_ctx_coverage.argtypes = [C.c_void_p, C.c_void_p]
    L.dsb_multi_enable_coverage.argtypes = [C.c_void_p, C.c_int]
    L.dsb_multi_coverage.argtypes = [C.c_void_p, C.c_void_p]
    L.dsb_coverage_format.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]; L.dsb_coverage_format.restype = C.c_long
    L.dsb_coverage_n_windows.argtypes = [C.c_void_p, C.c_uint32]; L.dsb_coverage_n_windows.restype = C.c_uint64
    L.dsb_ctx_enable_coverage_windows.argtypes = [C.c_void_p, C.c_uint32]
    L.dsb_ctx_coverage_windows.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.dsb_multi_enable_coverage_windows.argtypes = [C.c_void_p, C.c_uint32]
    L.dsb_multi_coverage_windows.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.dsb_coverage_windows_format.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_char_p, C.c_size_t]; L.dsb_coverage_windows_format.restype = C.c_long
    L.dsb_ctx_enable_abundance.argtypes = [C.c_void_p, C.c_int, C.c_uint32]
    L.dsb_ctx_reset_abundance.argtypes = [C.c_void_p]
    L.dsb_ctx_abundance.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dsb_multi_enable_abundance.argtypes = [C.c_void_p, C.c_int, C.c_uint32]
    L.dsb_multi_abundance.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dsb_abundance_format.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]; L.dsb_abundance_format.restype = C.c_long
    L.dsb_ctx_set_batch_ordinal.argtypes = [C.c_void_p, C.c_uint64]
    L.dsb_ctx_abundance_assign.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.dsb_multi_abundance_assign.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.dsb_format_assign.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]; L.dsb_format_assign.restype = C.c_long
    L.dsb_ctx_enable_lca.argtypes = [C.c_void_p, C.c_int, C.c_uint32]
    L.dsb_ctx_reset_lca.argtypes = [C.c_void_p]
    L.dsb_batch_lca.argtypes = [C.c_void_p, C.POINTER(C.POINTER(DsbReadLca))]
    L.dsb_ctx_lca_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]
    L.dsb_multi_enable_lca.argtypes = [C.c_void_p, C.c_int, C.c_uint32]
    L.dsb_multi_lca.argtypes = [C.c_void_p, C.POINTER(C.POINTER(DsbReadLca))]
    L.dsb_multi_lca_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]
    L.dsb_taxnames_load.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
    L.dsb_taxnames_close.argtypes = [C.c_void_p]; L.dsb_taxnames_close.restype = None
    L.dsb_format_kraken.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]; L.dsb_format_kraken.restype = C.c_long
    L.dsb_lca_report_format.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_char_p, C.c_size_t]; L.dsb_lca_report_format.restype = C.c_long
    L.dsb_ctx_enable_identity.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32]
    L.dsb_ctx_reset_identity.argtypes = [C.c_void_p]
    L.dsb_batch_identity.argtypes = [C.c_void_p, C.POINTER(C.POINTER(DsbHitIdentity))]
    L.dsb_ctx_identity.argtypes = [C.c_void_p, C.c_void_p]
    L.dsb_multi_enable_identity.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32]
    L.dsb_multi_identity.argtypes = [C.c_void_p, C.POINTER(C.POINTER(DsbHitIdentity))]
    L.dsb_multi_ref_identity.argtypes = [C.c_void_p, C.c_void_p]
    L.dsb_format_identity.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]; L.dsb_format_identity.restype = C.c_long
    L.dsb_identity_format.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]; L.dsb_identity_format.restype = C.c_long
    L.dsb_index_ref_bases.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p]
    L.dsb_ctx_edit_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p]
    L.dsb_ctx_enable_alignment.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint64]
    L.dsb_batch_alignment.argtypes = [C.c_void_p, C.POINTER(C.POINTER(DsbHitAlignment)), C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_uint64)]
    L.dsb_multi_enable_alignment.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint64]
    L.dsb_multi_alignment.argtypes = [C.c_void_p, C.POINTER(C.POINTER(DsbHitAlignment)), C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_uint64)]
    L.dsb_ctx_align_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.dsb_aln_plan.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.dsb_ctx_alignment_mode.argtypes = [C.c_void_p, C.c_uint32]
    L.dsb_multi_alignment_mode.argtypes = [C.c_void_p, C.c_uint32]
    L.dsb_ctx_align_pairs_mode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32,
                                           C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.dsb_format_aligned_sam.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]; L.dsb_format_aligned_sam.restype = C.c_long
    L.dsb_aligned_sam_header.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]; L.dsb_aligned_sam_header.restype = C.c_long
    L.dsb_strerror.argtypes = [C.c_int]; L.dsb_strerror.restype = C.c_char_p
    L.dsb_version.restype = C.c_char_p
    _lib = L
    return L


class DsbError(RuntimeError):
    def __init__(self, code, what):
        RuntimeError.__init__(self, "%s: %s (%d)" % (what, lib().dsb_strerror(code).decode(), code))
        self.code = code


class Index:
    """load_idx (src/idx.c:1103): the ten deSAMBA.* files of an index directory."""

    def __init__(self, path):
        self.h = C.c_void_p()
        rc = lib().dsb_index_open(os.fsencode(path), C.byref(self.h))
        if rc != 0:
            raise DsbError(rc, "dsb_index_open(%s)" % path)
        self.path = path

    def close(self):
        if self.h:
            lib().dsb_index_close(self.h); self.h = C.c_void_p()

    @property
    def n_ref(self):
        return lib().dsb_index_n_ref(self.h)

    @property
    def ek_len(self):
        return lib().dsb_index_ek_len(self.h)

    def ref_name(self, i):
        return lib().dsb_index_ref_name(self.h, i).decode()

    def ref_len(self, i):
        return int(lib().dsb_index_ref_len(self.h, i))

    def ref_bases(self, i, start, length):
        """bases [start, start + length) of reference i from the host copy of the 2-bit text: numpy u8 codes (0 A, 1 C, 2 G, 3 T)"""
        import numpy as np
        out = np.zeros(int(length), dtype=np.uint8)
        rc = lib().dsb_index_ref_bases(self.h, int(i), int(start), int(length), out.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise DsbError(rc, "dsb_index_ref_bases(%d, %d, %d)" % (i, start, length))
        return out

    def occ_host(self, r, c):
        cc = C.c_uint8(c)
        v = lib().dsb_index_occ_host(self.h, r, C.byref(cc))
        return v, cc.value


def build_index(fasta, out_dir, kmer_srt=None, device=0):
    """`deSAMBA index` on the GPU (build_index_main, src/idx.c:1254-1282): writes the deSAMBA.* files of an index
    directory from a reference FASTA; kmer_srt=None enumerates the 31-mers from the FASTA itself.  Returns DsbBuildStats."""
    st = DsbBuildStats()
    rc = lib().dsb_index_build(kmer_srt.encode() if kmer_srt else None, fasta.encode(), out_dir.encode(), device, C.byref(st))
    if rc != 0:
        raise DsbError(rc, "dsb_index_build(%s)" % fasta)
    return st


def make_reads(records):
    """records: list of (name, seq, qual) of bytes/str -> ctypes array (keeps the buffers alive)."""
    n = len(records)
    arr = (DsbRead * n)()
    keep = []
    for i, (name, seq, qual) in enumerate(records):
        name = name if isinstance(name, bytes) else name.encode()
        seq = seq if isinstance(seq, bytes) else seq.encode()
        qual = (qual if isinstance(qual, bytes) else qual.encode()) if qual is not None else None
        keep.append((name, seq, qual))
        arr[i].name, arr[i].seq, arr[i].qual, arr[i].len = name, seq, qual, len(seq)
    arr._keep = keep
    return arr


class Ctx:
    """classify_main's set-up (src/cly_mt.c:518-550) on one GPU."""

    def __init__(self, index, device=0, L_min_matching=170, min_score=64, max_sec_N=5, n_slots=0, max_read_len=0, max_batch_reads=0, input_slots=1, max_batch_bases=0):
        self.index = index
        self.opts = DsbOpts(L_min_matching, min_score, max_sec_N, n_slots, max_read_len, max_batch_reads, input_slots, 0, max_batch_bases)
        self.h = C.c_void_p()
        rc = lib().dsb_ctx_create(index.h, device, C.byref(self.opts), C.byref(self.h))
        if rc != 0:
            raise DsbError(rc, "dsb_ctx_create(device %d)" % device)
        self.reads = None
        # (reads, count) staged in each input slot, and those of the batch the last run() ran: taxa(), sam() and in_last_batch()
        # speak of that batch, as dsb_batch_taxa does
        self.slot = 0
        self.staged = {}
        self.ran = (None, 0)

    def close(self):
        if self.h:
            lib().dsb_ctx_destroy(self.h); self.h = C.c_void_p()

    def reset_history(self):
        lib().dsb_ctx_reset_history(self.h)

    def reload_env(self):
        """the DSB_* switches are read once, when the ctx is made: read them again (tests that change them on a living ctx)"""
        lib().dsb_ctx_reload_env(self.h)

    def set_history(self, max_len_before):
        lib().dsb_ctx_set_history(self.h, max_len_before)

    def use_synthetic_filter(self, table_bytes, fill):
        """measurement hook: synthetic exist-kmer tables for this ctx (seed lookup only); upload the batch afterwards"""
        rc = lib().dsb_ctx_use_synthetic_filter(self.h, table_bytes, fill)
        if rc != 0:
            raise DsbError(rc, "dsb_ctx_use_synthetic_filter")
        self.synthetic = (table_bytes, fill)
        self.synthetic_k = {27: 16, 28: 17, 29: 17, 30: 18, 31: 18, 32: 19, 33: 19, 34: 20}[int(table_bytes).bit_length() - 1]

    def select_slot(self, slot):
        rc = lib().dsb_ctx_select_slot(self.h, slot)
        if rc != 0:
            raise DsbError(rc, "dsb_ctx_select_slot(%d)" % slot)
        self.slot = slot

    def upload_text(self, text_ptr, text_len, seq_off, seq_len, n):
        """sequences inside one host blob (pinned if it came from dsb_host_alloc): one H2D copy, no per-read gather"""
        self.reads = None
        rc = lib().dsb_batch_upload_text(self.h, text_ptr, text_len, seq_off, seq_len, n)
        if rc != 0:
            raise DsbError(rc, "dsb_batch_upload_text")
        self.staged[self.slot] = (None, int(n))

    def upload(self, reads):
        self.reads = reads
        rc = lib().dsb_batch_upload(self.h, reads, len(reads))
        if rc != 0:
            raise DsbError(rc, "dsb_batch_upload")
        self.staged[self.slot] = (reads, len(reads))

    def upload_fastq(self, path, skip=0, max_reads=1 << 62):
        """stage a plain-text FASTQ file straight into HBM; returns the number of reads"""
        self.reads = None
        n = lib().dsb_batch_upload_fastq(self.h, os.fsencode(path), skip, max_reads)
        if n < 0:
            raise DsbError(int(n), "dsb_batch_upload_fastq(%s)" % path)
        self.n_uploaded = int(n)
        self.staged[self.slot] = (None, int(n))
        return int(n)

    def run(self):
        rc = lib().dsb_batch_run(self.h)
        if rc != 0:
            raise DsbError(rc, "dsb_batch_run")
        self.ran = self.staged.get(self.slot, (None, 0))

    def fetch(self, strict=True):
        res = DsbResult()
        rc = lib().dsb_batch_fetch(self.h, C.byref(res))
        if rc != 0 and (strict or rc != DSB_ECAP):
            raise DsbError(rc, "dsb_batch_fetch")
        return res

    def classify(self, reads, strict=True):
        self.upload(reads); self.run()
        return self.fetch(strict)

    def timing(self):
        t = DsbTiming()
        lib().dsb_batch_timing(self.h, C.byref(t))
        return t

    def read_len(self, read):
        """length of a read of the staged batch, whichever way it was uploaded (the library knows: windows + k - 1; 0 for a read
        shorter than 40 bases, which has no windows)"""
        reads = self.staged.get(self.slot, (self.reads, 0))[0] or self.reads
        if reads is not None:
            return reads[read].len
        n = C.c_uint32()
        lib().dsb_batch_exist_bits(self.h, read, 1, None, 0, C.byref(n))      # (too small a buffer: only the number of windows comes back)
        k = self.synthetic_k if getattr(self, "synthetic", None) else self.index.ek_len
        return n.value + k - 1 if n.value else 0

    def seeds(self, read, strand):
        cap = (self.read_len(read) >> 1) + 64
        buf = (DsbSeed * cap)(); n = C.c_uint32(); ts = C.c_uint32()
        rc = lib().dsb_batch_seeds(self.h, read, strand, buf, cap, C.byref(n), C.byref(ts))
        if rc != 0:
            raise DsbError(rc, "dsb_batch_seeds")
        return [(buf[i].offset, buf[i].len, buf[i].top) for i in range(n.value)], ts.value

    def exist_bits(self, read, strand):
        n = C.c_uint32()
        lib().dsb_batch_exist_bits(self.h, read, strand, None, 0, C.byref(n))        # the number of windows first
        cap = n.value + 1
        buf = (C.c_uint8 * cap)()
        rc = lib().dsb_batch_exist_bits(self.h, read, strand, buf, cap, C.byref(n))
        if rc != 0:
            raise DsbError(rc, "dsb_batch_exist_bits")
        return bytes(buf[:n.value])

    def set_taxonomy(self, taxonomy):
        """attach a Taxonomy (None detaches): every batch from now on ends with the per-read taxon kernel"""
        rc = lib().dsb_ctx_set_taxonomy(self.h, taxonomy.h if taxonomy is not None else None)
        if rc != 0:
            raise DsbError(rc, "dsb_ctx_set_taxonomy")
        self.taxonomy = taxonomy

    def taxa(self, records=False):
        """the taxon of each read of the last batch (numpy u32, 0 = unclassified): the walk over the read's own records;
        records=True: the DsbReadTaxon array itself (what Report.add takes)"""
        p = C.POINTER(DsbReadTaxon)()
        rc = lib().dsb_batch_taxa(self.h, C.byref(p))
        if rc != 0:
            raise DsbError(rc, "dsb_batch_taxa")
        n = self.in_last_batch()
        return _taxa(p, n, records)

    def enable_coverage(self, on=True):
        """per-reference coverage from now on (a bitmap of one bit per reference base in HBM), or off (freed)"""
        rc = lib().dsb_ctx_enable_coverage(self.h, 1 if on else 0)
        if rc != 0:
            raise DsbError(rc, "dsb_ctx_enable_coverage")

    def reset_coverage(self):
        rc = lib().dsb_ctx_reset_coverage(self.h)
        if rc != 0:
            raise DsbError(rc, "dsb_ctx_reset_coverage")

    def coverage(self):
        """everything since enable / reset: numpy structured array of n_ref rows (COVERAGE_FIELDS, u64)"""
        return _coverage(lib().dsb_ctx_coverage, self.h, self.index.n_ref, "dsb_ctx_coverage")

    def enable_coverage_windows(self, window=1000):
        """per-window coverage from now on (coverage must be on; the whole coverage state is zeroed), or off for window 0"""
        rc = lib().dsb_ctx_enable_coverage_windows(self.h, int(window))
        if rc != 0:
            raise DsbError(rc, "dsb_ctx_enable_coverage_windows")

    def coverage_windows(self):
        """everything since enable / reset: numpy structured array of n_coverage_windows rows (WINDOW_FIELDS, u64)"""
        return _coverage_windows(lib().dsb_ctx_coverage_windows, self.h, "dsb_ctx_coverage_windows")

    def enable_abundance(self, on=True, min_frac=0.95):
        """per-reference abundance by EM from now on (each read's candidate set kept in HBM), or off (freed).  min_frac: a read's
        candidates are the references whose best AS is at least min_frac x its best AS (0 < min_frac <= 1, in steps of 0.001)"""
        rc = lib().dsb_ctx_enable_abundance(self.h, 1 if on else 0, _permille(min_frac) if on else 0)
        if rc != 0:
            raise DsbError(rc, "dsb_ctx_enable_abundance")

    def reset_abundance(self):
        rc = lib().dsb_ctx_reset_abundance(self.h)
        if rc != 0:
            raise DsbError(rc, "dsb_ctx_reset_abundance")

    def abundance(self, max_iter=10000, tol=0.01):
        """EM over everything since enable / reset: (numpy structured array of n_ref rows, ABUNDANCE_DTYPE; summary dict)"""
        return _abundance(lib().dsb_ctx_abundance, self.h, self.index.n_ref, max_iter, tol, "dsb_ctx_abundance")

    def set_batch_ordinal(self, first):
        """read i of the batch staged in the selected slot is read first + i of the input (abundance_assign's order); holds for that
        slot's next run() / classify() alone.  Not set: the reads this context has collected since enable / reset."""
        rc = lib().dsb_ctx_set_batch_ordinal(self.h, int(first))
        if rc != 0:
            raise DsbError(rc, "dsb_ctx_set_batch_ordinal")

    def abundance_assign(self, max_iter=10000, tol=0.01):
        """abundance(), and each read assigned to one reference by its EM posterior: (ab, summary, records) -- records in input
        order (ASSIGN_DTYPE: ref_ID, DSB_ASSIGN_NONE for an unclassified read; n_cand; posterior)"""
        return _abundance_assign(lib().dsb_ctx_abundance_assign, self.h, self.index.n_ref, max_iter, tol, "dsb_ctx_abundance_assign")

    def enable_lca(self, on=True, min_frac=0.95):
        """per-read classification by the LCA of the near-best hits from now on (needs a Taxonomy attached), or off (freed).  min_frac: a
        hit takes part when its AS is at least min_frac x the read's best AS (0 < min_frac <= 1, in steps of 0.001)"""
        rc = lib().dsb_ctx_enable_lca(self.h, 1 if on else 0, _permille(min_frac) if on else 0)
        if rc != 0:
            raise DsbError(rc, "dsb_ctx_enable_lca")

    def reset_lca(self):
        rc = lib().dsb_ctx_reset_lca(self.h)
        if rc != 0:
            raise DsbError(rc, "dsb_ctx_reset_lca")

    def lca(self):
        """the LCA record of each read of the last batch: numpy structured array (LCA_DTYPE)"""
        p = C.POINTER(DsbReadLca)()
        rc = lib().dsb_batch_lca(self.h, C.byref(p))
        if rc != 0:
            raise DsbError(rc, "dsb_batch_lca")
        return _lca(p, self.in_last_batch())

    def lca_counts(self):
        """everything since enable / reset: (the taxa with clade_reads > 0 in ascending taxid, TAXON_COUNT_DTYPE; summary dict)"""
        return _lca_counts(lib().dsb_ctx_lca_counts, self.h, "dsb_ctx_lca_counts")

    def enable_identity(self, on=True, band=None, max_frac=None):
        """per-hit edit distance and per-reference identity from now on (banded alignment of every primary and supplementary record),
        or off (freed).  band: diagonals on either side of the corridor, 0 .. 1024 [256]; max_frac: a record with more edits than
        max_frac x its length is reported as over the cap, 0 < max_frac <= 1 in steps of 0.001 [0.3]"""
        b = DSB_IDENT_BAND_DEFAULT if band is None else int(band)
        p = DSB_IDENT_PERMILLE_DEFAULT if max_frac is None else _permille(max_frac)
        rc = lib().dsb_ctx_enable_identity(self.h, 1 if on else 0, b if on else 0, p if on else 0)
        if rc != 0:
            raise DsbError(rc, "dsb_ctx_enable_identity")

    def reset_identity(self):
        rc = lib().dsb_ctx_reset_identity(self.h)
        if rc != 0:
            raise DsbError(rc, "dsb_ctx_reset_identity")

    def identity(self, n_hits):
        """the identity record of each hit of the last batch (n_hits = its result's n_hits): numpy structured array (HIT_IDENTITY_DTYPE)"""
        p = C.POINTER(DsbHitIdentity)()
        rc = lib().dsb_batch_identity(self.h, C.byref(p))
        if rc != 0:
            raise DsbError(rc, "dsb_batch_identity")
        return _hit_identity(p, int(n_hits))

    def ref_identity(self):
        """everything since enable / reset: numpy structured array of n_ref rows (REF_IDENTITY_FIELDS, u64)"""
        return _ref_identity(lib().dsb_ctx_identity, self.h, self.index.n_ref, "dsb_ctx_identity")

    def edit_pairs(self, q_codes, q_off, q_len, t_codes, t_off, t_len, band=DSB_IDENT_BAND_DEFAULT, max_permille=DSB_IDENT_PERMILLE_DEFAULT):
        """dsb_ctx_edit_pairs: pair p aligns q_codes[q_off[p] : q_off[p] + q_len[p]] with t_codes[t_off[p] : ...] (u8 codes 0 .. 3) by the
        device function of k_hit_edits; returns a numpy structured array of one record per pair (HIT_IDENTITY_DTYPE)"""
        import numpy as np
        qc = np.ascontiguousarray(q_codes, dtype=np.uint8); tc = np.ascontiguousarray(t_codes, dtype=np.uint8)
        qo = np.ascontiguousarray(q_off, dtype=np.uint64); to = np.ascontiguousarray(t_off, dtype=np.uint64)
        ql = np.ascontiguousarray(q_len, dtype=np.uint32); tl = np.ascontiguousarray(t_len, dtype=np.uint32)
        n = len(qo)
        if not (len(to) == len(ql) == len(tl) == n):
            raise ValueError("edit_pairs: the four offset and length arrays differ in length")
        if n and (int((qo + ql).max()) > len(qc) or int((to + tl).max()) > len(tc)):
            raise ValueError("edit_pairs: a pair reaches beyond its codes")
        out = np.zeros(n, dtype=HIT_IDENTITY_DTYPE)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = lib().dsb_ctx_edit_pairs(self.h, p(qc), p(qo), p(ql), p(tc), p(to), p(tl), n, int(band), int(max_permille), p(out))
        if rc != 0:
            raise DsbError(rc, "dsb_ctx_edit_pairs")
        return out

    def enable_alignment(self, on=True, trace_kib=0, ops_cap=0):
        """base-level alignment of every counted record from now on (needs enable_identity; uses its band and cap), or off (freed).
        trace_kib: KiB of trace per wavefront, 1 .. 65536 [2048]; ops_cap: operations the batch's array holds [0: sized per batch]"""
        rc = lib().dsb_ctx_enable_alignment(self.h, 1 if on else 0, int(trace_kib) if on else 0, int(ops_cap) if on else 0)
        if rc != 0:
            raise DsbError(rc, "dsb_ctx_enable_alignment")

    def alignment_mode(self, mode):
        """dsb_ctx_alignment_mode: DSB_ALN_MODE_FULL or DSB_ALN_MODE_CHECKPOINT from the next batch on (needs enable_alignment, which
        always leaves the mode at FULL)"""
        rc = lib().dsb_ctx_alignment_mode(self.h, int(mode))
        if rc != 0:
            raise DsbError(rc, "dsb_ctx_alignment_mode")

    def alignment(self, n_hits):
        """(records, ops) of the last batch: one record per hit (HIT_ALIGNMENT_DTYPE) and the uint32 operation array they index"""
        return _alignment(lib().dsb_batch_alignment, self.h, int(n_hits), "dsb_batch_alignment")

    def align_pairs(self, q_codes, q_off, q_len, t_codes, t_off, t_len, band=DSB_IDENT_BAND_DEFAULT, max_permille=DSB_IDENT_PERMILLE_DEFAULT,
                    trace_kib=DSB_ALN_TRACE_KIB_DEFAULT, ops_cap=None, mode=DSB_ALN_MODE_FULL):
        """dsb_ctx_align_pairs_mode: edit_pairs with the path kept; returns (identity records, alignment records, ops).  ops_cap: room
        of the operation array [None: an operation per base of Q and T plus one per pair -- never short]; mode: DSB_ALN_MODE_FULL, or
        DSB_ALN_MODE_CHECKPOINT for the checkpointed traceback"""
        import numpy as np
        qc = np.ascontiguousarray(q_codes, dtype=np.uint8); tc = np.ascontiguousarray(t_codes, dtype=np.uint8)
        qo = np.ascontiguousarray(q_off, dtype=np.uint64); to = np.ascontiguousarray(t_off, dtype=np.uint64)
        ql = np.ascontiguousarray(q_len, dtype=np.uint32); tl = np.ascontiguousarray(t_len, dtype=np.uint32)
        n = len(qo)
        if not (len(to) == len(ql) == len(tl) == n):
            raise ValueError("align_pairs: the four offset and length arrays differ in length")
        if n and (int((qo + ql).max()) > len(qc) or int((to + tl).max()) > len(tc)):
            raise ValueError("align_pairs: a pair reaches beyond its codes")
        if ops_cap is None:
            ops_cap = 2 * (int(ql.astype(np.uint64).sum()) + int(tl.astype(np.uint64).sum())) + n    # (2 edits + 1 <= 2 max(n, m) + 1 per pair)
        ident = np.zeros(n, dtype=HIT_IDENTITY_DTYPE); aln = np.zeros(n, dtype=HIT_ALIGNMENT_DTYPE); ops = np.zeros(max(int(ops_cap), 1), dtype=np.uint32)
        used = C.c_uint64(0)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = lib().dsb_ctx_align_pairs_mode(self.h, p(qc), p(qo), p(ql), p(tc), p(to), p(tl), n, int(band), int(max_permille), int(trace_kib), int(mode),
                                            p(ident), p(aln), p(ops), int(ops_cap), C.byref(used))
        if rc != 0:
            raise DsbError(rc, "dsb_ctx_align_pairs")
        return ident, aln, ops[:used.value]

    def in_last_batch(self):
        return self.ran[1]

    def sam(self, res, full=False, reads=None):
        """Format a whole batch exactly as output_one_result_sam does (src/cly_mt.c:245-344)."""
        if reads is None:
            reads = self.ran[0] if self.ran[0] is not None else self.reads      # (a batch staged from text: names set by the caller)
        return format_sam(self.index, reads, res, self.opts.max_sec_N, full)


def format_sam(index, reads, res, max_sec_N=5, full=False):
    out = []
    buf = C.create_string_buffer(1 << 20)
    for i in range(len(reads)):
        rr = res.reads[i]
        hits = C.cast(C.byref(res.hits.contents, rr.first * C.sizeof(DsbHit)), C.POINTER(DsbHit)) if rr.n else None
        cap = len(buf)
        need = 4096 + 700 * rr.n + (2 * reads[i].len if full else 0)
        if need > cap:
            buf = C.create_string_buffer(need)
        n = lib().dsb_format_sam(index.h, C.byref(reads[i]), hits, rr.n, max_sec_N, 1 if full else 0, buf, len(buf))
        if n < 0:
            raise DsbError(DSB_EINVAL, "dsb_format_sam")
        out.append(buf.raw[:n])
    return b"".join(out)


class Multi:
    """dsb_ctx_create_multi: one context per listed device; classify() shards a batch over them (no collective)."""

    def __init__(self, index, devices, L_min_matching=170, min_score=64, max_sec_N=5, n_slots=0):
        self.index = index
        self.opts = DsbOpts(L_min_matching, min_score, max_sec_N, n_slots, 0, 0, 1, 0)
        ids = (C.c_int * len(devices))(*devices)
        self.h = C.c_void_p()
        rc = lib().dsb_ctx_create_multi(index.h, ids, len(devices), C.byref(self.opts), C.byref(self.h))
        if rc != 0:
            raise DsbError(rc, "dsb_ctx_create_multi(%r)" % (devices,))

    def close(self):
        if self.h:
            lib().dsb_multi_destroy(self.h); self.h = C.c_void_p()

    def reset_history(self):
        lib().dsb_multi_reset_history(self.h)

    def last_calls(self):
        """dsb_classify_batch calls each context made in the last classify()"""
        return [int(lib().dsb_multi_last_calls(self.h, i)) for i in range(int(lib().dsb_multi_n(self.h)))]

    def classify(self, reads, strict=True):
        res = DsbResult()
        rc = lib().dsb_multi_classify_batch(self.h, reads, len(reads), C.byref(res))
        if rc != 0 and (strict or rc != DSB_ECAP):
            raise DsbError(rc, "dsb_multi_classify_batch")
        self.n_last = len(reads)
        return res

    def set_taxonomy(self, taxonomy):
        rc = lib().dsb_multi_set_taxonomy(self.h, taxonomy.h if taxonomy is not None else None)
        if rc != 0:
            raise DsbError(rc, "dsb_multi_set_taxonomy")
        self.taxonomy = taxonomy

    def enable_coverage(self, on=True):
        rc = lib().dsb_multi_enable_coverage(self.h, 1 if on else 0)
        if rc != 0:
            raise DsbError(rc, "dsb_multi_enable_coverage")

    def coverage(self):
        """Ctx.coverage merged over the contexts"""
        return _coverage(lib().dsb_multi_coverage, self.h, self.index.n_ref, "dsb_multi_coverage")

    def enable_coverage_windows(self, window=1000):
        rc = lib().dsb_multi_enable_coverage_windows(self.h, int(window))
        if rc != 0:
            raise DsbError(rc, "dsb_multi_enable_coverage_windows")

    def coverage_windows(self):
        """Ctx.coverage_windows merged over the contexts"""
        return _coverage_windows(lib().dsb_multi_coverage_windows, self.h, "dsb_multi_coverage_windows")

    def enable_abundance(self, on=True, min_frac=0.95):
        rc = lib().dsb_multi_enable_abundance(self.h, 1 if on else 0, _permille(min_frac) if on else 0)
        if rc != 0:
            raise DsbError(rc, "dsb_multi_enable_abundance")

    def reset_abundance(self):
        for i in range(int(lib().dsb_multi_n(self.h))):
            rc = lib().dsb_ctx_reset_abundance(lib().dsb_multi_ctx(self.h, i))
            if rc != 0:
                raise DsbError(rc, "dsb_ctx_reset_abundance")

    def abundance(self, max_iter=10000, tol=0.01):
        """Ctx.abundance over the contexts' reads together"""
        return _abundance(lib().dsb_multi_abundance, self.h, self.index.n_ref, max_iter, tol, "dsb_multi_abundance")

    def abundance_assign(self, max_iter=10000, tol=0.01):
        """Ctx.abundance_assign over the contexts' reads together, in the input order of the classify() calls"""
        return _abundance_assign(lib().dsb_multi_abundance_assign, self.h, self.index.n_ref, max_iter, tol, "dsb_multi_abundance_assign")

    def enable_lca(self, on=True, min_frac=0.95):
        rc = lib().dsb_multi_enable_lca(self.h, 1 if on else 0, _permille(min_frac) if on else 0)
        if rc != 0:
            raise DsbError(rc, "dsb_multi_enable_lca")

    def reset_lca(self):
        for i in range(int(lib().dsb_multi_n(self.h))):
            rc = lib().dsb_ctx_reset_lca(lib().dsb_multi_ctx(self.h, i))
            if rc != 0:
                raise DsbError(rc, "dsb_ctx_reset_lca")

    def lca(self):
        """Ctx.lca for the last classify(), in input order"""
        p = C.POINTER(DsbReadLca)()
        rc = lib().dsb_multi_lca(self.h, C.byref(p))
        if rc != 0:
            raise DsbError(rc, "dsb_multi_lca")
        return _lca(p, getattr(self, "n_last", 0))

    def lca_counts(self):
        """Ctx.lca_counts over the contexts' reads together"""
        return _lca_counts(lib().dsb_multi_lca_counts, self.h, "dsb_multi_lca_counts")

    def enable_identity(self, on=True, band=None, max_frac=None):
        b = DSB_IDENT_BAND_DEFAULT if band is None else int(band)
        p = DSB_IDENT_PERMILLE_DEFAULT if max_frac is None else _permille(max_frac)
        rc = lib().dsb_multi_enable_identity(self.h, 1 if on else 0, b if on else 0, p if on else 0)
        if rc != 0:
            raise DsbError(rc, "dsb_multi_enable_identity")

    def identity(self, n_hits):
        """Ctx.identity for the last classify(): one record per hit of its result"""
        p = C.POINTER(DsbHitIdentity)()
        rc = lib().dsb_multi_identity(self.h, C.byref(p))
        if rc != 0:
            raise DsbError(rc, "dsb_multi_identity")
        return _hit_identity(p, int(n_hits))

    def ref_identity(self):
        """Ctx.ref_identity added over the contexts"""
        return _ref_identity(lib().dsb_multi_ref_identity, self.h, self.index.n_ref, "dsb_multi_ref_identity")

    def enable_alignment(self, on=True, trace_kib=0, ops_cap=0):
        """Ctx.enable_alignment on every context"""
        rc = lib().dsb_multi_enable_alignment(self.h, 1 if on else 0, int(trace_kib) if on else 0, int(ops_cap) if on else 0)
        if rc != 0:
            raise DsbError(rc, "dsb_multi_enable_alignment")

    def alignment_mode(self, mode):
        """Ctx.alignment_mode on every context"""
        rc = lib().dsb_multi_alignment_mode(self.h, int(mode))
        if rc != 0:
            raise DsbError(rc, "dsb_multi_alignment_mode")

    def alignment(self, n_hits):
        """Ctx.alignment for the last classify(): one record per hit of its result, ops_off rebased into the one array"""
        return _alignment(lib().dsb_multi_alignment, self.h, int(n_hits), "dsb_multi_alignment")

    def taxa(self, records=False):
        """Ctx.taxa for the last classify(), in input order"""
        p = C.POINTER(DsbReadTaxon)()
        rc = lib().dsb_multi_taxa(self.h, C.byref(p))
        if rc != 0:
            raise DsbError(rc, "dsb_multi_taxa")
        return _taxa(p, getattr(self, "n_last", 0), records)


def _taxa(p, n, records):
    arr = (DsbReadTaxon * n)()
    if n:
        C.memmove(arr, p, n * C.sizeof(DsbReadTaxon))
    if records:
        return arr
    import numpy as np
    return np.array([arr[i].taxid for i in range(n)], dtype=np.uint32)


COVERAGE_DTYPE = [(f, "<u8") for f in COVERAGE_FIELDS]


def _coverage(fn, h, n_ref, what):
    import numpy as np
    out = np.zeros(n_ref, dtype=COVERAGE_DTYPE)
    rc = fn(h, out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise DsbError(rc, what)
    return out


WINDOW_DTYPE = [(f, "<u8") for f in WINDOW_FIELDS]


def _coverage_windows(fn, h, what):
    import numpy as np
    n = C.c_size_t(0)
    rc = fn(h, None, 0, C.byref(n))
    if rc != 0:
        raise DsbError(rc, what)
    out = np.zeros(n.value, dtype=WINDOW_DTYPE)
    rc = fn(h, out.ctypes.data_as(C.c_void_p), n.value, C.byref(n))
    if rc != 0:
        raise DsbError(rc, what)
    return out


def n_coverage_windows(index, window):
    """dsb_coverage_n_windows: the number of windows of `window` bases over all references (0 for window 0)"""
    return int(lib().dsb_coverage_n_windows(index.h, int(window)))


def _permille(min_frac):
    f = float(min_frac)
    if not (0.0 < f <= 1.0) or int(f * 1000 + 0.5) < 1:
        raise ValueError("min_frac must lie in (0, 1] (steps of 0.001): %r" % (min_frac,))
    return int(f * 1000 + 0.5)


SUMMARY_FIELDS = ("reads", "classified", "classes", "iterations", "converged", "max_change", "min_permille")


def _abundance(fn, h, n_ref, max_iter, tol, what):
    import numpy as np
    out = np.zeros(n_ref, dtype=ABUNDANCE_DTYPE)
    s = DsbAbundanceSummary()
    o = DsbEmOpts(int(max_iter), 0, float(tol))
    rc = fn(h, C.byref(o), out.ctypes.data_as(C.c_void_p), C.byref(s))
    if rc != 0:
        raise DsbError(rc, what)
    return out, {f: getattr(s, f) for f in SUMMARY_FIELDS}


def _abundance_assign(fn, h, n_ref, max_iter, tol, what):
    import numpy as np
    out = np.zeros(n_ref, dtype=ABUNDANCE_DTYPE)
    s = DsbAbundanceSummary()
    o = DsbEmOpts(int(max_iter), 0, float(tol))
    n = C.c_size_t(0)
    rc = fn(h, C.byref(o), None, None, None, 0, C.byref(n))        # (count)
    if rc != 0:
        raise DsbError(rc, what)
    recs = np.zeros(n.value, dtype=ASSIGN_DTYPE)
    rc = fn(h, C.byref(o), out.ctypes.data_as(C.c_void_p), C.byref(s), recs.ctypes.data_as(C.c_void_p), max(n.value, 1), C.byref(n))
    if rc != 0:
        raise DsbError(rc, what)
    return out, {f: getattr(s, f) for f in SUMMARY_FIELDS}, recs


def format_assign(index, reads, records):
    """dsb_format_assign over the reads of a run: one line (bytes) per read of make_reads()'s array and abundance_assign()'s records"""
    import numpy as np
    records = np.ascontiguousarray(records, dtype=ASSIGN_DTYPE)
    if len(records) != len(reads):
        raise ValueError("format_assign: %d records for %d reads" % (len(records), len(reads)))
    out = []
    for i in range(len(reads)):
        cap = 512
        while True:
            buf = C.create_string_buffer(cap)
            n = lib().dsb_format_assign(index.h, C.byref(reads[i]), records[i:i + 1].ctypes.data_as(C.c_void_p), buf, cap)
            if n >= 0:
                out.append(buf.raw[:n]); break
            if records[i]["ref_ID"] != DSB_ASSIGN_NONE and records[i]["ref_ID"] >= index.n_ref:
                raise ValueError("format_assign: record %d names reference %d of %d" % (i, records[i]["ref_ID"], index.n_ref))
            cap *= 4
    return b"".join(out)


def format_abundance(index, ab, summary):
    """dsb_abundance_format: the abundance table (bytes) of Ctx/Multi.abundance()'s array and summary dict"""
    import numpy as np
    ab = np.ascontiguousarray(ab, dtype=ABUNDANCE_DTYPE)
    if len(ab) != index.n_ref:
        raise ValueError("format_abundance: %d rows for %d references" % (len(ab), index.n_ref))
    s = DsbAbundanceSummary(**{f: summary[f] for f in SUMMARY_FIELDS})
    cap = 1 << 16
    while True:
        buf = C.create_string_buffer(cap)
        n = lib().dsb_abundance_format(index.h, ab.ctypes.data_as(C.c_void_p), C.byref(s), buf, cap)
        if n >= 0:
            return buf.raw[:n]
        cap *= 4


def format_coverage_windows(index, cov, win, window):
    """dsb_coverage_windows_format: the per-window table (bytes) of a coverage array and a window array of size `window`"""
    import numpy as np
    cov = np.ascontiguousarray(cov, dtype=COVERAGE_DTYPE)
    win = np.ascontiguousarray(win, dtype=WINDOW_DTYPE)
    if len(cov) != index.n_ref or int(window) < 1 or len(win) != n_coverage_windows(index, window):
        raise ValueError("format_coverage_windows: %d rows, %d windows of %d bases for %d references" % (len(cov), len(win), int(window), index.n_ref))
    cap = 1 << 16
    while True:
        buf = C.create_string_buffer(cap)
        n = lib().dsb_coverage_windows_format(index.h, cov.ctypes.data_as(C.c_void_p), win.ctypes.data_as(C.c_void_p), int(window), buf, cap)
        if n >= 0:
            return buf.raw[:n]
        cap *= 4


def format_coverage(index, cov):
    """dsb_coverage_format: the `samtools coverage`-style table (bytes) of a coverage array (Ctx/Multi.coverage())"""
    import numpy as np
    cov = np.ascontiguousarray(cov, dtype=COVERAGE_DTYPE)
    if len(cov) != index.n_ref:
        raise ValueError("format_coverage: %d rows for %d references" % (len(cov), index.n_ref))
    cap = 1 << 16
    while True:
        buf = C.create_string_buffer(cap)
        n = lib().dsb_coverage_format(index.h, cov.ctypes.data_as(C.c_void_p), buf, cap)
        if n >= 0:
            return buf.raw[:n]
        cap *= 4


def _lca(p, n):
    import numpy as np
    out = np.zeros(n, dtype=LCA_DTYPE)
    if n:
        C.memmove(out.ctypes.data, p, n * C.sizeof(DsbReadLca))
    return out


def _lca_counts(fn, h, what):
    import numpy as np
    n, s = C.c_size_t(0), DsbLcaSummary()
    rc = fn(h, None, 0, C.byref(n), C.byref(s))
    if rc != 0:
        raise DsbError(rc, what)
    out = np.zeros(n.value, dtype=TAXON_COUNT_DTYPE)
    if n.value:
        rc = fn(h, out.ctypes.data_as(C.c_void_p), n.value, C.byref(n), C.byref(s))
        if rc != 0:
            raise DsbError(rc, what)
    return out, {f: getattr(s, f) for f in LCA_SUMMARY_FIELDS}


def _hit_identity(p, n):
    import numpy as np
    out = np.zeros(n, dtype=HIT_IDENTITY_DTYPE)
    if n:
        C.memmove(out.ctypes.data, p, n * C.sizeof(DsbHitIdentity))
    return out


def _ref_identity(fn, h, n_ref, what):
    import numpy as np
    out = np.zeros(n_ref, dtype=REF_IDENTITY_DTYPE)
    rc = fn(h, out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise DsbError(rc, what)
    return out


def _alignment(fn, h, n_hits, what):
    import numpy as np
    pr = C.POINTER(DsbHitAlignment)(); po = C.POINTER(C.c_uint32)(); n = C.c_uint64(0)
    rc = fn(h, C.byref(pr), C.byref(po), C.byref(n))
    if rc != 0:
        raise DsbError(rc, what)
    recs = np.zeros(n_hits, dtype=HIT_ALIGNMENT_DTYPE); ops = np.zeros(n.value, dtype=np.uint32)
    if n_hits:
        C.memmove(recs.ctypes.data, pr, n_hits * C.sizeof(DsbHitAlignment))
    if n.value:
        C.memmove(ops.ctypes.data, po, n.value * 4)
    return recs, ops


def aln_plan(n, m, band=DSB_IDENT_BAND_DEFAULT, max_permille=DSB_IDENT_PERMILLE_DEFAULT, trace_kib=DSB_ALN_TRACE_KIB_DEFAULT):
    """dsb_aln_plan: the plan of an n x m pair in checkpoint mode, (K, n_ckpt), or None where it has none"""
    K, n_ck = C.c_uint32(0), C.c_uint32(0)
    rc = lib().dsb_aln_plan(int(n), int(m), int(band), int(max_permille), int(trace_kib), C.byref(K), C.byref(n_ck))
    if rc < 0:
        raise DsbError(rc, "dsb_aln_plan")
    return (K.value, n_ck.value) if rc else None


def aligned_sam_header(index):
    """dsb_aligned_sam_header: @HD, one @SQ per reference, @PG (bytes)"""
    cap = 1 << 16
    while True:
        buf = C.create_string_buffer(cap)
        n = lib().dsb_aligned_sam_header(index.h, buf, cap)
        if n >= 0:
            return buf.raw[:n]
        cap *= 4


def format_aligned_sam(index, reads, res, ident, aln, ops):
    """dsb_format_aligned_sam over a batch: the SAM lines (bytes) of make_reads()'s array, its result, Ctx/Multi.identity()'s records
    and Ctx/Multi.alignment()'s records and operations"""
    import numpy as np
    ident = np.ascontiguousarray(ident, dtype=HIT_IDENTITY_DTYPE); aln = np.ascontiguousarray(aln, dtype=HIT_ALIGNMENT_DTYPE)
    ops = np.ascontiguousarray(ops, dtype=np.uint32)
    if len(ident) != res.n_hits or len(aln) != res.n_hits:
        raise ValueError("format_aligned_sam: %d and %d records for %d hits" % (len(ident), len(aln), res.n_hits))
    if len(aln) and int((aln["ops_off"] + aln["n_ops"])[aln["n_ops"] > 0].max(initial=0)) > len(ops):
        raise ValueError("format_aligned_sam: a record reaches beyond the operations")
    out = []
    for i in range(len(reads)):
        rr = res.reads[i]
        hits = C.byref(res.hits.contents, rr.first * C.sizeof(DsbHit)) if rr.n else None
        idp = ident[rr.first:rr.first + rr.n].ctypes.data_as(C.c_void_p) if rr.n else None
        alp = aln[rr.first:rr.first + rr.n].ctypes.data_as(C.c_void_p) if rr.n else None
        cap = 1024 + (2 * reads[i].len + len(reads[i].name) + 256) * (rr.n + 1) + 12 * int(aln["n_ops"][rr.first:rr.first + rr.n].sum())
        while True:
            buf = C.create_string_buffer(cap)
            n = lib().dsb_format_aligned_sam(index.h, C.byref(reads[i]), C.byref(rr), hits, idp, alp, ops.ctypes.data_as(C.c_void_p), buf, cap)
            if n >= 0:
                out.append(buf.raw[:n]); break
            if cap > (1 << 28):
                raise DsbError(DSB_EINVAL, "dsb_format_aligned_sam")
            cap *= 4
    return b"".join(out)


def format_identity(index, reads, res, ident):
    """dsb_format_identity over a batch: the per-record lines (bytes) of make_reads()'s array, its result and Ctx/Multi.identity()'s records"""
    import numpy as np
    ident = np.ascontiguousarray(ident, dtype=HIT_IDENTITY_DTYPE)
    if len(ident) != res.n_hits:
        raise ValueError("format_identity: %d records for %d hits" % (len(ident), res.n_hits))
    out = []
    for i in range(len(reads)):
        rr = res.reads[i]
        hits = C.byref(res.hits.contents, rr.first * C.sizeof(DsbHit)) if rr.n else None
        idp = ident[rr.first:rr.first + rr.n].ctypes.data_as(C.c_void_p) if rr.n else None
        cap = 512 + 256 * rr.n + len(reads[i].name) * (rr.n + 1)
        while True:
            buf = C.create_string_buffer(cap)
            n = lib().dsb_format_identity(index.h, C.byref(reads[i]), C.byref(rr), hits, idp, buf, cap)
            if n >= 0:
                out.append(buf.raw[:n]); break
            if cap > (1 << 26):
                raise DsbError(DSB_EINVAL, "dsb_format_identity")
            cap *= 4
    return b"".join(out)


def format_ref_identity(index, tab):
    """dsb_identity_format: the per-reference identity table (bytes) of Ctx/Multi.ref_identity()'s array"""
    import numpy as np
    tab = np.ascontiguousarray(tab, dtype=REF_IDENTITY_DTYPE)
    if len(tab) != index.n_ref:
        raise ValueError("format_ref_identity: %d rows for %d references" % (len(tab), index.n_ref))
    cap = 1 << 16
    while True:
        buf = C.create_string_buffer(cap)
        n = lib().dsb_identity_format(index.h, tab.ctypes.data_as(C.c_void_p), buf, cap)
        if n >= 0:
            return buf.raw[:n]
        cap *= 4


def format_kraken(reads, lca):
    """dsb_format_kraken over a batch: Kraken's per-read lines (bytes) of make_reads()'s array and Ctx/Multi.lca()'s records"""
    import numpy as np
    lca = np.ascontiguousarray(lca, dtype=LCA_DTYPE)
    if len(lca) != len(reads):
        raise ValueError("format_kraken: %d records for %d reads" % (len(lca), len(reads)))
    out = []
    for i in range(len(reads)):
        cap = 256
        while True:
            buf = C.create_string_buffer(cap)
            n = lib().dsb_format_kraken(C.byref(reads[i]), lca[i:i + 1].ctypes.data_as(C.c_void_p), buf, cap)
            if n >= 0:
                out.append(buf.raw[:n]); break
            cap *= 4
    return b"".join(out)


def format_lca_report(taxonomy, rows, summary, names=None):
    """dsb_lca_report_format: Kraken's report (bytes) of Ctx/Multi.lca_counts()'s rows and summary dict; names: a TaxNames or None"""
    import numpy as np
    rows = np.ascontiguousarray(rows, dtype=TAXON_COUNT_DTYPE)
    s = DsbLcaSummary(**{f: summary[f] for f in LCA_SUMMARY_FIELDS})
    cap = 1 << 16
    while True:
        buf = C.create_string_buffer(cap)
        n = lib().dsb_lca_report_format(taxonomy.h, names.h if names is not None else None, rows.ctypes.data_as(C.c_void_p), len(rows), C.byref(s), buf, cap)
        if n >= 0:
            return buf.raw[:n]
        cap *= 4


class TaxNames:
    """names.dmp: the "scientific name" of each taxid (for format_lca_report); DsbError DSB_EIO on a file that cannot be read"""

    def __init__(self, path):
        self.h = C.c_void_p()
        rc = lib().dsb_taxnames_load(os.fsencode(path), C.byref(self.h))
        if rc != 0:
            raise DsbError(rc, "dsb_taxnames_load(%s)" % path)
        self.path = path

    def close(self):
        if self.h:
            lib().dsb_taxnames_close(self.h); self.h = C.c_void_p()


class Taxonomy:
    """nodes.dmp as `deSAMBA analysis` reads it (max_tid = last line's taxid + 1 000 000); DsbError on a parent cycle
    (DSB_EINVAL) or a file that cannot be read (DSB_EIO)."""

    def __init__(self, path):
        self.h = C.c_void_p()
        rc = lib().dsb_taxonomy_load(os.fsencode(path), C.byref(self.h))
        if rc != 0:
            raise DsbError(rc, "dsb_taxonomy_load(%s)" % path)
        self.path = path

    def close(self):
        if self.h:
            lib().dsb_taxonomy_close(self.h); self.h = C.c_void_p()

    @property
    def max_tid(self):
        return int(lib().dsb_taxonomy_max_tid(self.h))

    def parent(self, taxid):
        return int(lib().dsb_taxonomy_parent(self.h, taxid))


class Report:
    """the abundance report of `analysis ana_meta[_base]`, fed batch by batch in input order"""

    def __init__(self, taxonomy):
        self.taxonomy = taxonomy
        self.h = C.c_void_p()
        rc = lib().dsb_report_create(taxonomy.h, C.byref(self.h))
        if rc != 0:
            raise DsbError(rc, "dsb_report_create")

    def close(self):
        if self.h:
            lib().dsb_report_destroy(self.h); self.h = C.c_void_p()

    def add(self, index, reads, res, taxa=None, max_sec_N=5):
        """reads / res of one batch; taxa: Ctx.taxa(records=True) of it, or None (every read walked on the host)"""
        rc = lib().dsb_report_add(self.h, index.h, reads, C.byref(res), taxa, len(reads), max_sec_N)
        if rc != 0:
            raise DsbError(rc, "dsb_report_add")

    def add_sam(self, text):
        rc = lib().dsb_report_add_sam(self.h, text, len(text))
        if rc != 0:
            raise DsbError(rc, "dsb_report_add_sam")

    def text(self, by_base=False):
        cap = 1 << 16
        while True:
            buf = C.create_string_buffer(cap)
            n = lib().dsb_report_format(self.h, 1 if by_base else 0, buf, cap)
            if n >= 0:
                return buf.raw[:n]
            cap *= 4


def shard_plan(lengths, world, chunk_bases=0, chunk_reads=0):
    """dsb_shard_plan -> list of (start, end, hist_max_before, rank)"""
    n = len(lengths)
    arr = (C.c_uint32 * max(n, 1))(*lengths)
    cnt = C.c_size_t()
    lib().dsb_shard_plan(arr, n, world, chunk_bases, chunk_reads, None, 0, C.byref(cnt))
    out = (DsbChunk * max(cnt.value, 1))()
    rc = lib().dsb_shard_plan(arr, n, world, chunk_bases, chunk_reads, out, cnt.value, C.byref(cnt))
    if rc != 0:
        raise DsbError(rc, "dsb_shard_plan")
    return [(out[i].start, out[i].end, out[i].hist_max_before, out[i].rank) for i in range(cnt.value)]


def read_fastq(path, limit=None):
    """Plain-text FASTQ/FASTA reader with the record rules of the reference's kseq_read (src/lib/utils.c:939-977; the
    OLD kseq: '\\r' stays in sequence and quality, the first character of a sequence line is data even if it is '\\n',
    quality is read in whole lines).  Returns (name, seq, qual) tuples; records with a quality string of the wrong
    length are dropped as read_reads (src/cly_mt.c:42-56) drops them."""
    with open(path, "rb") as f:
        data = f.read()
    return parse_fastq(data, limit)


def parse_fastq(data, limit=None):
    recs = []
    n = len(data)
    p = 0
    last = 0
    space = b" \t\n\v\f\r"
    while True:
        if last == 0:
            a, b = data.find(b">", p), data.find(b"@", p)
            if a < 0 and b < 0:
                break
            p = min(x for x in (a, b) if x >= 0) + 1
        q = p
        while q < n and data[q] not in space:
            q += 1
        if q >= n and q == p:
            break
        name = data[p:q]
        if q < n and data[q:q + 1] != b"\n":
            e = data.find(b"\n", q)
            q = n if e < 0 else e
        p = min(q + 1, n) if q < n else n
        seq = []
        c = -1
        while True:
            if p >= n:
                c = -1
                break
            c = data[p]
            if c in b">+@":
                p += 1
                break
            e = data.find(b"\n", p + 1)
            e = n if e < 0 else e
            seq.append(data[p:e])
            p = min(e + 1, n)
        seq = b"".join(seq)
        last = c if c in (ord(">"), ord("@")) else 0
        qual = None
        bad = False
        if c == ord("+"):
            e = data.find(b"\n", p)
            if e < 0:
                break
            p = e + 1
            ql = []
            tot = 0
            while True:
                if p >= n:
                    break
                e = data.find(b"\n", p)
                e = n if e < 0 else e
                ql.append(data[p:e]); tot += e - p
                p = min(e + 1, n)
                if tot >= len(seq):
                    break
            qual = b"".join(ql)
            last = 0
            bad = len(qual) != len(seq)
        if not bad:
            recs.append((name, seq, qual))
            if limit and len(recs) >= limit:
                break
    return recs
