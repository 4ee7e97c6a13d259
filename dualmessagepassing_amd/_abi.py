"""The declarations of the C ABI (include/dmp_hip.h) as ctypes: the structs, the limits and the signature table.

This is the only module that knows a layout of the header; ``_lib`` binds the loaded library with ``SIGNATURES`` and the
launch wrappers fill the struct classes.  Written out by hand, not generated: tests/test_lib_abi.py parses the header
and compares every return type, argument list, struct field and limit below with it.
"""
import ctypes

c_int = ctypes.c_int
c_i32 = ctypes.c_int32
c_i64 = ctypes.c_int64
c_u64 = ctypes.c_uint64
c_f32 = ctypes.c_float
c_double = ctypes.c_double
c_ptr = ctypes.c_void_p
c_size = ctypes.c_size_t

ABI_VERSION = 97

# ---- limits of the header that the host side relies on (``#define``s of the same names)
DMP_COLLATE_MAX_JOBS = 4
DMP_POOL_MAX_JOBS = 4
DMP_REDUCE_MAX_SEGMENTS = 16
DMP_ADAMW_MAX_SKIP = 16
DMP_ADAMW_MAX_SEGMENTS = 1024
DMP_LOOKUP_MAX_JOBS = 8
DMP_CONCAT_MAX_JOBS = 12
DMP_GEMM_MAX_JOBS = 12
DMP_GEMM_MAX_TERMS = 3
DMP_ATB_MAX_JOBS = 8
DMP_MEM_MEAN, DMP_MEM_SUM, DMP_MEM_MAX = 0, 1, 2      # the pooling modes of dmp_mem_init_fwd / _bwd
DMP_LRP_MAX_NEIGHBOURS = 32                            # distinct out-neighbours of a node the permutation index admits
DMP_LRP_MAX_SEQ_LEN = 6
DMP_LRP_OVER_CAP, DMP_LRP_SELF_LOOP, DMP_LRP_DROPPED = 1, 2, 4      # bits of the status word of dmp_lrp_count / _fill
DMP_RANK_BAD_TYPE = 1                                  # status word of dmp_rank_counts_typed: a type code above 62 was met
DMP_RESIDENT_MAX_SLOTS = 4096                          # pairs (real + inert) of a batch dmp_collate_resident assembles
DMP_SUBISO_MAX_PN, DMP_SUBISO_MAX_PM = 16, 64          # the pairs dmp_subiso_label_dev admits: pattern nodes / edges,
DMP_SUBISO_MAX_GN, DMP_SUBISO_MAX_GM = 512, 2048       # graph nodes / distinct (src, dst, label) graph edges
DMP_SUBISO_MAX_BUDGET = 16777216                       # the largest trial budget of one of its work items
DMP_SUBISO_DESC_WORDS = 8                              # int32 words of a pair's row in dmp_subiso_image.desc


# ---- the structs, named and ordered as in the header; pointers are c_void_p (assigned from ``data_ptr()`` / None)
class dmp_collate_job(ctypes.Structure):
    _fields_ = [("local_src", c_ptr), ("local_dst", c_ptr), ("num_nodes", c_ptr), ("num_edges", c_ptr), ("B", c_i64), ("N", c_i64),
                ("E", c_i64), ("node_off", c_ptr), ("edge_off", c_ptr), ("src", c_ptr), ("dst", c_ptr), ("edge_graph", c_ptr),
                ("node_graph", c_ptr)]


class dmp_pool_job(ctypes.Structure):
    _fields_ = [("sizes_a", c_ptr), ("sizes_b", c_ptr), ("Ba", c_i64), ("Bb", c_i64), ("flag_a", c_ptr), ("flag_b", c_ptr),
                ("rows_a", c_i64), ("R", c_i64), ("chunk", c_int), ("off", c_ptr), ("gptr", c_ptr), ("vptr", c_ptr), ("vent", c_ptr),
                ("gent", c_ptr), ("seg", c_ptr), ("flag8", c_ptr), ("rowmap", c_ptr), ("sizes", c_ptr)]


class dmp_smallk_job(ctypes.Structure):
    _fields_ = [("X", c_ptr), ("ldx", c_i64), ("D", c_ptr), ("ldd", c_i64), ("gate", c_ptr), ("rowmask", c_ptr), ("R", c_i64),
                ("partial", c_ptr)]


class dmp_l0_pack_job(ctypes.Structure):
    _fields_ = [("enc_p", c_ptr), ("ldp", c_i64), ("rows_p", c_i64), ("enc_g", c_ptr), ("ldg", c_i64), ("gate", c_ptr), ("rows_g", c_i64),
                ("K", c_int), ("Kpad", c_int), ("goff", c_int), ("out", c_ptr)]


class dmp_kept_job(ctypes.Structure):
    _fields_ = [("mask", c_ptr), ("R", c_i64), ("tiles", c_int), ("scratch", c_ptr), ("list", c_ptr), ("count", c_ptr)]


class dmp_rowmask_job(ctypes.Structure):
    _fields_ = [("gate", c_ptr), ("R", c_i64), ("mask", c_ptr)]


class dmp_filter_job(ctypes.Structure):
    _fields_ = [("p_seg", c_ptr), ("p_label", c_ptr), ("num_p", c_i64), ("p_sizes", c_ptr), ("p_max", c_i64), ("g_seg", c_ptr),
                ("g_label", c_ptr), ("num_g", c_i64), ("num_labels", c_i64), ("present_off", c_i64), ("gate", c_ptr), ("seg_is_i32", c_i64)]


class dmp_mask_job(ctypes.Structure):
    _fields_ = [("sizes", c_ptr), ("off", c_ptr), ("max_len", c_i64), ("rev", c_ptr), ("mask", c_ptr), ("count", c_ptr)]


class dmp_lookup_job(ctypes.Structure):
    _fields_ = [("table", c_ptr), ("ld", c_i64), ("table_rows", c_i64), ("width", c_int), ("idx", c_ptr), ("rows", c_i64), ("out", c_ptr)]


class dmp_concat_job(ctypes.Structure):
    _fields_ = [("a", c_ptr), ("na", c_i64), ("b", c_ptr), ("nb", c_i64), ("out", c_ptr), ("elem_size", c_int), ("add_b", c_i64),
                ("fill_a", c_f32)]


class dmp_layer_weights(ctypes.Structure):
    _fields_ = [("nloop_w", c_ptr), ("in_w", c_ptr), ("out_w", c_ptr), ("nbias", c_ptr), ("eloop_w", c_ptr), ("src_w", c_ptr),
                ("dst_w", c_ptr), ("ebias", c_ptr), ("nW0", c_ptr), ("nb0", c_ptr), ("eW0", c_ptr), ("eb0", c_ptr), ("nW2", c_ptr),
                ("eW2", c_ptr), ("eye", c_ptr)]


class dmp_layer_folded(ctypes.Structure):
    _fields_ = [("Bn", c_ptr), ("bn", c_ptr), ("Wx", c_ptr), ("Wes", c_ptr), ("be", c_ptr), ("WesT", c_ptr), ("nW2t", c_ptr),
                ("eW2t", c_ptr)]


class dmp_layer_folded_grads(ctypes.Structure):
    _fields_ = [("dBn", c_ptr), ("dbn", c_ptr), ("dWx", c_ptr), ("dWes", c_ptr), ("dbe", c_ptr)]


class dmp_layer_weight_grads(ctypes.Structure):
    _fields_ = [("nloop_w", c_ptr), ("in_w", c_ptr), ("out_w", c_ptr), ("nbias", c_ptr), ("eloop_w", c_ptr), ("src_w", c_ptr),
                ("dst_w", c_ptr), ("ebias", c_ptr), ("nW0", c_ptr), ("eW0", c_ptr)]


class dmp_gemm_term(ctypes.Structure):
    _fields_ = [("A", c_ptr), ("lda", c_i64), ("B", c_ptr), ("ldb", c_i64), ("transA", c_i32), ("transB", c_i32), ("K", c_i32),
                ("pad", c_i32)]


class dmp_gemm_job(ctypes.Structure):
    _fields_ = [("term", dmp_gemm_term * DMP_GEMM_MAX_TERMS), ("C0", c_ptr), ("ldc0", c_i64), ("C", c_ptr), ("ldc", c_i64),
                ("num_terms", c_i32), ("M", c_i32), ("N", c_i32), ("pad", c_i32)]


class dmp_head_weights(ctypes.Structure):
    _fields_ = [("Wp", c_ptr), ("bp", c_ptr), ("Wg", c_ptr), ("bg", c_ptr), ("W1", c_ptr), ("b1", c_ptr), ("W2", c_ptr), ("b2", c_ptr)]


class dmp_head_io(ctypes.Structure):
    _fields_ = [("ps", c_ptr), ("ld_ps", c_i64), ("gs", c_ptr), ("ld_gs", c_i64), ("pl", c_ptr), ("gl", c_ptr), ("scale_p", c_f32),
                ("scale_g", c_f32), ("F", c_ptr), ("Y1S", c_ptr), ("y", c_ptr)]


class dmp_head_grads(ctypes.Structure):
    _fields_ = [("dy", c_ptr), ("dy_scale", c_ptr), ("dY1", c_ptr), ("dP", c_ptr), ("dG", c_ptr), ("dps", c_ptr), ("ld_dps", c_i64),
                ("dgs", c_ptr), ("ld_dgs", c_i64), ("dWp", c_ptr), ("dbp", c_ptr), ("dWg", c_ptr), ("dbg", c_ptr), ("dW1", c_ptr),
                ("db1", c_ptr), ("dW2", c_ptr), ("db2", c_ptr)]


class dmp_typed_job(ctypes.Structure):
    _fields_ = [("Hin", c_ptr), ("ldh", c_i64), ("W2", c_ptr), ("ldw", c_i64), ("w_in_out", c_int), ("bias", c_ptr), ("R", c_ptr),
                ("ldr", c_i64), ("R2", c_ptr), ("ldr2", c_i64), ("act", c_int), ("slope", c_f32), ("out", c_ptr), ("ldo", c_i64)]


class dmp_chain_panel(ctypes.Structure):
    _fields_ = [("W", c_ptr), ("ld", c_i64), ("transposed", c_int)]


class dmp_atb2_job(ctypes.Structure):
    _fields_ = [("Z", c_ptr), ("ldz", c_i64), ("D", c_ptr), ("ldd", c_i64), ("partial_T", c_ptr), ("partial_B", c_ptr),
                ("partial_stride", c_i64), ("ldp", c_int)]


class dmp_atb_job(ctypes.Structure):
    _fields_ = [("A", c_ptr), ("lda", c_i64), ("B", c_ptr), ("ldb", c_i64), ("gate", c_ptr), ("partial", c_ptr), ("partial_stride", c_i64),
                ("ldp", c_int), ("partial_colsum", c_ptr), ("cs_ld", c_int), ("rowmask", c_ptr)]


class dmp_resident_side(ctypes.Structure):
    _fields_ = [("src", c_ptr), ("dst", c_ptr), ("vlabel", c_ptr), ("elabel", c_ptr), ("eid", c_ptr), ("rev", c_ptr), ("node_ptr", c_ptr),
                ("edge_ptr", c_ptr)]


class dmp_resident_batch(ctypes.Structure):
    _fields_ = [("src", c_ptr), ("dst", c_ptr), ("num_nodes", c_ptr), ("num_edges", c_ptr), ("nid", c_ptr), ("vlabel", c_ptr), ("eid", c_ptr),
                ("elabel", c_ptr), ("rev", c_ptr)]


class dmp_subiso_image(ctypes.Structure):
    _fields_ = [("desc", c_ptr), ("p_cbeg", c_ptr), ("p_cend", c_ptr), ("p_tend", c_ptr), ("p_ends", c_ptr), ("p_elab", c_ptr),
                ("g_rowptr", c_ptr), ("g_ent", c_ptr), ("g_cand", c_ptr), ("g_inv", c_ptr), ("chunk_pair", c_ptr), ("chunk_root", c_ptr),
                ("num_pairs", c_i64), ("total_pn", c_i64), ("total_pm", c_i64), ("total_gn", c_i64), ("total_gm", c_i64),
                ("total_um", c_i64), ("num_chunks", c_i64), ("max_gn", c_int), ("max_um", c_int)]


_p = ctypes.POINTER      # ``const dmp_X *``: takes an array ``(dmp_X * n)()``, ``byref(x)`` or None, nothing else


# name -> (restype, argtypes), one entry per function of the header
SIGNATURES = {
    "dmp_abi_version": (c_int, []),
    "dmp_last_hip_error": (ctypes.c_char_p, []),
    "dmp_csr_workspace_words": (c_size, [c_i64, c_i64]),
    "dmp_csr_build": (c_int, [c_ptr, c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr]),
    "dmp_incidence_build": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_ptr]),
    "dmp_degree_coef": (c_int, [c_ptr, c_i64, c_ptr, c_ptr]),
    "dmp_collate": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_ptr, c_ptr, c_ptr, c_ptr,
                            c_ptr, c_ptr, c_ptr]),
    "dmp_add_reversed_edges": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_i64,
                                       c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr]),
    "dmp_line_graph_count": (c_int, [c_ptr, c_ptr, c_i64, c_ptr, c_ptr]),
    "dmp_line_graph_fill": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_ptr]),
    "dmp_first_edge_of_id": (c_int, [c_ptr, c_i64, c_i64, c_ptr, c_ptr]),
    "dmp_dedupe_table_words": (c_size, [c_i64]),
    "dmp_dedupe_first": (c_int, [c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_ptr, c_ptr]),
    "dmp_subiso_node_weights": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_ptr, c_i64, c_ptr, c_ptr]),
    "dmp_dual_subisomorphisms": (c_int, [c_ptr, c_i64, c_ptr, c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64,
                                         c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr]),
    "dmp_subiso_enumerate": (c_i64, [c_i64, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64,
                                     c_i64]),
    "dmp_subiso_count_batch": (c_int, [c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr,
                                       c_ptr, c_int]),
    "dmp_random_walks": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_u64, c_ptr, c_ptr, c_ptr]),
    "dmp_sample_in_edges": (c_int, [c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_u64, c_ptr, c_ptr]),
    "dmp_pattern_edge_active": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_ptr]),
    "dmp_subiso_edge_weights": (c_int, [c_ptr, c_i64, c_ptr, c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr,
                                        c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_ptr, c_ptr]),
    "dmp_class_tiles_workspace_words": (c_size, [c_i64, c_int]),
    "dmp_class_tiles": (c_int, [c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr]),
    "dmp_csr_keep_scratch_words": (c_i64, [c_i64]),
    "dmp_csr_keep": (c_int, [c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_ptr, c_ptr]),
    "dmp_class_tiles_gated": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr]),
    "dmp_scan_workspace_words": (c_size, [c_i64]),
    "dmp_exclusive_scan_i64": (c_int, [c_ptr, c_i64, c_ptr, c_ptr, c_ptr]),
    "dmp_seg_sum": (c_int, [c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_ptr, c_i64, c_int, c_ptr]),
    "dmp_seg_sum2": (c_int, [c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_f32, c_f32, c_ptr, c_i64,
                             c_int, c_ptr]),
    "dmp_small_gemm_jobs": (c_int, [_p(dmp_gemm_job), c_int, c_ptr]),
    "dmp_pool_index_jobs": (c_int, [_p(dmp_pool_job), c_int, c_ptr]),
    "dmp_collate_jobs": (c_int, [_p(dmp_collate_job), c_int, c_ptr]),
    "dmp_csr_build_graphs_max_nodes": (c_int, []),
    "dmp_csr_build_graphs": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr,
                                     c_ptr, c_ptr, c_ptr, c_ptr]),
    "dmp_pool_weight_sums": (c_int, [c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_ptr]),
    "dmp_gate_compact_hist_nodes": (c_int, []),
    "dmp_gate_compact": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_i64, c_int, c_ptr, c_ptr, c_ptr, c_ptr,
                                 c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr]),
    "dmp_out_degrees": (c_int, [c_ptr, c_i64, c_i64, c_ptr, c_ptr]),
    "dmp_seg_sum2_graphs_max_nodes": (c_int, []),
    "dmp_seg_sum2_graphs": (c_int, [c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_int, c_int, c_f32, c_f32,
                                    c_ptr, c_i64, c_ptr]),
    "dmp_seg_sum2_graphs_masked": (c_int, [c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_int, c_int, c_f32, c_f32,
                                           c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_i64, c_ptr]),
    "dmp_seg_sum2_rows": (c_int, [c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_int, c_i64, c_int, c_f32, c_f32, c_ptr, c_i64, c_ptr]),
    "dmp_incidence_keep": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_ptr]),
    "dmp_seg_sum2_tiled": (c_int, [c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_int, c_int, c_f32, c_f32,
                                   c_ptr, c_i64, c_ptr]),
    "dmp_gather_rows": (c_int, [c_ptr, c_i64, c_ptr, c_ptr, c_i64, c_int, c_ptr, c_i64, c_ptr]),
    "dmp_gather_select": (c_int, [c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_f32, c_f32,
                                  c_ptr, c_i64, c_ptr]),
    "dmp_colsum_partial_rows": (c_i64, [c_i64, c_int]),
    "dmp_gate_residual": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_i64, c_int, c_ptr, c_i64, c_ptr]),
    "dmp_scale_rows_colsum": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_int, c_ptr, c_i64, c_ptr, c_ptr]),
    "dmp_relu_bwd_colsum": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_i64, c_int, c_f32, c_ptr, c_i64, c_ptr, c_ptr]),
    "dmp_edge_combine_bwd_g_colsum": (c_int, [c_ptr, c_i64, c_ptr, c_ptr, c_i64, c_int, c_ptr, c_i64, c_ptr, c_ptr]),
    "dmp_colsum_partials": (c_int, [c_ptr, c_i64, c_i64, c_int, c_ptr, c_ptr]),
    "dmp_reduce_partials": (c_int, [c_ptr, c_i64, c_i64, c_ptr, c_int, c_ptr]),
    "dmp_add_bias_relu": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_i64, c_int, c_f32, c_ptr, c_i64, c_ptr]),
    "dmp_heads_forward": (c_int, [_p(dmp_head_weights), _p(dmp_head_io), c_int, c_int, c_int, c_f32, c_ptr]),
    "dmp_heads_backward": (c_int, [_p(dmp_head_weights), _p(dmp_head_io), _p(dmp_head_grads), c_int, c_int, c_int, c_f32, c_ptr]),
    "dmp_fold_layers": (c_int, [_p(dmp_layer_weights), _p(dmp_layer_folded), c_int, c_int, c_ptr]),
    "dmp_unfold_layers": (c_int, [_p(dmp_layer_weights), _p(dmp_layer_folded_grads), _p(dmp_layer_weight_grads), c_int, c_int, c_ptr]),
    "dmp_smallk_embed_gate": (c_int, [c_ptr, c_i64, c_int, c_ptr, c_i64, c_ptr, c_i64, c_int, c_ptr, c_i64, c_ptr]),
    "dmp_smallk_embed_live": (c_int, [c_ptr, c_i64, c_int, c_ptr, c_i64, c_ptr, c_i64, c_int, c_ptr, c_i64, c_ptr]),
    "dmp_smallk_atb_blocks": (c_i64, [c_i64]),
    "dmp_smallk_embed_cols": (c_int, [c_ptr, c_i64, c_int, c_ptr, c_i64, c_ptr, c_i64, c_int, c_int, c_ptr, c_i64, c_ptr]),
    "dmp_smallk_atb_cols_masked": (c_int, [c_ptr, c_i64, c_int, c_ptr, c_i64, c_int, c_ptr, c_i64, c_ptr, c_ptr, c_i64, c_int, c_ptr, c_ptr]),
    "dmp_smallk_atb_cols_rows": (c_int, [c_ptr, c_i64, c_int, c_ptr, c_i64, c_int, c_ptr, c_i64, c_ptr, c_ptr, c_i64, c_int, c_ptr, c_ptr]),
    "dmp_smallk_atb": (c_int, [c_ptr, c_i64, c_int, c_ptr, c_i64, c_ptr, c_i64, c_int, c_ptr, c_ptr]),
    "dmp_smallk_atb_jobs": (c_int, [_p(dmp_smallk_job), c_int, c_int, c_int, c_ptr]),
    "dmp_l0_pack_jobs": (c_int, [_p(dmp_l0_pack_job), c_int, c_ptr]),
    "dmp_count_loss": (c_int, [c_ptr, c_ptr, c_i64, c_int, c_f32, c_ptr, c_ptr, c_ptr]),
    "dmp_match_loss_workspace_words": (c_i64, [c_i64, c_i64]),
    "dmp_match_loss": (c_int, [c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr]),
    "dmp_reduce_partials_multi": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_ptr]),
    "dmp_l0_pack": (c_int, [c_ptr, c_i64, c_i64, c_ptr, c_i64, c_ptr, c_i64, c_int, c_int, c_int, c_ptr, c_ptr]),
    "dmp_l0_edge_fwd_masked": (c_int, [c_ptr, c_i64, c_int, c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int,
                                       c_f32, c_ptr, c_i64, c_ptr]),
    "dmp_l0_bwd_w_blocks": (c_i64, [c_i64]),
    "dmp_l0_node_pack_rows": (c_i64, []),
    "dmp_l0_node_fwd": (c_int, [c_ptr, c_i64, c_int, c_ptr, c_i64, c_int, c_int, c_ptr, c_i64, c_ptr, c_f32, c_ptr,
                                c_ptr, c_ptr, c_i64, c_i64, c_i64, c_i64, c_int, c_ptr, c_i64, c_ptr, c_i64, c_ptr]),
    "dmp_l0_node_fwd_mfma_max_codes": (c_int, []),
    "dmp_l0_node_fwd_mfma": (c_int, [c_ptr, c_i64, c_int, c_ptr, c_i64, c_int, c_int, c_ptr, c_i64, c_i64, c_int, c_i64, c_ptr, c_f32, c_ptr,
                                     c_ptr, c_ptr, c_i64, c_i64, c_i64, c_int, c_ptr, c_i64, c_ptr, c_i64, c_ptr]),
    "dmp_l0_node_codes_bwd_blocks": (c_i64, [c_i64]),
    "dmp_l0_node_codes_bwd": (c_int, [c_ptr, c_i64, c_int, c_int, c_ptr, c_i64, c_int, c_int, c_int, c_i64, c_ptr, c_i64, c_ptr, c_i64, c_ptr,
                                      c_ptr, c_i64, c_i64, c_i64, c_int, c_ptr, c_ptr, c_ptr]),
    "dmp_bn_partial_rows": (c_i64, [c_i64, c_int]),
    "dmp_bn_train_fwd": (c_int, [c_ptr, c_i64, c_i64, c_int, c_ptr, c_ptr, c_f32, c_f32, c_ptr, c_ptr, c_int, c_f32, c_ptr, c_ptr, c_ptr,
                                 c_i64, c_ptr]),
    "dmp_bn_train_bwd": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_i64, c_i64, c_int, c_ptr, c_int, c_f32, c_ptr, c_ptr, c_ptr, c_i64,
                                 c_ptr]),
    "dmp_bn_train_fwd_rows": (c_int, [c_ptr, c_i64, c_i64, c_ptr, c_int, c_ptr, c_ptr, c_f32, c_f32, c_ptr, c_ptr, c_int, c_f32, c_ptr, c_ptr,
                                      c_ptr, c_i64, c_ptr]),
    "dmp_bn_train_bwd_rows": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_i64, c_i64, c_ptr, c_int, c_ptr, c_int, c_f32, c_ptr, c_ptr, c_ptr,
                                      c_i64, c_ptr]),
    "dmp_l0_bwd_w_masked": (c_int, [c_ptr, c_i64, c_int, c_ptr, c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_i64, c_int, c_ptr, c_ptr]),
    "dmp_scalar_filter_gates": (c_int, [_p(dmp_filter_job), c_int, c_i64, c_ptr, c_i64, c_ptr]),
    "dmp_csr_pair_workspace_words": (c_size, [c_i64]),
    "dmp_csr_build_pair": (c_int, [c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr,
                                   c_ptr, c_ptr]),
    "dmp_heads_blend": (c_int, [c_ptr, c_ptr, c_ptr, c_int, c_int, c_ptr, c_ptr]),
    "dmp_pool_out": (c_int, [c_ptr, c_ptr, c_i64, c_int, c_ptr, c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_ptr, c_i64,
                             c_int, c_ptr, c_ptr, c_ptr, c_ptr]),
    "dmp_rows_gemm": (c_int, [c_ptr, c_i64, c_i64, c_int, c_ptr, c_int, c_ptr, c_i64, c_ptr]),
    "dmp_pool_wgrad_blocks": (c_i64, [c_i64]),
    "dmp_pool_wgrad": (c_int, [c_ptr, c_i64, c_i64, c_int, c_ptr, c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_int, c_ptr, c_ptr, c_ptr]),
    "dmp_concat_pairs": (c_int, [_p(dmp_concat_job), c_int, c_ptr]),
    "dmp_table_rows": (c_int, [_p(dmp_lookup_job), c_int, c_ptr]),
    "dmp_len_masks": (c_int, [_p(dmp_mask_job), c_int, c_i64, c_ptr]),
    "dmp_pack_segments": (c_int, [c_ptr, c_ptr, c_ptr, c_int, c_int, c_ptr, c_ptr]),
    "dmp_adamw_step": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_double, c_double, c_double, c_double,
                               c_double, c_i64, c_ptr]),
    "dmp_adamw_step_skip": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_double, c_double, c_double, c_double,
                                    c_double, c_i64, c_ptr, c_ptr, c_int, c_ptr]),
    "dmp_adamw_step_dev": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_double, c_double, c_double, c_double,
                                   c_ptr, c_ptr, c_int, c_ptr]),
    "dmp_adamw_step_segments": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_ptr, c_int, c_ptr, c_ptr, c_ptr, c_double, c_double,
                                        c_double, c_double, c_ptr, c_int, c_ptr]),
    "dmp_adamw_step_guarded": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_double, c_double, c_double, c_double,
                                       c_ptr, c_ptr, c_int, c_ptr, c_int, c_ptr]),
    "dmp_edge_select_build": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_ptr]),
    "dmp_edge_select_nodes": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_ptr]),
    "dmp_edge_fwd_fused": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_ptr, c_ptr,
                                   c_i64, c_int, c_f32, c_ptr, c_i64, c_ptr]),
    "dmp_edge_fwd_typed": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr,
                                   c_ptr, c_i64, c_i64, c_int, c_f32, c_ptr, c_i64, c_ptr]),
    "dmp_bwd_z_typed_arow": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_i64, c_i64, c_ptr, c_i64, c_ptr, c_ptr, c_f32,
                                     c_f32, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_int, c_ptr, c_i64, c_ptr, c_i64, c_ptr]),
    "dmp_mask_slots": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_ptr]),
    "dmp_pool_relu_bwd_blocks": (c_i64, [c_i64, c_int]),
    "dmp_pool_relu_bwd": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_f32, c_ptr, c_i64,
                                  c_ptr, c_ptr, c_ptr]),
    "dmp_relu_bwd_gathered_colsum": (c_int, [c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_f32, c_ptr, c_i64, c_ptr, c_ptr]),
    "dmp_dev_set_exact_fp32": (None, [c_int]),
    "dmp_dev_get_exact_fp32": (c_int, []),
    "dmp_rel_gemm": (c_int, [c_ptr, c_i64, c_i64, c_ptr, c_i64, c_int, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_i64,
                             c_int, c_ptr, c_i64, c_ptr]),
    "dmp_rel_atb_blocks": (c_i64, [c_int]),
    "dmp_rel_atb": (c_int, [c_ptr, c_i64, c_i64, c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_i64, c_int, c_ptr, c_ptr]),
    "dmp_atb_typed_blocks_h": (c_i64, [c_i64, c_int]),
    "dmp_atb_rows_blocks_h": (c_i64, [c_i64, c_int, c_int, c_int]),
    "dmp_atb_rows_plain": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_i64, c_int, c_int, c_int, c_ptr, c_ptr]),
    "dmp_atb_rows_masked": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_ptr, c_i64, c_int, c_int, c_int, c_ptr, c_ptr, c_ptr]),
    "dmp_atb_jobs_blocks_h": (c_i64, [c_i64, c_int, c_int]),
    "dmp_atb_rows_jobs_h": (c_int, [_p(dmp_atb_job), c_int, c_i64, c_int, c_ptr, c_ptr, c_ptr, c_i64, c_ptr]),
    "dmp_atb_tile_jobs_blocks": (c_i64, [c_i64, c_int, c_int]),
    "dmp_mfma_partial_rows_h": (c_i64, [c_i64, c_int]),
    "dmp_gemm_k64": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_int, c_ptr, c_i64, c_i64, c_ptr]),
    "dmp_atb_typed": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_ptr, c_ptr, c_ptr]),
    "dmp_out_fwd_fused_rows": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_int, c_ptr, c_i64, c_i64, c_int, c_int, c_ptr,
                                       c_i64, c_ptr]),
    "dmp_bwd_h1_fused_rows": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_int, c_i64, c_int, c_f32, c_ptr,
                                      c_i64, c_ptr, c_ptr, c_ptr]),
    "dmp_kept_rows_scratch_words": (c_i64, [c_i64]),
    "dmp_kept_rows": (c_int, [c_ptr, c_i64, c_int, c_ptr, c_ptr, c_ptr, c_ptr]),
    "dmp_l0_edge_fwd_rows": (c_int, [c_ptr, c_i64, c_int, c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int,
                                     c_f32, c_ptr, c_i64, c_ptr]),
    "dmp_l0_bwd_w_rows": (c_int, [c_ptr, c_i64, c_int, c_ptr, c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_ptr, c_i64, c_int, c_ptr, c_ptr]),
    "dmp_typed_partial_rows": (c_i64, [c_i64, c_int]),
    "dmp_out_fwd_typed": (c_int, [_p(dmp_typed_job), c_int, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_ptr]),
    "dmp_bwd_h1_typed": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_f32, c_ptr, c_i64,
                                 c_ptr, c_ptr, c_ptr]),
    "dmp_kept_rows_jobs": (c_int, [_p(dmp_kept_job), c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_ptr]),
    "dmp_row_mask_bits_jobs": (c_int, [_p(dmp_rowmask_job), c_int, c_ptr]),
    "dmp_atb2_blocks": (c_i64, [c_i64, c_int]),
    "dmp_atb2_jobs": (c_int, [_p(dmp_atb2_job), c_int, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_ptr]),
    "dmp_bwd_z_w": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_i64, c_i64, c_ptr, c_i64, c_ptr, c_ptr, c_f32, c_f32,
                            c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_ptr]),
    "dmp_out_fwd_typed_codes": (c_int, [_p(dmp_typed_job), c_ptr, c_i64, c_int, c_ptr, c_i64, c_i64, c_i64, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_ptr]),
    "dmp_bwd_h1_w_blocks": (c_i64, [c_i64]),
    "dmp_bwd_h1_w": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_ptr, c_i64, c_i64, c_int, c_f32, c_ptr, c_i64,
                             c_ptr, c_ptr, c_ptr, c_ptr]),
    "dmp_bwd_h1_w_max_codes": (c_int, []),
    "dmp_bwd_h1_w_codes": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_ptr, c_i64, c_i64, c_int, c_f32, c_ptr, c_i64,
                                   c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_ptr, c_i64, c_i64, c_int, c_ptr, c_ptr]),
    "dmp_node_chain_blocks": (c_i64, [c_i64]),
    "dmp_node_chain_panel_words": (c_i64, []),
    "dmp_node_chain_pack": (c_int, [_p(dmp_chain_panel), c_int, c_ptr, c_ptr]),
    "dmp_node_chain_fwd": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_int, c_f32, c_ptr, c_ptr, c_i64, c_i64, c_int,
                                   c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_i64, c_ptr]),
    "dmp_node_chain_bwd": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_int, c_f32, c_ptr, c_ptr, c_i64, c_i64, c_int,
                                   c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_ptr, c_ptr]),
    "dmp_edge_mlp_fwd": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_ptr, c_ptr, c_i64,
                                 c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_f32, c_ptr, c_i64, c_ptr, c_i64, c_ptr]),
    "dmp_l0_edge_mlp_max_codes": (c_int, []),
    "dmp_l0_edge_mlp_fwd": (c_int, [c_ptr, c_i64, c_int, c_ptr, c_i64, c_int, c_i64, c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_f32,
                                    c_ptr, c_i64, c_int, c_ptr, c_ptr, c_i64, c_i64, c_ptr, c_i64, c_i64, c_ptr, c_ptr, c_i64, c_i64, c_int,
                                    c_ptr, c_i64, c_ptr, c_i64, c_ptr]),
    "dmp_row_mask_bits": (c_int, [c_ptr, c_i64, c_ptr, c_ptr]),
    "dmp_row_mask_rows": (c_int, [c_ptr, c_i64, c_int, c_i64, c_ptr, c_ptr]),
    "dmp_bwd_z_fused": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_i64, c_i64, c_ptr, c_i64, c_ptr, c_ptr, c_ptr,
                                c_f32, c_f32, c_i64, c_int, c_ptr, c_i64, c_ptr]),
    "dmp_gemm_k128": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_int, c_ptr, c_i64, c_i64, c_int, c_ptr]),
    "dmp_edge_combine": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64,
                                 c_int, c_int, c_f32, c_ptr, c_i64, c_ptr]),
    "dmp_relu_bwd_g_colsum": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_ptr, c_i64, c_int, c_f32, c_ptr, c_i64,
                                      c_ptr, c_ptr]),
    "dmp_edge_combine_bwd_g": (c_int, [c_ptr, c_i64, c_ptr, c_ptr, c_i64, c_int, c_ptr, c_i64, c_ptr]),
    "dmp_compgcn_agg": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int,
                                c_ptr, c_i64, c_ptr]),
    "dmp_compgcn_agg_bwd": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_ptr, c_ptr, c_ptr,
                                    c_i64, c_int, c_int, c_ptr, c_i64, c_ptr, c_i64, c_ptr]),
    "dmp_attn_supported_dh": (c_int, [c_int]),
    "dmp_attn_fwd": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_int, c_int, c_f32, c_ptr, c_ptr, c_ptr, c_ptr]),
    "dmp_attn_bwd": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_int, c_int, c_f32, c_ptr,
                             c_ptr, c_ptr, c_ptr, c_ptr]),
    "dmp_mem_init_fwd": (c_int, [c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_i64, c_i64, c_int, c_int, c_int, c_int, c_int, c_ptr, c_ptr,
                                 c_ptr, c_ptr, c_ptr, c_ptr, c_ptr]),
    "dmp_mem_init_bwd": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_int, c_int, c_int, c_ptr, c_ptr, c_ptr]),
    "dmp_cnn_fwd": (c_int, [c_ptr, c_i64, c_i64, c_int, c_ptr, c_ptr, c_int, c_int, c_int, c_int, c_int, c_f32, c_ptr, c_int, c_ptr,
                            c_ptr, c_ptr, c_ptr, c_ptr]),
    "dmp_cnn_route_bwd": (c_int, [c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_int, c_int, c_int, c_f32, c_ptr, c_ptr]),
    "dmp_cnn_wgrad_chunks": (c_i64, [c_i64]),
    "dmp_cnn_wgrad": (c_int, [c_ptr, c_ptr, c_i64, c_i64, c_i64, c_int, c_int, c_int, c_ptr, c_ptr]),
    "dmp_rnn_fwd": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_int, c_int, c_ptr, c_ptr, c_ptr, c_ptr]),
    "dmp_rnn_bwd": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_int, c_int, c_ptr, c_ptr]),
    "dmp_relconv_supported": (c_int, [c_int, c_int]),
    "dmp_relconv_fwd": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_int, c_int, c_int, c_ptr,
                                c_ptr]),
    "dmp_relconv_bwd": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_int, c_int, c_int, c_ptr,
                                c_ptr]),
    "dmp_relcorr_supported": (c_int, [c_int, c_int, c_int]),
    "dmp_relcorr_weights_fwd": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_int, c_int, c_int, c_f32, c_ptr, c_ptr]),
    "dmp_relcorr_weights_bwd": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_int, c_int, c_int, c_int, c_f32, c_ptr, c_ptr, c_ptr, c_ptr,
                                        c_ptr]),
    "dmp_txl_supported": (c_int, [c_int, c_int, c_int]),
    "dmp_txl_attn_fwd": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_int, c_int, c_f32, c_ptr, c_ptr, c_ptr,
                                 c_ptr]),
    "dmp_txl_bwd_groups": (c_i64, [c_i64, c_int]),
    "dmp_txl_attn_bwd": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_int, c_int, c_int, c_int, c_f32,
                                 c_ptr, c_ptr, c_ptr, c_ptr, c_ptr]),
    "dmp_lrp_workspace_words": (c_size, [c_i64, c_i64]),
    "dmp_lrp_count": (c_int, [c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_int, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr]),
    "dmp_lrp_fill": (c_int, [c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_int, c_i64, c_ptr, c_ptr, c_ptr]),
    "dmp_rank_supported": (c_int, [c_int]),
    "dmp_rank_counts": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_int, c_ptr, c_ptr, c_ptr]),
    "dmp_rank_typed_workspace_words": (c_size, [c_i64]),
    "dmp_rank_counts_typed": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_ptr, c_i64, c_i64, c_int, c_ptr, c_ptr, c_ptr,
                                      c_ptr, c_ptr, c_ptr]),
    "dmp_lrp_pool_supported": (c_int, [c_int, c_int, c_int]),
    "dmp_lrp_pool_workspace_words": (c_size, [c_i64, c_int, c_int, c_int]),
    "dmp_lrp_pool_fwd": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_int, c_int, c_int, c_ptr, c_ptr, c_ptr]),
    "dmp_lrp_pool_bwd": (c_int, [c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, c_i64, c_int, c_int, c_int, c_ptr,
                                 c_ptr, c_ptr, c_ptr, c_ptr]),
    "dmp_collate_resident": (c_int, [_p(dmp_resident_side), c_ptr, c_ptr, c_ptr, c_ptr, c_i64, c_i64, _p(dmp_resident_batch), c_ptr, c_ptr,
                                     c_ptr, c_i64, c_i64, c_ptr, c_ptr]),
    "dmp_subiso_label_dev": (c_int, [_p(dmp_subiso_image), c_i64, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr, c_ptr]),
    "dmp_eval_terms": (c_int, [c_ptr, c_ptr, c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_ptr, c_i64, c_ptr, c_i64, c_ptr, c_ptr, c_i64,
                               c_ptr, c_ptr, c_ptr, c_ptr, c_ptr]),
}
