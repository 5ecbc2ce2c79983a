"""ctypes binding of libmdx.so (the C ABI declared in include/mdx.h).

There is NO fallback: if the shared library is missing or a call fails, an
exception is raised.  `build()` compiles it in-tree with hipcc for gfx950
(cross-compiles without a GPU); the built file travels with the source tree.
"""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MDIR_AMD_LIB") or os.path.join(_HERE, "libmdx.so")   # override: A/B builds only
CSRC = os.path.join(_HERE, "csrc")

MDX_DIM_MAJOR, MDX_ROW_MAJOR = 0, 1
MDX_POOL_GEM, MDX_POOL_MAC, MDX_POOL_SPOC = 0, 1, 2
MDX_F32, MDX_F16, MDX_I8 = 0, 1, 2
MDX_F32_CHAIN, MDX_F32_SPLIT3, MDX_F32_SPLIT2 = 0, 1, 2
RANK_ROUTES = {1: "SMALL", 2: "PACKED", 3: "KV"}              # include/mdx.h MDX_RANK_ROUTE_*
TOPK_ROUTES = {1: "SAMPLED", 2: "SELECT", 3: "SORT"}          # include/mdx.h MDX_TOPK_ROUTE_*
COMPUTE = {"chain": MDX_F32_CHAIN, "exact": MDX_F32_CHAIN, "split3": MDX_F32_SPLIT3, "split2": MDX_F32_SPLIT2}
STORAGE = {"f32": MDX_F32, "f16": MDX_F16, "i8": MDX_I8}
POOL_KINDS = {"gem": MDX_POOL_GEM, "mac": MDX_POOL_MAC, "spoc": MDX_POOL_SPOC}


class MdxError(RuntimeError):
    """A libmdx call returned a negative status."""


_STATUS_EXC = {-1: ValueError, -2: MdxError, -3: MemoryError, -4: ValueError}

_lib = None
ABI_VERSION = 3        # include/mdx.h MDX_ABI_VERSION this binding was written against


def build(force=False):
    """Compile libmdx.so with hipcc --offload-arch=gfx950 (see csrc/Makefile)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))]
    srcs += [os.path.join(_HERE, "..", "include", h) for h in ("mdx.h", "mdx_knn_join.h", "mdx_trunk_f16.h", "mdx_groups.h", "mdx_krecip.h", "mdx_photometric.h", "mdx_train.h", "mdx_kmeans.h", "mdx_ivf.h", "mdx_lists_i8.h", "mdx_lists_pq.h", "mdx_lists_edit.h", "mdx_refine.h", "mdx_knn_reverse.h", "mdx_unet.h", "mdx_overlap.h", "mdx_graph.h")]
    stale = not os.path.exists(LIB_PATH) or \
        any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-C", CSRC] + (["-B"] if force else []))
    return LIB_PATH


class JpegInfo(ctypes.Structure):
    """``mdx_jpeg_info`` of include/mdx.h."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("ncomp", ctypes.c_int32),
                ("hsamp", ctypes.c_int32 * 3), ("vsamp", ctypes.c_int32 * 3),
                ("blocks_w", ctypes.c_int32 * 3), ("blocks_h", ctypes.c_int32 * 3), ("supported", ctypes.c_int32),
                ("block_offset", ctypes.c_int64 * 3), ("nblocks", ctypes.c_int64)]


def _declare(lib):
    i32, i64, f32, p = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    pp = ctypes.POINTER(ctypes.c_void_p)
    pi64 = ctypes.POINTER(ctypes.c_int64)
    sig = {
        "mdx_abi_version": (i32, []),
        "mdx_last_error": (ctypes.c_char_p, []),
        "mdx_capture_recover": (i32, [p]),
        "mdx_rmac_workspace": (i64, [i32, i32, i32]),
        "mdx_rmac": (i32, [p, i32, i32, i32, i32, ctypes.POINTER(ctypes.c_int32), i32, f32, p, i64, p, p]),
        "mdx_roipool": (i32, [p, i32, i32, i32, i32, ctypes.POINTER(ctypes.c_int32), i32, i32, f32, f32, p, p]),
        "mdx_region_sum": (i32, [p, i32, i32, i32, f32, p, p]),
        "mdx_pool_l2n": (i32, [p, i32, i32, i32, i32, i32, f32, f32, f32, p, p]),
        "mdx_l2n_rows": (i32, [p, i64, i64, p, f32, p]),
        "mdx_ms_aggregate": (i32, [pp, i32, i64, f32, p, p]),
        "mdx_ms_aggregate_batch": (i32, [pp, i32, i64, i64, f32, p, p]),
        "mdx_pool_multi": (i32, [pp, i32, i32, i32, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), i32, f32, f32, p, p]),
        "mdx_l2n_aggregate": (i32, [p, i32, i64, i64, f32, f32, p, p]),
        "mdx_bn_act": (i32, [p, p, i64, i64, i64, p, p, p, p, f32, i32, p]),
        "mdx_u8_to_chw": (i32, [p, i64, i64, i64, i32, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), p, p]),
        "mdx_clahe_workspace": (i64, [i64, i64, i64, i32, i32]),
        "mdx_clahe_u8_to_chw": (i32, [p, i64, i64, i64, i32, i32, i32, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), p, i64, p, p]),
        "mdx_bilinear_pyramid": (i32, [p, i64, i64, i32, i32, i32, ctypes.POINTER(ctypes.c_double), pp, p]),
        "mdx_resample_u8": (i32, [p, i64, i32, i32, i32, i32, i32, p, p, i32, p, p]),
        "mdx_jpeg_probe": (i32, [p, i64, p]),
        "mdx_jpeg_coefficients": (i32, [p, i64, p, i64, p]),
        "mdx_jpeg_pixels": (i32, [p, p, p, p, p, p]),
        "mdx_index_create": (i32, [pp, p, i64, i64, i32, i64, p]),
        "mdx_index_create_ex": (i32, [pp, p, i64, i64, i32, i64, i32, p]),
        "mdx_index_bytes": (i64, [i64, i64, i32]),
        "mdx_index_create_in": (i32, [pp, p, i64, i64, i32, i64, i32, p, i64, p]),
        "mdx_index_destroy": (i32, [p]),
        "mdx_rescore_workspace": (i64, [i64, i64, i64]),
        "mdx_rescore": (i32, [p, i64, i64, i64, p, i64, i32, p, p, i64, p, p, p, i64, p]),
        "mdx_index_i8_bounds": (i32, [p, p, p]),
        "mdx_rescore_certify": (i32, [p, i64, i64, p, p, i64, i32, p, p, i64, p, p, p]),
        "mdx_center_rows": (i32, [p, i64, i64, i32, p, p, p]),
        "mdx_join_stats": (i32, [p, p, i64, p, p]),
        "mdx_join_candidates": (i32, [p, p, p, p, i64, i64, i32, f32, p, i64, p, p]),
        "mdx_join_resolve_workspace": (i64, [i64, i64]),
        "mdx_join_resolve": (i32, [p, i64, p, i64, i64, p, i64, f32, i64, i64, p, p, p, p, i64, p]),
        "mdx_range_select_workspace": (i64, [i64, i64]),
        "mdx_range_select": (i32, [p, i64, i64, i64, f32, i64, p, p, p, i64, p, i64, p]),
        "mdx_knn_bounds_workspace": (i64, [i64, i64, i64, i64]),
        "mdx_knn_bounds": (i32, [p, p, p, p, i64, i64, i64, i64, p, p, i64, p]),
        "mdx_join_candidates_rows": (i32, [p, p, p, p, i64, i64, p, p, i64, p, p]),
        "mdx_knn_resolve_workspace": (i64, [i64, i64]),
        "mdx_knn_resolve": (i32, [p, i64, p, i64, i64, p, i64, i64, i64, i64, p, p, p, p, i64, p]),
        "mdx_groups_init": (i32, [p, i64, i64, p, p]),
        "mdx_groups_union_pairs": (i32, [p, i64, i64, p, i64, ctypes.POINTER(ctypes.c_float), i64, p, i64, p, p]),
        "mdx_groups_union_dense": (i32, [p, i64, i64, i64, i64, i64, ctypes.POINTER(ctypes.c_float), i64, p, i64, p, p]),
        "mdx_groups_labels": (i32, [p, i64, i64, p, p]),
        "mdx_krecip_sets": (i32, [p, i64, i64, p, p, p, p, p]),
        "mdx_krecip_raw_offsets": (i32, [i64, i64, p, p, p, p, p, p]),
        "mdx_krecip_raw_fill": (i32, [p, i64, i64, p, p, i64, i64, p, p, p, p, p, p, p, i64, p]),
        "mdx_krecip_expand_offsets": (i32, [p, i64, i64, i64, p, p, i64, p, p]),
        "mdx_krecip_expand_fill": (i32, [p, i64, i64, i64, p, p, p, i64, p, p, p, i64, p]),
        "mdx_krecip_rerank_workspace": (i64, [i64, i64]),
        "mdx_krecip_rerank": (i32, [p, p, p, i64, i64, i64, p, p, p, i64, p, p, p, i64, p, i64, p, i64, i64, f32, p, i64, p, i64, p]),
        "mdx_photometric_workspace": (i64, [i64, i64, i64]),
        "mdx_photometric_tables": (i32, [p, p]),
        "mdx_histmatch_u8_to_chw": (i32, [p, i64, i64, i64, p, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), p, i64, p, p]),
        "mdx_gamma_u8_to_chw": (i32, [p, i64, i64, i64, ctypes.c_double, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), p, i64, p, p]),
        "mdx_pool_bwd_workspace": (i64, [i32, i32]),
        "mdx_pool_bwd": (i32, [p, p, p, i32, i32, i32, i32, i32, f32, f32, p, p, p, i64, p]),
        "mdx_l2n_rows_bwd": (i32, [p, p, i64, i64, f32, p, p]),
        "mdx_tuple_loss_workspace": (i64, [i64]),
        "mdx_contrastive_loss": (i32, [p, p, i64, i64, i64, f32, f32, p, p, p, i64, p]),
        "mdx_triplet_loss": (i32, [p, p, i64, i64, i64, f32, p, p, p, i64, p]),
        "mdx_kmeans_argmax": (i32, [p, i64, i64, i64, p, p, p]),
        "mdx_kmeans_sums_workspace": (i64, [i64, i64, i64]),
        "mdx_kmeans_sums": (i32, [p, i64, i64, i64, p, p, i64, p, p, i64, p]),
        "mdx_kmeans_finish": (i32, [p, i64, i64, f32, p, p, p]),
        "mdx_ivf_plan_workspace": (i64, [i64, i64, i64]),
        "mdx_ivf_plan": (i32, [p, i64, i64, p, i64, i64, i64, p, i64, p]),
        "mdx_ivf_scan": (i32, [p, i64, i64, i64, p, i64, p, i64, p, i64, i32, p, i64, p, i64, i64, i64, p, p, p]),
        "mdx_ivf_select": (i32, [p, p, i64, i64, i64, i64, p, i64, i64, p, p, p]),
        "mdx_lists_i8_encode": (i32, [p, i64, i64, i64, p, i64, p, p, p]),
        "mdx_lists_i8_bounds": (i32, [p, p, i64, i64, p, p]),
        "mdx_lists_i8_scan": (i32, [p, p, i64, i64, p, p, i64, p, p, i64, i64, p, i64, i64, i64, p, p, p]),
        "mdx_pq_lut": (i32, [p, i64, i64, p, i64, i32, p, p, p]),
        "mdx_lists_pq_scan": (i32, [p, i64, i64, i64, p, i64, p, i64, p, p, p, i64, i64, p, i64, i64, p, p, p]),
        "mdx_lists_merge": (i32, [p, i64, p, p, i64, p, i64, p, p, i64, i64, i64, p, i64, p, p, p]),
        "mdx_lists_compact": (i32, [p, i64, p, p, i64, i64, i64, p, i64, p, i64, p, p, p]),
        "mdx_refine_i8_workspace": (i64, [i64, i64]),
        "mdx_refine_i8": (i32, [p, p, i64, i64, p, i64, p, p, i64, p, i64, p, p, p, i64, p]),
        "mdx_knn_reverse_count": (i32, [p, p, i64, i64, p, p]),
        "mdx_knn_reverse_fill": (i32, [p, p, i64, i64, p, p, p, i64, p]),
        "mdx_knn_reverse_merge": (i32, [p, p, i64, i64, p, p, i64, p, p, p, p]),
        "mdx_bn_act_into": (i32, [p, p, i64, i64, i64, i64, p, p, p, p, f32, i32, f32, p]),
        "mdx_topk_overlap": (i32, [p, i64, p, i64, i64, ctypes.POINTER(ctypes.c_int32), i64, p, p]),
        "mdx_graph_search": (i32, [p, i64, i64, i64, p, i64, p, i64, i32, p, p, i64, i64, i64, i64, i64, i32, p, p, p, p, p]),
        "mdx_graph_detours": (i32, [p, i64, i64, p, p]),
        "mdx_bn_act_f16": (i32, [p, p, i64, i64, i64, p, p, p, p, f32, i32, p]),
        "mdx_pool_l2n_f16": (i32, [p, i32, i32, i32, i32, i32, f32, f32, f32, p, p]),
        "mdx_pool_multi_f16": (i32, [pp, i32, i32, i32, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), i32, f32, f32, p, p]),
        "mdx_index_info": (i32, [p, pi64, pi64, pi64, pi64]),
        "mdx_scores_workspace": (i64, [i64, i64]),
        "mdx_quantize_i8": (i32, [p, i64, i64, i32, p, p, p]),
        "mdx_scores": (i32, [p, p, i64, i32, p, p, p, i64, p]),
        "mdx_scores_rowmajor": (i32, [p, i64, i64, p, i64, i32, p, p, p, i64, p]),
        "mdx_scores_workspace_ex": (i64, [i64, i64, i32]),
        "mdx_scores_ex": (i32, [p, p, i64, i32, p, p, p, i64, i32, p]),
        "mdx_rank_workspace": (i64, [i64, i64]),
        "mdx_rank_full": (i32, [p, i64, i64, i64, p, p, i64, p]),
        "mdx_rank_full_segments": (i32, [pp, pi64, i32, i64, i64, p, p, i64, p]),
        "mdx_topk": (i32, [p, i64, i64, i64, i64, p, p, p, i64, p]),
        "mdx_rank_route": (i32, [i64, p]),
        "mdx_topk_route": (i32, [i64, i64, i64, i64]),
        "mdx_rank_of": (i32, [p, i64, i64, p, p, i64, p, p, p]),
        "mdx_rank_positions": (i32, [p, i64, i64, i64, p, p, i64, p, p]),
        "mdx_gather_scores": (i32, [p, i64, i64, p, p, i64, p, p]),
        "mdx_rank_count": (i32, [p, i64, i64, i64, p, p, p, i64, p, p]),
        "mdx_knn_aggregate": (i32, [p, i64, i64, i64, p, p, i64, i64, p, i64, f32, f32, p, i64, p]),
        "mdx_knn_graph_workspace": (i64, [i64]),
        "mdx_knn_graph": (i32, [p, p, i64, i64, f32, p, p, p, p, i64, p]),
        "mdx_diffusion_workspace": (i64, [i64, i64]),
        "mdx_diffusion": (i32, [p, p, p, i64, i64, p, i64, p, p, i64, i64, f32, f32, i64, f32, p, i64, p, p, p, i64, p]),
        "mdx_knn_graph_weights": (i32, [p, p, i64, i64, f32, p, p, p, p, i64, p]),
        "mdx_diffusion_truncated_workspace": (i64, [i64, i64, i64, i64]),
        "mdx_diffusion_truncated": (i32, [p, p, p, i64, i64, p, i64, p, p, i64, i64, i64, f32, f32, i64, f32, p, i64, p, p, p, i64,
                                          p]),
        "mdx_conv1x1_transpose_weights": (i32, [p, i64, i64, p, p]),
        "mdx_conv1x1_bn_act": (i32, [p, p, i64, i64, i64, i64, p, p, p, p, f32, p, i32, p, p]),
        "mdx_gram_f64_workspace": (i64, [i64, i64]),
        "mdx_gram_f64": (i32, [p, i64, i64, p, p, p, i64, p]),
        "mdx_project_f64_workspace": (i64, [i64, i64]),
        "mdx_project_f64": (i32, [p, i64, i64, p, i64, p, p, p, i64, p]),
        "mdx_l2n_cols_f64": (i32, [p, i64, i64, ctypes.c_double, p]),
        "mdx_comm_unique_id": (i32, [p]),
        "mdx_comm_init": (i32, [pp, p, i32, i32]),
        "mdx_comm_destroy": (i32, [p]),
        "mdx_comm_info": (i32, [p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
        "mdx_query_bounds": (i32, [i64, i32, i32, pi64, pi64]),
        "mdx_allgather_scores": (i32, [p, p, i64, pi64, p, p]),
        "mdx_exchange_scores": (i32, [p, p, i64, pi64, p, p]),
        "mdx_p2p_create": (i32, [pp, i32, i32, i64, i64, p]),
        "mdx_p2p_connect": (i32, [p, p]),
        "mdx_p2p_connect_ptrs": (i32, [p, pp]),
        "mdx_p2p_base": (p, [p]),
        "mdx_p2p_bytes": (i64, [p]),
        "mdx_scores_p2p": (i32, [p, p, i64, i32, p, p, p, i64, p]),
        "mdx_p2p_close_step": (i32, [p, pp, p]),
        "mdx_p2p_status": (i32, [p, ctypes.POINTER(ctypes.c_uint32), p]),
        "mdx_p2p_destroy": (i32, [p]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export it
        fn.restype, fn.argtypes = res, args
    return sig


EXPORTS = ("mdx_abi_version", "mdx_last_error", "mdx_capture_recover", "mdx_rmac_workspace", "mdx_rmac", "mdx_roipool", "mdx_region_sum", "mdx_pool_l2n", "mdx_l2n_rows", "mdx_ms_aggregate",
           "mdx_ms_aggregate_batch", "mdx_pool_multi", "mdx_l2n_aggregate", "mdx_bn_act", "mdx_u8_to_chw", "mdx_resample_u8", "mdx_bilinear_pyramid", "mdx_jpeg_probe", "mdx_jpeg_coefficients", "mdx_jpeg_pixels",
           "mdx_index_create", "mdx_index_create_ex", "mdx_index_bytes", "mdx_index_create_in", "mdx_index_destroy", "mdx_index_info", "mdx_scores_workspace", "mdx_quantize_i8",
           "mdx_scores", "mdx_scores_rowmajor", "mdx_scores_workspace_ex", "mdx_scores_ex", "mdx_rank_workspace", "mdx_rank_full", "mdx_rank_full_segments", "mdx_topk", "mdx_rank_route", "mdx_topk_route", "mdx_rank_of", "mdx_rank_positions",
           "mdx_gather_scores", "mdx_rank_count", "mdx_knn_aggregate", "mdx_knn_graph_workspace", "mdx_knn_graph",
           "mdx_diffusion_workspace", "mdx_diffusion", "mdx_knn_graph_weights", "mdx_diffusion_truncated_workspace",
           "mdx_diffusion_truncated", "mdx_rescore_workspace", "mdx_rescore", "mdx_index_i8_bounds", "mdx_rescore_certify",
           "mdx_center_rows", "mdx_join_stats", "mdx_join_candidates", "mdx_join_resolve_workspace", "mdx_join_resolve",
           "mdx_range_select_workspace", "mdx_range_select",
           "mdx_conv1x1_transpose_weights", "mdx_conv1x1_bn_act", "mdx_clahe_workspace", "mdx_clahe_u8_to_chw", "mdx_gram_f64_workspace", "mdx_gram_f64", "mdx_project_f64_workspace", "mdx_project_f64", "mdx_l2n_cols_f64", "mdx_comm_unique_id", "mdx_comm_init",
           "mdx_comm_destroy", "mdx_comm_info", "mdx_query_bounds", "mdx_allgather_scores", "mdx_exchange_scores",
           "mdx_p2p_create", "mdx_p2p_connect", "mdx_p2p_connect_ptrs", "mdx_p2p_base", "mdx_p2p_bytes", "mdx_scores_p2p", "mdx_p2p_close_step",
           "mdx_p2p_status", "mdx_p2p_destroy")

# include/mdx_knn_join.h (included by mdx.h): the exact kNN join.  Apart from EXPORTS because tests/test_cabi.py and
# tests/test_memguard_host.py pin EXPORTS to mdx.h's own prototypes and their number; tests/test_knn_join_host.py is the census
# of these (include/mdx.h, "exact kNN join", says more)
KNN_JOIN_EXPORTS = ("mdx_knn_bounds_workspace", "mdx_knn_bounds", "mdx_join_candidates_rows", "mdx_knn_resolve_workspace", "mdx_knn_resolve")

# include/mdx_trunk_f16.h (included by mdx.h): the fp16 trunk mode, apart from EXPORTS for the same reason; the census of these is
# tests/test_trunk_f16_host.py (include/mdx.h, "fp16 trunk")
TRUNK_F16_EXPORTS = ("mdx_bn_act_f16", "mdx_pool_l2n_f16", "mdx_pool_multi_f16")

# include/mdx_groups.h (included by mdx.h): the near-duplicate groups, apart from EXPORTS for the same reason; the census of these
# is tests/test_groups_host.py (include/mdx.h, "near-duplicate groups")
GROUPS_EXPORTS = ("mdx_groups_init", "mdx_groups_union_pairs", "mdx_groups_union_dense", "mdx_groups_labels")

# include/mdx_krecip.h (included by mdx.h): k-reciprocal re-ranking, apart from EXPORTS for the same reason; the census of these is
# tests/test_krecip_host.py (include/mdx.h, "k-reciprocal re-ranking")
KRECIP_EXPORTS = ("mdx_krecip_sets", "mdx_krecip_raw_offsets", "mdx_krecip_raw_fill", "mdx_krecip_expand_offsets",
                  "mdx_krecip_expand_fill", "mdx_krecip_rerank_workspace", "mdx_krecip_rerank")

# include/mdx_photometric.h (included by mdx.h): histogram matching and gamma equalisation, apart from EXPORTS for the same reason; the
# census of these is tests/test_photometric_host.py (include/mdx.h, "photometric normalisation")
PHOTOMETRIC_EXPORTS = ("mdx_photometric_workspace", "mdx_photometric_tables", "mdx_histmatch_u8_to_chw", "mdx_gamma_u8_to_chw")

# include/mdx_train.h (included by mdx.h): the backward of the descriptor tail and the tuple losses, apart from EXPORTS for the same
# reason; the census of these is tests/test_train_host.py (include/mdx.h, "trainable tail")
TRAIN_EXPORTS = ("mdx_pool_bwd_workspace", "mdx_pool_bwd", "mdx_l2n_rows_bwd", "mdx_tuple_loss_workspace", "mdx_contrastive_loss",
                 "mdx_triplet_loss")

# include/mdx_kmeans.h (included by mdx.h): spherical k-means, apart from EXPORTS for the same reason; the census of these is
# tests/test_kmeans_host.py (include/mdx.h, "spherical k-means")
KMEANS_EXPORTS = ("mdx_kmeans_argmax", "mdx_kmeans_sums_workspace", "mdx_kmeans_sums", "mdx_kmeans_finish")

# include/mdx_ivf.h (included by mdx.h): the inverted file, apart from EXPORTS for the same reason; the census of these is
# tests/test_ivf_host.py (include/mdx.h, "inverted file")
IVF_EXPORTS = ("mdx_ivf_plan_workspace", "mdx_ivf_plan", "mdx_ivf_scan", "mdx_ivf_select")

# include/mdx_lists_i8.h (included by mdx.h): int8 list storage for the inverted file, apart from EXPORTS for the same reason; the
# census of these is tests/test_lists_i8_host.py (include/mdx.h, "inverted file, int8 lists")
LISTS_I8_EXPORTS = ("mdx_lists_i8_encode", "mdx_lists_i8_bounds", "mdx_lists_i8_scan")

# include/mdx_lists_pq.h (included by mdx.h): product-quantised lists for the inverted file, apart from EXPORTS for the same reason; the
# census of these is tests/test_pq_host.py (include/mdx.h, "inverted file, product-quantised lists")
LISTS_PQ_EXPORTS = ("mdx_pq_lut", "mdx_lists_pq_scan")

# include/mdx_lists_edit.h (included by mdx.h): merging and compacting the lists of the inverted file, apart from EXPORTS for the same
# reason; the census of these is tests/test_lists_edit_host.py (include/mdx.h, "inverted file, editing the lists")
LISTS_EDIT_EXPORTS = ("mdx_lists_merge", "mdx_lists_compact")

# include/mdx_refine.h (included by mdx.h): int8 refinement of shortlists on codes kept in list order, apart from EXPORTS for the same
# reason; the census of these is tests/test_refine_host.py (include/mdx.h, "inverted file, int8 refinement of shortlists")
REFINE_EXPORTS = ("mdx_refine_i8_workspace", "mdx_refine_i8")

# include/mdx_knn_reverse.h (included by mdx.h): the reverse-edge merge of kNN lists, apart from EXPORTS for the same reason; the census
# of these is tests/test_knn_reverse_host.py (include/mdx.h, "kNN lists, reverse-edge merge")
KNN_REVERSE_EXPORTS = ("mdx_knn_reverse_count", "mdx_knn_reverse_fill", "mdx_knn_reverse_merge")

# include/mdx_unet.h (included by mdx.h): the U-Net epilogue into a channel slice, apart from EXPORTS for the same reason; the census of
# these is tests/test_unet_host.py (include/mdx.h, "U-Net epilogue")
UNET_EXPORTS = ("mdx_bn_act_into",)
MDX_ACT_NONE, MDX_ACT_RELU, MDX_ACT_LEAKY = 0, 1, 2            # include/mdx_unet.h

# include/mdx_overlap.h (included by mdx.h): the overlap of two sets of top-K lists, apart from EXPORTS for the same reason; the census
# of these is tests/test_overlap_host.py (include/mdx.h, "top-K lists, overlap")
OVERLAP_EXPORTS = ("mdx_topk_overlap",)

# include/mdx_graph.h (included by mdx.h): the graph index, apart from EXPORTS for the same reason; the census of these is
# tests/test_graph_host.py (include/mdx.h, "graph index")
GRAPH_EXPORTS = ("mdx_graph_search", "mdx_graph_detours")


def lib():
    """The loaded library; raises if it was never built (no silent fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MdxError("libmdx.so is not built (%s); run `python -c 'import __graft_entry__ as g; "
                           "g.build()'` or `make -C mdir_amd/csrc`" % LIB_PATH)
        # torch first: its wheel carries its own libamdhip64, and libmdx.so must bind to THAT copy of the HIP runtime -- loaded
        # before torch it would pull in /opt/rocm's, and a process with two HIP runtimes loses the device ("no ROCm-capable
        # device is detected" at the first launch)
        import torch  # noqa: F401
        handle = ctypes.CDLL(LIB_PATH)
        _declare(handle)
        if handle.mdx_abi_version() != ABI_VERSION:
            raise MdxError("libmdx.so ABI version %d, this package binds version %d (include/mdx.h MDX_ABI_VERSION): rebuild "
                           "with `make -C mdir_amd/csrc`" % (handle.mdx_abi_version(), ABI_VERSION))
        _lib = handle
    return _lib


def check(status, what=""):
    if status != 0:
        msg = lib().mdx_last_error().decode(errors="replace")
        raise _STATUS_EXC.get(status, MdxError)("%s failed (status %d): %s" % (what or "libmdx", status, msg))
