"""
ctypes binding of libprosstt_amd.so (include/prosstt_amd.h) and of the libraries beside it: each is described once in
LIBRARIES, ADDED_LIBRARIES, LATER_LIBRARIES or NEWER_LIBRARIES (the sampler's later entry points in SAMPLER_LATER), and load /
check do the rest.

There is NO CPU fallback: if the library is missing, or no gfx950 device is
visible, every numeric entry point of the package raises.  torch is used only
as plumbing (device memory, the current stream, torch.distributed).
"""
import ctypes
import os
import threading
from collections import namedtuple

_HERE = os.path.dirname(os.path.abspath(__file__))

OK, EINVAL, EDOMAIN, EHIP, ENOMEM, ENODEV, ERCCL = 0, -1, -2, -3, -4, -5, -6
HOST_INPUTS, HOST_OUTPUT, CHECK_DOMAIN, TIME_KERNEL, CHECK_DEFERRED, MEANS_CACHED, PARAMS_NONNEG = 1, 2, 4, 8, 16, 32, 64
STATS_ACCUMULATE = 1

# One shared library, by the name of its row in prosstt_amd/csrc/Makefile: ``path`` (its environment variable overrides
# the file in lib/), ``header`` (the file under include/ that declares it), ``hip`` (it runs on the device: torch is
# imported before it, and there is no CPU fallback for it), ``symbols`` (every symbol its header declares -> (restype,
# argtypes or None for "not declared here")), ``last_error`` (the symbol that returns the message of a failed call, or
# None).
_Library = namedtuple("_Library", "path header hip symbols last_error")


def _path(env, filename):
    return os.environ.get(env) or os.path.join(_HERE, "lib", filename)


def _int(*argtypes):
    return ctypes.c_int, list(argtypes)


_ptr_to = ctypes.POINTER
_text = (ctypes.c_char_p, None)
vp, i32, i64, u32, u64, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_double
_widen = _int(vp, vp, u64, i32)

LIBRARIES = {
    "sampler": _Library(_path("PROSSTT_AMD_LIB", "libprosstt_amd.so"), "prosstt_amd.h", True, {
        "prosstt_amd_version": (ctypes.c_int, None),
        "prosstt_amd_last_error": _text,
        "prosstt_amd_device_count": _int(_ptr_to(ctypes.c_int)),
        "prosstt_amd_ctx_create": _int(ctypes.c_int, vp, _ptr_to(vp)),
        "prosstt_amd_ctx_destroy": _int(vp),
        "prosstt_amd_ctx_synchronize": _int(vp),
        "prosstt_amd_last_kernel_ms": _int(vp, _ptr_to(ctypes.c_float)),
        "prosstt_amd_sample_counts": _int(vp, vp, i64, i32, vp, vp, vp, vp, i64, u64, u64, vp, vp, i64, u32),
        "prosstt_amd_plan_order": _int(vp, i64, i64, vp),
        "prosstt_amd_last_list": _int(vp, vp, vp, i64, _ptr_to(i64), _ptr_to(i32)),
        "prosstt_amd_run_plan": _int(vp, i64, i64, i32, vp),
        "prosstt_amd_last_run_plan": _int(vp, vp, i64, _ptr_to(i64), _ptr_to(i32)),
        "prosstt_amd_nb_params": _int(vp, vp, i64, i32, vp, vp, vp, vp, i64, vp, vp, vp, vp, u32),
        "prosstt_amd_hw_math": _int(vp, i32, u32, u64, vp, u32),
        "prosstt_amd_hw_math_at": _int(vp, i32, vp, u64, vp, u32),
        "prosstt_amd_comm_unique_id": _int(vp),
        "prosstt_amd_comm_init": _int(vp, vp, i32, i32, _ptr_to(vp)),
        "prosstt_amd_comm_destroy": _int(vp),
        "prosstt_amd_gather_counts": _int(vp, vp, vp, vp, i32, i32, vp),
        "prosstt_amd_comm_selftest": _int(vp, vp, u64),
        "prosstt_amd_domain_status": _int(vp, _ptr_to(i32)),
        "prosstt_amd_numpy_programs": _int(vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp),
        "prosstt_amd_lineage_attempt": _int(vp, vp, i32, i32, vp, i64, i32, vp, vp, vp, vp),
        "prosstt_amd_lineage_attempt_batch": _int(vp, vp, i32, i32, i32, vp, i64, i32, vp, vp, vp, vp),
        "prosstt_amd_lineage_walk": _int(vp, u64, u64, i32, i32, vp),
        "prosstt_amd_lineage_walk_batch": _int(vp, u64, u64, i32, i32, i32, vp),
        "prosstt_amd_lineage_commit": _int(vp, vp, i32, i32, vp, i64, vp, vp),
        "prosstt_amd_gene_max": _int(vp, vp, i64, i64, vp),
        "prosstt_amd_means_from_rel": _int(vp, vp, vp, i64, i64, vp),
    }, "prosstt_amd_last_error"),
    # host-side helpers, no HIP
    "host": _Library(_path("PROSSTT_AMD_HOST_LIB", "libprosstt_amd_host.so"), "prosstt_amd_host.h", False, {
        "prosstt_amd_host_widen_i32_i64": _widen,
        "prosstt_amd_host_widen_u16_i64": _widen,
        "prosstt_amd_host_widen_u16_i32": _widen,
        "prosstt_amd_host_widen_u8_i64": _widen,
        "prosstt_amd_host_widen_u8_i32": _widen,
        "prosstt_amd_host_scatter_i32": _int(vp, i32, vp, vp, u64, i32),
        "prosstt_amd_host_has_avx2": (ctypes.c_int, None),
    }, None),
    # summary statistics of a device count matrix
    "stats": _Library(_path("PROSSTT_AMD_STATS_LIB", "libprosstt_amd_stats.so"), "prosstt_amd_stats.h", True, {
        "prosstt_amd_stats_last_error": _text,
        "prosstt_amd_stats_workspace_bytes": _int(i64, i64, _ptr_to(u64)),
        "prosstt_amd_stats_count_summary": _int(vp, vp, i64, i64, i64, vp, u64, vp, vp, vp, vp, vp, vp, u32),
    }, "prosstt_amd_stats_last_error"),
    # products with the log-normalised count matrix
    "embed": _Library(_path("PROSSTT_AMD_EMBED_LIB", "libprosstt_amd_embed.so"), "prosstt_amd_embed.h", True, {
        "prosstt_amd_embed_last_error": _text,
        "prosstt_amd_embed_workspace_bytes": _int(i64, i64, i64, _ptr_to(u64)),
        "prosstt_amd_embed_gene_moments": _int(vp, vp, i64, i64, i64, vp, vp, u64, vp, vp, vp),
        "prosstt_amd_embed_matmul": _int(vp, vp, i64, i64, i64, vp, vp, i64, vp, vp, u64, vp),
        "prosstt_amd_embed_rmatmul": _int(vp, vp, i64, i64, i64, vp, vp, i64, vp, vp, u64, vp),
    }, "prosstt_amd_embed_last_error"),
    # exact k nearest neighbours of the rows of an f32 panel
    "knn": _Library(_path("PROSSTT_AMD_KNN_LIB", "libprosstt_amd_knn.so"), "prosstt_amd_knn.h", True, {
        "prosstt_amd_knn_last_error": _text,
        "prosstt_amd_knn_workspace_bytes": _int(i64, i64, i64, i64, _ptr_to(u64)),
        "prosstt_amd_knn_search": _int(vp, vp, i64, i64, i64, i64, i64, vp, vp, vp, u64),
    }, "prosstt_amd_knn_last_error"),
    # connectivities of the kNN graph and its diffusion operator
    "graph": _Library(_path("PROSSTT_AMD_GRAPH_LIB", "libprosstt_amd_graph.so"), "prosstt_amd_graph.h", True, {
        "prosstt_amd_graph_last_error": _text,
        "prosstt_amd_graph_workspace_bytes": _int(i64, i64, _ptr_to(u64)),
        "prosstt_amd_graph_memberships": _int(vp, vp, vp, i64, i64, vp, vp, vp, vp),
        "prosstt_amd_graph_symmetrize_emit": _int(vp, vp, vp, i64, i64, vp, u64),
        "prosstt_amd_graph_symmetrize_fold": _int(vp, vp, vp, vp, i64, i64, i64, vp, u64, vp, vp, vp),
        "prosstt_amd_graph_normalize": _int(vp, vp, vp, vp, i64, i64, vp, vp, vp, vp),
        "prosstt_amd_graph_spmv": _int(vp, vp, vp, vp, i64, i64, vp, vp, i32),
    }, "prosstt_amd_graph_last_error"),
    # the epochs of a UMAP layout of the connectivity graph
    "layout": _Library(_path("PROSSTT_AMD_LAYOUT_LIB", "libprosstt_amd_layout.so"), "prosstt_amd_layout.h", True, {
        "prosstt_amd_layout_last_error": _text,
        "prosstt_amd_layout_epochs": _int(vp, vp, vp, vp, i64, i64, i32, vp, vp, i32, i32, i32, f64, f64, f64, f64, i32, u64, i32),
        "prosstt_amd_layout_negatives": _int(vp, u64, i32, i64, i64, i32, i64, vp),
    }, "prosstt_amd_layout_last_error"),
}

# Libraries added after tests/test_native_libraries.py pinned its census of LIBRARIES (the names and symbol counts of the
# seven rows above): rows of the same shape, looked up after LIBRARIES; tests/test_native_tsne.py holds their census.
# Merging the two tables, and the two censuses with them, is a follow-up.
ADDED_LIBRARIES = {
    # exact t-SNE: affinities, the all-pairs gradient, its descent and the objective
    "tsne": _Library(_path("PROSSTT_AMD_TSNE_LIB", "libprosstt_amd_tsne.so"), "prosstt_amd_tsne.h", True, {
        "prosstt_amd_tsne_last_error": _text,
        "prosstt_amd_tsne_workspace_bytes": _int(i64, i32, i32, _ptr_to(u64)),
        "prosstt_amd_tsne_affinities": _int(vp, vp, vp, i64, i64, f64, vp, vp, vp),
        "prosstt_amd_tsne_symmetrize_fold": _int(vp, vp, vp, vp, i64, i64, i64, vp, u64, vp, vp, vp),
        "prosstt_amd_tsne_gradient": _int(vp, vp, vp, vp, i64, i64, i32, vp, f64, i32, vp, u64, vp, vp, vp),
        "prosstt_amd_tsne_iterations": _int(vp, vp, vp, vp, i64, i64, i32, vp, vp, vp, vp, i32, i32, i32, f64, f64, i32, vp, u64),
        "prosstt_amd_tsne_objective": _int(vp, vp, vp, vp, i64, i64, i32, vp, vp),
    }, "prosstt_amd_tsne_last_error"),
}

# Every library added after that goes HERE: tests/test_native_tsne.py pinned the names of ADDED_LIBRARIES in its turn.  Rows
# of the same shape, looked up after the other two tables; tests/test_native_later.py checks each row against its header,
# its makefile row and the built library, and takes the symbol count from the header, so that a new row breaks no test.
LATER_LIBRARIES = {
    # diffusion pseudotime: distance rows of a diffusion map and the concordance sums of its branching
    "dpt": _Library(_path("PROSSTT_AMD_DPT_LIB", "libprosstt_amd_dpt.so"), "prosstt_amd_dpt.h", True, {
        "prosstt_amd_dpt_last_error": _text,
        "prosstt_amd_dpt_workspace_bytes": _int(i64, i32, i32, _ptr_to(u64)),
        "prosstt_amd_dpt_rows": _int(vp, vp, i64, vp, i64, i64, vp, i64, vp),
        "prosstt_amd_dpt_concordance": _int(vp, vp, vp, i64, i32, i32, vp, u64, vp, vp),
    }, "prosstt_amd_dpt_last_error"),
    # marker genes: per-group sums over the log-normalised count matrix
    "markers": _Library(_path("PROSSTT_AMD_MARKERS_LIB", "libprosstt_amd_markers.so"), "prosstt_amd_markers.h", True, {
        "prosstt_amd_markers_last_error": _text,
        "prosstt_amd_markers_workspace_bytes": _int(i64, i64, i64, i64, _ptr_to(u64)),
        "prosstt_amd_markers_group_moments": _int(vp, vp, i64, i64, i64, vp, vp, i64, vp, i64, i64, vp, u64, vp, vp, vp, vp, vp),
    }, "prosstt_amd_markers_last_error"),
    # Louvain clustering of the connectivities: quantised weights, sweeps, community totals and the aggregation
    "cluster": _Library(_path("PROSSTT_AMD_CLUSTER_LIB", "libprosstt_amd_cluster.so"), "prosstt_amd_cluster.h", True, {
        "prosstt_amd_cluster_last_error": _text,
        "prosstt_amd_cluster_workspace_bytes": _int(i64, i64, _ptr_to(u64)),
        "prosstt_amd_cluster_quantize": _int(vp, vp, vp, vp, i64, i64, vp, vp, vp),
        "prosstt_amd_cluster_sweep": _int(vp, vp, vp, vp, vp, i64, i64, vp, i64, i64, i64, vp, vp, i64, f64, i32, i32, vp, vp, vp),
        "prosstt_amd_cluster_totals": _int(vp, vp, vp, vp, vp, i64, i64, vp, vp, vp, vp),
        "prosstt_amd_cluster_aggregate_emit": _int(vp, vp, vp, i64, i64, vp, i64, vp, u64, vp),
        "prosstt_amd_cluster_aggregate_fold": _int(vp, vp, vp, vp, vp, i64, i64, i64, vp, vp, vp, vp),
    }, "prosstt_amd_cluster_last_error"),
    # Wilcoxon marker genes: per gene a sort of the log-normalised entries, folded into exact rank sums per group
    "ranks": _Library(_path("PROSSTT_AMD_RANKS_LIB", "libprosstt_amd_ranks.so"), "prosstt_amd_ranks.h", True, {
        "prosstt_amd_ranks_last_error": _text,
        "prosstt_amd_ranks_workspace_bytes": _int(i64, i64, i64, _ptr_to(u64)),
        "prosstt_amd_ranks_rank_sums": _int(vp, vp, i64, i64, i64, vp, vp, i64, vp, i64, i64, i64, vp, u64, vp, vp, vp),
    }, "prosstt_amd_ranks_last_error"),
    # highly variable genes: sums of the counts clipped per gene, moments of x / s, and the chosen columns as a new matrix
    "hvg": _Library(_path("PROSSTT_AMD_HVG_LIB", "libprosstt_amd_hvg.so"), "prosstt_amd_hvg.h", True, {
        "prosstt_amd_hvg_last_error": _text,
        "prosstt_amd_hvg_workspace_bytes": _int(i64, i64, _ptr_to(u64)),
        "prosstt_amd_hvg_clipped_sums": _int(vp, vp, i64, i64, i64, vp, vp, u64, vp, vp, vp, vp),
        "prosstt_amd_hvg_normalized_moments": _int(vp, vp, i64, i64, i64, vp, vp, u64, vp, vp, vp),
        "prosstt_amd_hvg_gather_columns": _int(vp, vp, i64, i64, i64, vp, i64, vp, i64, vp),
    }, "prosstt_amd_hvg_last_error"),
    # spatial autocorrelation: sums over the edges of a cell graph of the log-normalised entries, and the smoothed matrix
    "autocorr": _Library(_path("PROSSTT_AMD_AUTOCORR_LIB", "libprosstt_amd_autocorr.so"), "prosstt_amd_autocorr.h", True, {
        "prosstt_amd_autocorr_last_error": _text,
        "prosstt_amd_autocorr_workspace_bytes": _int(i64, i64, i64, _ptr_to(u64)),
        "prosstt_amd_autocorr_gene_sums": _int(vp, vp, i64, i64, i64, vp, vp, vp, vp, vp, i64, vp, i64, i32, vp, u64, vp, vp, vp, vp, vp),
        "prosstt_amd_autocorr_smooth": _int(vp, vp, i64, i64, i64, vp, vp, vp, vp, vp, i64, i32, i32, vp, i64, vp),
    }, "prosstt_amd_autocorr_last_error"),
    # the count model's log-likelihood for several candidate (alpha, beta) per gene: what fit.count_model maximises
    "fit": _Library(_path("PROSSTT_AMD_FIT_LIB", "libprosstt_amd_fit.so"), "prosstt_amd_fit.h", True, {
        "prosstt_amd_fit_last_error": _text,
        "prosstt_amd_fit_workspace_bytes": _int(i64, i64, i64, _ptr_to(u64)),
        "prosstt_amd_fit_loglik": _int(vp, vp, i64, i64, i64, vp, vp, i64, vp, i64, vp, vp, i64, vp, u64, vp, vp, vp, vp),
    }, "prosstt_amd_fit_last_error"),
    # expression trends: exact integer sums of the cells around every node of the lineage tree, by a node-by-cell weight matrix
    "trends": _Library(_path("PROSSTT_AMD_TRENDS_LIB", "libprosstt_amd_trends.so"), "prosstt_amd_trends.h", True, {
        "prosstt_amd_trends_last_error": _text,
        "prosstt_amd_trends_workspace_bytes": _int(i64, i64, i64, i64, _ptr_to(u64)),
        "prosstt_amd_trends_node_sums": _int(vp, vp, i64, i64, i64, vp, vp, vp, i64, i64, i64, vp, u64, vp, vp, vp),
    }, "prosstt_amd_trends_last_error"),
    # mapping of cells onto the tree: the Poisson score of every cell at every node by f32 MFMA, its argmax and log-sum-exps
    "mapping": _Library(_path("PROSSTT_AMD_MAPPING_LIB", "libprosstt_amd_mapping.so"), "prosstt_amd_mapping.h", True, {
        "prosstt_amd_mapping_last_error": _text,
        "prosstt_amd_mapping_workspace_bytes": _int(i64, i64, i64, i64, _ptr_to(u64)),
        "prosstt_amd_mapping_node_scores": _int(vp, vp, i64, i64, i64, vp, vp, i64, i64, vp, vp, vp, i64, i64, vp, u64, vp, vp,
                                                vp, vp, vp, vp),
        "prosstt_amd_mapping_node_scores_tiled": _int(vp, vp, i64, i64, i64, vp, vp, i64, i64, vp, vp, vp, i64, i64, i32, vp, u64,
                                                      vp, vp, vp, vp, vp, vp),
    }, "prosstt_amd_mapping_last_error"),
    # principal tree: squared distances to the centres, the soft or hard assignment with its per-node sums, the projection
    "ptree": _Library(_path("PROSSTT_AMD_PTREE_LIB", "libprosstt_amd_ptree.so"), "prosstt_amd_ptree.h", True, {
        "prosstt_amd_ptree_last_error": _text,
        "prosstt_amd_ptree_workspace_bytes": _int(i64, i64, i64, i32, _ptr_to(u64)),
        "prosstt_amd_ptree_assign": _int(vp, vp, i64, i64, i64, vp, i64, i64, f64, vp, u64, vp, vp, vp, vp, vp, vp, vp),
        "prosstt_amd_ptree_project": _int(vp, vp, i64, i64, i64, vp, i64, i64, vp, i64, vp, vp, vp, vp),
    }, "prosstt_amd_ptree_last_error"),
}

# Every library added after tests/test_guard.py pinned the union of the three tables above to the rows of
# tests/test_gpu_guard_bands.py (its census: one guard-band row per library, in a test file that no later change may edit)
# goes HERE.  Rows of the same shape, looked up after the other three tables.  Every library in this table brings its own
# guard-band test file (tests/test_gpu_<name>_guard_bands.py, on tests/guard.py as the shared file uses it);
# tests/test_native_newer.py checks each row against its header, its makefile row and the built library, takes the symbol count
# from the header, and checks that the four tables do not overlap and that each row's guard-band file is there.
NEWER_LIBRARIES = {
    # regression of the count model on a design: per gene the quasi-score, the information or the meat, and the
    # quasi-log-likelihood, what regress.regression iterates on
    "regress": _Library(_path("PROSSTT_AMD_REGRESS_LIB", "libprosstt_amd_regress.so"), "prosstt_amd_regress.h", True, {
        "prosstt_amd_regress_last_error": _text,
        "prosstt_amd_regress_workspace_bytes": _int(i64, i64, i64, _ptr_to(u64)),
        "prosstt_amd_regress_normal_equations": _int(vp, vp, i64, i64, i64, vp, vp, i64, vp, i64, i64, vp, vp, vp, i32, i32, vp,
                                                     u64, vp, vp, vp, vp, vp),
    }, "prosstt_amd_regress_last_error"),
    # scores against the simulated truth: exact sign and tree-distance sums over all pairs of cells, per pair of true classes
    "evaluate": _Library(_path("PROSSTT_AMD_EVALUATE_LIB", "libprosstt_amd_evaluate.so"), "prosstt_amd_evaluate.h", True, {
        "prosstt_amd_evaluate_last_error": _text,
        "prosstt_amd_evaluate_workspace_bytes": _int(i64, i32, i32, _ptr_to(u64)),
        "prosstt_amd_evaluate_pair_counts": _int(vp, vp, vp, vp, i64, i32, i32, vp, u64, vp, vp),
        "prosstt_amd_evaluate_pair_moments": _int(vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, vp, u64, vp, vp),
    }, "prosstt_amd_evaluate_last_error"),
    # GLM-PCA factors: per cell the quasi-score, the information and the quasi-log-likelihood of its regression on the genes'
    # loadings, the half of factors.glmpca's round that regress cannot do without transposing the matrix
    "factors": _Library(_path("PROSSTT_AMD_FACTORS_LIB", "libprosstt_amd_factors.so"), "prosstt_amd_factors.h", True, {
        "prosstt_amd_factors_last_error": _text,
        "prosstt_amd_factors_gene_blocking": _int(i64, i64, _ptr_to(i64)),
        "prosstt_amd_factors_workspace_bytes": _int(i64, i64, i64, i64, _ptr_to(u64)),
        "prosstt_amd_factors_cell_equations": _int(vp, vp, i64, i64, i64, vp, vp, vp, i64, i64, vp, vp, vp, i32, i64, vp, u64,
                                                   vp, vp, vp, vp, vp),
    }, "prosstt_amd_factors_last_error"),
    # binomial thinning: the part [lo, hi) of every count by THIN-1, a pure function of (seed, cell, gene), and its complement;
    # what thin.split, thin.fold and thin.downsample are made of
    "thin": _Library(_path("PROSSTT_AMD_THIN_LIB", "libprosstt_amd_thin.so"), "prosstt_amd_thin.h", True, {
        "prosstt_amd_thin_last_error": _text,
        "prosstt_amd_thin_plan": _int(i64, i64, vp, i64, vp, i64, vp, i64, _ptr_to(i32), _ptr_to(i64), _ptr_to(i64), _ptr_to(i64)),
        "prosstt_amd_thin_interval": _int(vp, vp, i64, i64, i64, u64, vp, i64, i64, u32, u32, vp, vp, vp, i64, vp, i64, vp),
    }, "prosstt_amd_thin_last_error"),
}


# Entry points of the sampler library declared after tests/test_native_libraries.py pinned its census of prosstt_amd.h:
# (their header, symbol -> prototype), declared by ``load`` beside the sampler's row; tests/test_strip_plan_host.py checks
# them against the header and the built library.
SAMPLER_LATER = ("prosstt_amd_plan.h", {
    "prosstt_amd_strip_plan": _int(i64, i32, i32, i32, i32, vp, _ptr_to(i32), _ptr_to(i32), _ptr_to(i32)),
    "prosstt_amd_last_strip_plan": _int(vp, vp, _ptr_to(i32), _ptr_to(i32), _ptr_to(i32)),
})


def _library(name):
    for table in (LIBRARIES, ADDED_LIBRARIES, LATER_LIBRARIES):
        if name in table:
            return table[name]
    return NEWER_LIBRARIES[name]


class NativeError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("prosstt_amd error %d: %s" % (code, message))
        self.code = code


_loaded = {}
_lock = threading.Lock()


def load(name="sampler"):
    """The library ``name`` of LIBRARIES, ADDED_LIBRARIES, LATER_LIBRARIES or NEWER_LIBRARIES with its prototypes declared (loaded
    once).  Raises if it has not been built."""
    lib = _library(name)
    with _lock:
        if name not in _loaded:
            if not os.path.exists(lib.path):
                raise RuntimeError("%s not found: build it with `make -C prosstt_amd/csrc %s` (or "
                                   "`python -c 'import __graft_entry__ as g; g.build()'`)%s"
                                   % (lib.path, name, ". prosstt_amd has no CPU fallback." if lib.hip else ""))
            if lib.hip:
                # torch first: it bundles its own libamdhip64.so.7, and the dynamic loader shares one
                # copy per SONAME.  Loading ours first would bind torch to /opt/rocm's runtime instead;
                # either way both must sit on ONE HIP runtime for streams and device pointers to be
                # exchangeable, and torch's own is the combination the wheel was built against.
                import torch  # noqa: F401
            L = ctypes.CDLL(lib.path)
            symbols = dict(lib.symbols, **SAMPLER_LATER[1]) if name == "sampler" else lib.symbols
            for symbol, (restype, argtypes) in symbols.items():
                fn = getattr(L, symbol)
                fn.restype = restype
                if argtypes is not None:
                    fn.argtypes = argtypes
            _loaded[name] = L
        return _loaded[name]


def check(code, name="sampler"):
    """Raise with the message of library ``name`` unless ``code`` is OK: NativeError, or ValueError for EDOMAIN (a code
    of the sampler's ABI alone)."""
    if code != OK:
        msg = getattr(load(name), _library(name).last_error)().decode("utf-8", "replace")
        if code == EDOMAIN:
            raise ValueError(msg)          # what scipy raises in the reference (simulation.py:647)
        raise NativeError(code, msg)


def device_count():
    n = ctypes.c_int(0)
    rc = load().prosstt_amd_device_count(ctypes.byref(n))
    return n.value if rc == OK else 0
