"""ctypes binding of libnumbskull_amd.so (the C-ABI declared in include/numbskull_amd.h).

There is no CPU fallback: if the shared library is missing the import of any compute path fails
loudly with build instructions, and if no MI355X is visible ``nsk_graph_create`` returns
NSK_E_DEVICE, raised here as RuntimeError.
"""

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NSK_LIB") or os.path.join(_HERE, "libnumbskull_amd.so")   # NSK_LIB: ablation builds (tools/)

OK, E_INVALID, E_FACTOR_FUNC, E_INDEX, E_DEVICE, E_RANGE, E_NOMEM = 0, -1, -2, -3, -4, -5, -6
FLAG_HEAD_BY_VID = 1
FLAG_PARTITION = 2
SCAN_CHROMATIC, SCAN_SEQUENTIAL = 0, 1
BUF_VALUE, BUF_VALUE_EVID, BUF_WEIGHT, BUF_SEND, BUF_RECV, BUF_SEND_EVID, BUF_RECV_EVID = range(7)

# every symbol include/numbskull_amd.h declares (tests/test_cabi.py checks the export list)
SYMBOLS = (
    "nsk_graph_create", "nsk_graph_destroy", "nsk_state_upload", "nsk_state_download",
    "nsk_set_seed", "nsk_set_rng_tag", "nsk_set_scan", "nsk_set_learn_cap", "nsk_set_learn_lag", "nsk_gibbs_sweeps", "nsk_learn_sweeps", "nsk_graph_get_info",
    "nsk_graph_get_colors", "nsk_graph_get_layout", "nsk_graph_get_generators", "nsk_graph_get_weight_slots", "nsk_graph_plan", "nsk_graph_plan_needs", "nsk_graph_plan_routes", "nsk_graph_get_routes", "nsk_graph_plan_classes", "nsk_profile_begin", "nsk_profile_end", "nsk_device_buffer",
    "nsk_set_stream", "nsk_synchronize", "nsk_ghost_needs", "nsk_exchange_setup", "nsk_exchange_pack",
    "nsk_exchange_unpack", "nsk_comm_unique_id", "nsk_comm_init", "nsk_gibbs_sweeps_exchange",
    "nsk_learn_sweeps_exchange", "nsk_pf_setup", "nsk_p2p_setup", "nsk_p2p_export", "nsk_p2p_import", "nsk_p2p_import_local",
    "nsk_gibbs_sweeps_p2p", "nsk_learn_sweeps_p2p", "nsk_p2p_exchange", "nsk_p2p_selftest", "nsk_p2p_fuse", "nsk_p2p_check", "nsk_p2p_reset", "nsk_profile_mark", "nsk_profile_read", "nsk_graph_order", "nsk_comm_volume", "nsk_graph_partition", "nsk_compute_var_map", "nsk_state_layout", "nsk_parse_factors", "nsk_parse_domains", "nsk_write_probabilities",
    "nsk_set_chains", "nsk_get_chains", "nsk_chains_upload", "nsk_chains_download",
    "nsk_trace_setup", "nsk_trace_rows", "nsk_trace_download", "nsk_trace_clear",
    "nsk_log_potential", "nsk_factor_values", "nsk_trace_log_potential", "nsk_trace_download_log_potential",
    "nsk_weight_stats", "nsk_trace_weight_stats", "nsk_trace_download_weight_stats",
    "nsk_conditionals", "nsk_trace_conditionals", "nsk_trace_download_conditionals", "nsk_icm", "nsk_tempered_sweeps",
    "nsk_smc_sweeps", "nsk_pt_sweeps", "nsk_pl_gradient", "nsk_mple_steps", "nsk_weight_moments", "nsk_pcd_steps", "nsk_pcd_latent_steps",
    "nsk_bp_setup", "nsk_bp_layout", "nsk_bp_run", "nsk_bp_beliefs", "nsk_bp_download", "nsk_bp_clear",
    "nsk_bp_refresh", "nsk_bp_moments", "nsk_bp_learn_steps", "nsk_bp_select", "nsk_bp_selected", "nsk_bp_latent_steps",
    "nsk_trace_ess", "nsk_trace_autocov_counts", "nsk_trace_pair_counts",
    "nsk_trace_value_autocov_counts", "nsk_trace_value_ess", "nsk_trace_value_pair_counts",
    "nsk_selftest_exp", "nsk_selftest_philox", "nsk_selftest_stream", "nsk_device_count", "nsk_last_error", "nsk_version",
)


class GraphDesc(C.Structure):
    _fields_ = [("nweight", C.c_int64), ("nvar", C.c_int64), ("nfactor", C.c_int64),
                ("nedge", C.c_int64), ("nvtf", C.c_int64), ("nfactor_index", C.c_int64),
                ("weight", C.c_void_p), ("variable", C.c_void_p), ("factor", C.c_void_p),
                ("fmap", C.c_void_p), ("vmap", C.c_void_p), ("factor_index", C.c_void_p),
                ("flags", C.c_int32), ("device", C.c_int32),
                ("own_begin", C.c_int64), ("own_end", C.c_int64)]


class GraphInfo(C.Structure):
    _fields_ = [("nvar", C.c_int64), ("nowned", C.c_int64), ("ncolors", C.c_int64),
                ("value_bytes", C.c_int64), ("device_bytes", C.c_int64),
                ("nfast", C.c_int64), ("ngeneric", C.c_int64),
                ("alg_bytes_inference", C.c_double), ("alg_bytes_learning", C.c_double),
                ("sweeps_done", C.c_int64), ("layout_bytes_inference", C.c_double),
                ("layout_bytes_learning", C.c_double), ("ztab_entries", C.c_int64),
                ("compile_seconds", C.c_double), ("learn_cap", C.c_double),
                ("learn_clipped", C.c_int64), ("grad_shift", C.c_int64),
                ("acc_copies", C.c_int64), ("learn_lag", C.c_int64), ("direct_weights", C.c_int64),
                ("weight_slots", C.c_int64), ("layout_hash", C.c_int64), ("p2p_fused", C.c_int64),
                ("tab_quads", C.c_int64), ("wide_quads", C.c_int64),
                ("hubs", C.c_int64), ("hubs_ep", C.c_int64), ("hubs_block", C.c_int64),
                ("tiles_shape", C.c_int64), ("tiles_shape_padded", C.c_int64), ("tiles_lane", C.c_int64),
                ("tiles_general", C.c_int64), ("tiles_general_roles", C.c_int64),
                ("ep_groups", C.c_int64), ("ep_groups_two_pass", C.c_int64)]


class BpInfo(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("nfactor", "nedges", "ntable", "nmsg", "nfree", "nisolated", "nclamped",
                                         "nbelief", "max_table", "device_bytes")]


# belief propagation (include/numbskull_amd.h): the caps of a factor, what nsk_bp_download hands out, and the grids of its
# launches (csrc/nsk_bp.hip bp_blocks): one item a lane, blocks of BP_BLOCK lanes (BP_VAR_BLOCK in the variable phase),
# at most BP_MAX_BLOCKS -- or the diagnostic cap NSK_BP_GRID_CAP; more items loop
BP_MAX_MEMBERS, BP_MAX_TABLE = 16, 4096
BP_THETA, BP_FACTOR_BELIEFS, BP_F2V, BP_V2F = range(4)
BP_BLOCK, BP_VAR_BLOCK, BP_MAX_BLOCKS = 256, 128, 2048
BP_VAR_REG = 6          # a binary variable of at most this many edges is served from registers (csrc/nsk_kernels_bp.h)


def bp_trips(items, cap=0, block=BP_BLOCK):
    """Trips the lanes of a belief-propagation launch over ``items`` items make."""
    limit = min(BP_MAX_BLOCKS, int(cap)) if cap > 0 else BP_MAX_BLOCKS
    blocks = max(1, min((int(items) + block - 1) // block, limit))
    return (int(items) + blocks * block - 1) // (blocks * block)


# the launch of nsk_pl_gradient / nsk_mple_steps (csrc/nsk_kernels_plgrad.h nsk_plgrad_blocks): blocks of PLGRAD_BLOCK lanes
# per chain; one selected variable per lane up to PLGRAD_CU_BLOCKS blocks, then two per lane before the grid grows, at
# most PLGRAD_MAX_BLOCKS blocks -- a longer selection loops further; LDS bins up to PLGRAD_BINS weights
PLGRAD_BLOCK, PLGRAD_CU_BLOCKS, PLGRAD_MAX_BLOCKS, PLGRAD_BINS = 256, 256, 2048, 256


def plgrad_blocks(nsel):
    """Blocks per chain of the gradient launch for a selection of ``nsel`` variables with a position."""
    one = (int(nsel) + PLGRAD_BLOCK - 1) // PLGRAD_BLOCK
    if one <= PLGRAD_CU_BLOCKS:
        return max(1, one)
    return max(PLGRAD_CU_BLOCKS, min(PLGRAD_MAX_BLOCKS, (one + 1) // 2))


# the launches of nsk_weight_moments / nsk_pcd_steps (csrc/nsk_kernels_pcd.h nsk_moments_blocks): one weight of at most
# MOMENTS_SHORT factors per lane, one piece of at most MOMENTS_PIECE factors of a longer one per wave, blocks of
# MOMENTS_BLOCK lanes in whole rounds of 8, at most MOMENTS_MAX_BLOCKS -- or the diagnostic cap NSK_MOMENTS_GRID_CAP,
# rounded down to a whole round but at least one; more items loop
MOMENTS_BLOCK, MOMENTS_SHORT, MOMENTS_PIECE, MOMENTS_MAX_BLOCKS = 256, 16, 2048, 2048


def moments_blocks(items, per_block, cap=0):
    """Blocks of a moment launch over ``items`` lanes' or waves' items, ``per_block`` of them a block and trip."""
    need = ((int(items) + per_block - 1) // per_block + 7) // 8 * 8
    limit = max(8, min(MOMENTS_MAX_BLOCKS, int(cap) // 8 * 8)) if cap > 0 else MOMENTS_MAX_BLOCKS
    return max(8, min(need, limit))


def moments_trips(items, per_block, cap=0):
    """Trips the lanes (``per_block`` = MOMENTS_BLOCK) or waves (MOMENTS_BLOCK // 64) of that launch make."""
    per_trip = moments_blocks(items, per_block, cap) * per_block
    return (int(items) + per_trip - 1) // per_trip


# the route word of nsk_graph_plan_routes / nsk_graph_get_routes (include/numbskull_amd.h "Routes")
ROUTE_NONE, ROUTE_TABLE, ROUTE_UNIFORM, ROUTE_SHAPE, ROUTE_LANE, ROUTE_GENERAL, ROUTE_GROUP, ROUTE_HUB, ROUTE_GENERIC = range(9)


def route_fields(r):
    """The fields of route words (an int or an array of them), by name."""
    return {"kind": r & 15, "own_entries": (r >> 4) & 31, "own_width": (r >> 9) & 7, "tile_entries": (r >> 12) & 31,
            "tile_width": (r >> 17) & 7, "two_pass": (r >> 20) & 1, "null_word": (r >> 21) & 1,
            "hub_ep": (r >> 22) & 1, "hub_block": (r >> 23) & 1}


# the class record of nsk_graph_plan_classes (include/numbskull_amd.h "Class plans"): CLASS_REC int32 per colour class
CLASS_REC = 48
CLASS_FIELDS = ("skip", "gen_on", "gen_items", "gen_grid", "gen_stream", "gen_ep", "gen_maxc", "gen_capped", "gen_tile0",
                "gen_ntiles", "gen_hblocks", "gen_gblocks", "gen_rblocks", "gen_nrest", "gen_behind", "gen_nblocks",
                "generic_on", "generic_n", "generic_grid", "generic_stream", "heavy_on", "heavy_n", "heavy_grid", "heavy_stream",
                "fast_on", "fast_n", "fast_grid", "fast_stream", "dyn_on", "dyn_n", "dyn_grid", "dyn_stream",
                "nhub", "nbh", "ngroups", "ndyn", "nlrest", "nrest", "ngeneric", "ntiles", "fb", "fe", "he", "e",
                "kstat", "update", "segments", "seg_tiles")
assert len(CLASS_FIELDS) == CLASS_REC


def class_fields(rec):
    """The fields of class records (one record, or an array of them: the last axis), by name."""
    rec = np.asarray(rec)
    return {k: rec[..., i] for i, k in enumerate(CLASS_FIELDS)}


_lib = None


def lib():
    """The loaded library; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "numbskull_amd: %s is missing. Build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()' or "
                "make -C numbskull_amd/csrc); there is no CPU fallback." % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.nsk_last_error.restype = C.c_char_p
        L.nsk_version.restype = C.c_char_p
        for name in SYMBOLS:
            if not hasattr(L, name):
                if not os.environ.get("NSK_LIB"):      # (an older ablation build under NSK_LIB may lack newer entry points)
                    raise AttributeError("libnumbskull_amd.so lacks %s: header and library disagree" % name)
                # a call of a missing entry point FAILS (it used to report success: an A/B run against
                # an older build then compared different semantics without saying so)
                def missing(*a, _name=name):
                    raise AttributeError("%s lacks %s (an older build under NSK_LIB)" % (LIB_PATH, _name))
                setattr(L, name, missing)
        L.nsk_gibbs_sweeps.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int]
        L.nsk_learn_sweeps.argtypes = [C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_int,
                                       C.c_double, C.c_int64, C.c_int]
        L.nsk_set_seed.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
        L.nsk_set_rng_tag.argtypes = [C.c_void_p, C.c_uint32]
        L.nsk_set_scan.argtypes = [C.c_void_p, C.c_int]
        L.nsk_set_learn_cap.argtypes = [C.c_void_p, C.c_double]
        L.nsk_set_learn_lag.argtypes = [C.c_void_p, C.c_int]
        L.nsk_state_upload.argtypes = [C.c_void_p] * 5
        L.nsk_state_download.argtypes = [C.c_void_p] * 5
        L.nsk_set_chains.argtypes = [C.c_void_p, C.c_int]
        L.nsk_get_chains.argtypes = [C.c_void_p]
        L.nsk_chains_upload.argtypes = [C.c_void_p] * 3
        L.nsk_chains_download.argtypes = [C.c_void_p] * 3
        L.nsk_trace_setup.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64]
        L.nsk_trace_rows.argtypes = [C.c_void_p] + [C.POINTER(C.c_int64)] * 3
        L.nsk_trace_download.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
        L.nsk_trace_clear.argtypes = [C.c_void_p]
        L.nsk_log_potential.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p]
        L.nsk_factor_values.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p]
        L.nsk_trace_log_potential.argtypes = [C.c_void_p, C.c_int]
        L.nsk_trace_download_log_potential.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
        L.nsk_weight_stats.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_void_p]
        L.nsk_trace_weight_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int]
        L.nsk_trace_download_weight_stats.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
        L.nsk_conditionals.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
        L.nsk_trace_conditionals.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.nsk_trace_download_conditionals.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
        L.nsk_icm.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
        L.nsk_bp_setup.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.POINTER(BpInfo)]
        L.nsk_bp_layout.argtypes = [C.c_void_p] * 5
        L.nsk_bp_run.argtypes = [C.c_void_p, C.c_int64, C.c_double, C.c_double, C.POINTER(C.c_int64), C.c_void_p]
        L.nsk_bp_beliefs.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.nsk_bp_download.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.nsk_bp_clear.argtypes = [C.c_void_p]
        L.nsk_bp_refresh.argtypes = [C.c_void_p]
        L.nsk_bp_moments.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
        L.nsk_bp_learn_steps.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_double, C.c_double, C.c_int, C.c_double,
                                         C.c_double, C.c_double, C.c_int] + [C.c_void_p] * 5
        L.nsk_bp_select.argtypes = [C.c_void_p, C.c_int]
        L.nsk_bp_selected.argtypes = [C.c_void_p]
        L.nsk_bp_latent_steps.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_double, C.c_double, C.c_int, C.c_double,
                                          C.c_double, C.c_double, C.c_int] + [C.c_void_p] * 5
        L.nsk_pl_gradient.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 3
        L.nsk_mple_steps.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64,
                                     C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
        L.nsk_weight_moments.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p]
        L.nsk_pcd_steps.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_double, C.c_double, C.c_double,
                                    C.c_int, C.c_void_p, C.c_void_p]
        L.nsk_pcd_latent_steps.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_double, C.c_double,
                                           C.c_double, C.c_int, C.c_void_p, C.c_void_p]
        L.nsk_tempered_sweeps.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int] + [C.c_void_p] * 4
        L.nsk_smc_sweeps.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_double] + [C.c_void_p] * 6
        L.nsk_pt_sweeps.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.nsk_trace_ess.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64] + [C.c_void_p] * 4
        L.nsk_trace_autocov_counts.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
        L.nsk_trace_pair_counts.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
        L.nsk_trace_value_autocov_counts.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
        L.nsk_trace_value_ess.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 4
        L.nsk_trace_value_pair_counts.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
        L.nsk_graph_create.argtypes = [C.POINTER(GraphDesc), C.POINTER(C.c_void_p)]
        L.nsk_graph_destroy.argtypes = [C.c_void_p]
        L.nsk_graph_get_info.argtypes = [C.c_void_p, C.POINTER(GraphInfo)]
        L.nsk_graph_get_colors.argtypes = [C.c_void_p, C.c_void_p]
        L.nsk_graph_get_layout.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
        L.nsk_graph_get_generators.argtypes = [C.c_void_p, C.c_void_p]
        L.nsk_graph_get_weight_slots.argtypes = [C.c_void_p, C.c_void_p]
        L.nsk_graph_plan.argtypes = [C.POINTER(GraphDesc), C.c_void_p, C.POINTER(GraphInfo)]
        L.nsk_graph_plan_needs.argtypes = [C.POINTER(GraphDesc), C.POINTER(C.c_int64), C.c_void_p]
        L.nsk_graph_plan_routes.argtypes = [C.POINTER(GraphDesc), C.c_void_p]
        L.nsk_graph_get_routes.argtypes = [C.c_void_p, C.c_void_p]
        L.nsk_graph_plan_classes.argtypes = [C.POINTER(GraphDesc), C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int64)]
        L.nsk_profile_begin.argtypes = [C.c_void_p]
        L.nsk_profile_end.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
        L.nsk_device_buffer.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p),
                                        C.POINTER(C.c_int64)]
        L.nsk_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.nsk_synchronize.argtypes = [C.c_void_p]
        L.nsk_ghost_needs.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]
        L.nsk_exchange_setup.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                         C.c_void_p, C.c_int64]
        L.nsk_exchange_pack.argtypes = [C.c_void_p, C.c_int]
        L.nsk_exchange_unpack.argtypes = [C.c_void_p, C.c_int]
        L.nsk_comm_unique_id.argtypes = [C.c_char_p, C.c_void_p]
        L.nsk_comm_init.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_char_p]
        L.nsk_gibbs_sweeps_exchange.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int]
        L.nsk_learn_sweeps_exchange.argtypes = [C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_int,
                                                C.c_double, C.c_int64, C.c_int]
        L.nsk_pf_setup.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.nsk_p2p_setup.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6
        L.nsk_p2p_export.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        L.nsk_p2p_import.argtypes = [C.c_void_p, C.c_void_p]
        L.nsk_p2p_import_local.argtypes = [C.c_void_p, C.c_void_p]
        L.nsk_gibbs_sweeps_p2p.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int]
        L.nsk_learn_sweeps_p2p.argtypes = [C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_int,
                                           C.c_double, C.c_int64, C.c_int]
        L.nsk_p2p_exchange.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.nsk_p2p_selftest.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.nsk_p2p_fuse.argtypes = [C.c_void_p, C.c_int]
        L.nsk_p2p_check.argtypes = [C.c_void_p]
        L.nsk_p2p_reset.argtypes = [C.c_void_p]
        L.nsk_profile_mark.argtypes = [C.c_void_p]
        L.nsk_profile_read.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
        L.nsk_graph_order.argtypes = [C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p,
                                      C.c_void_p, C.POINTER(C.c_int64)]
        L.nsk_comm_volume.argtypes = [C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int,
                                      C.POINTER(C.c_int64)]
        L.nsk_graph_partition.argtypes = [C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_uint64,
                                          C.c_void_p, C.c_void_p, C.c_void_p]
        L.nsk_compute_var_map.argtypes = [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                          C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_int64]
        L.nsk_state_layout.argtypes = [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.nsk_parse_factors.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.nsk_parse_domains.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                        C.c_void_p, C.c_int64]
        L.nsk_write_probabilities.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                              C.c_void_p, C.c_void_p, C.c_int64, C.c_double]
        L.nsk_device_count.argtypes = [C.POINTER(C.c_int)]
        L.nsk_selftest_exp.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int64]
        L.nsk_selftest_stream.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.nsk_selftest_philox.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int64,
                                          C.c_void_p]
        _lib = L
    return _lib


_EXC = {E_FACTOR_FUNC: NotImplementedError, E_INDEX: IndexError, E_RANGE: OverflowError,
        E_NOMEM: MemoryError, E_INVALID: ValueError, E_DEVICE: RuntimeError}


def check(rc):
    """Map a C-ABI status to the exception the reference would raise."""
    if rc == OK:
        return
    msg = lib().nsk_last_error().decode("utf-8", "replace")
    raise _EXC.get(rc, RuntimeError)(msg or "numbskull_amd error %d" % rc)


def ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)


def device_count():
    n = C.c_int(0)
    rc = lib().nsk_device_count(C.byref(n))
    return n.value if rc == OK else 0


def as_c(a, dtype=None):
    """C-contiguous view/copy of ``a`` (record arrays keep their packed dtype)."""
    return np.ascontiguousarray(a, dtype)
