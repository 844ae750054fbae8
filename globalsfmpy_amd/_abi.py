"""ctypes mirror of include/gsfm_rot.h (the C-ABI drop-in boundary).

The shared library is the product: if libgsfm_rot.so is missing or does not load,
importing the solver fails loudly -- there is no CPU fallback.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GSFM_ROT_LIB") or os.path.join(_HERE, "libgsfm_rot.so")  # override: A/B builds of the kernels (tools/)

# gsfm_status
OK, ERR_INVALID_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_EMPTY, ERR_COMM, ERR_UNSUPPORTED = range(7)

# gsfm_rot_error_type == RotationErrorType (reference include/pairwise_rotation_error_quat.hpp:50-61)
QUATERNION_NORM = 0
ROTATION_MAT_FNORM = 1
QUATERNION_COSINE = 2
ANGLE_AXIS_COVARIANCE = 3
ANGLE_AXIS = 4
ANGLE_AXIS_INLIERS = 5
ANGLE_AXIS_COV_INLIERS = 6
ANGLE_AXIS_COVTRACE = 7
ANGLE_AXIS_COVNORM = 8

# gsfm_loss_kind
LOSS_TRIVIAL, LOSS_HUBER, LOSS_SOFT_L1, LOSS_CAUCHY, LOSS_ARCTAN, LOSS_TOLERANT, LOSS_TUKEY, \
    LOSS_LONE_HALF, LOSS_LTWO, LOSS_GEMAN_MCCLURE, LOSS_MAGSAC = range(11)
LOSS_OP_SCALE, LOSS_OP_PUSH_ARG, LOSS_OP_COMPOSE = 32, 33, 34
LOSS_MAX_NODES = 16

TERMINATION_NAMES = ["FUNCTION_TOLERANCE", "GRADIENT_TOLERANCE", "PARAMETER_TOLERANCE", "NO_CONVERGENCE", "FAILURE"]


class LossNode(C.Structure):
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("p", C.c_double * 3)]


class Options(C.Structure):
    _fields_ = [
        ("max_num_iterations", C.c_int32), ("num_threads", C.c_int32),
        ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double),
        ("parameter_tolerance", C.c_double), ("initial_trust_region_radius", C.c_double),
        ("max_trust_region_radius", C.c_double), ("min_trust_region_radius", C.c_double),
        ("min_relative_decrease", C.c_double), ("min_lm_diagonal", C.c_double),
        ("max_lm_diagonal", C.c_double), ("jacobi_scaling", C.c_int32),
        ("max_cg_iterations", C.c_int32), ("cg_relative_tolerance", C.c_double),
        ("cg_check_interval", C.c_int32), ("verbose", C.c_int32),
        ("pcg_single_reduction", C.c_int32), ("cg_stall_iterations", C.c_int32),
        ("dense_cholesky_max_cams", C.c_int32), ("pcg_hip_graph", C.c_int32),
        ("pcg_forcing", C.c_int32), ("dense_cholesky_auto_cams", C.c_int32), ("pcg_forcing_tolerance", C.c_double),
        ("lm_device_control", C.c_int32), ("component_rest", C.c_int32),
    ]


class Summary(C.Structure):
    _fields_ = [
        ("termination", C.c_int32), ("num_iterations", C.c_int32),
        ("num_successful_steps", C.c_int32), ("num_unsuccessful_steps", C.c_int32),
        ("num_residual_sweeps", C.c_int32), ("num_linearizations", C.c_int32),
        ("num_cg_iterations", C.c_int32), ("iters_to_1e6", C.c_int32),
        ("nonfinite", C.c_int32), ("outer_iterations", C.c_int32),
        ("num_edges_used", C.c_uint64),
        ("initial_cost", C.c_double), ("final_cost", C.c_double),
        ("final_gradient_max_norm", C.c_double), ("final_radius", C.c_double),
        ("last_weight_change", C.c_double),
        ("t_total_ms", C.c_double), ("t_linearize_ms", C.c_double),
        ("t_sweep_ms", C.c_double), ("t_cg_ms", C.c_double),
        ("num_dense_solves", C.c_int32), ("num_graph_launches", C.c_int32),
        ("num_collectives", C.c_int32), ("num_pcg_collectives", C.c_int32),
        ("num_pcg_launched", C.c_int32), ("num_forcing_refinements", C.c_int32),
        ("num_inexact_steps", C.c_int32), ("num_pcg_capped_steps", C.c_int32),
        ("worst_accepted_cg_residual", C.c_double), ("num_forcing_restarts", C.c_int32), ("reserved_", C.c_int32),
    ]

    def as_dict(self):
        d = {name: getattr(self, name) for name, _ in self._fields_}
        d["termination_name"] = TERMINATION_NAMES[self.termination] if 0 <= self.termination < 5 else "?"
        return d


class StepInfo(C.Structure):
    """gsfm_rot_step_info (gsfm_rot_step_check, a testing aid)"""
    _fields_ = [
        ("path", C.c_int32), ("cg_iterations", C.c_int32), ("loose_cg_iterations", C.c_int32), ("coarse_n", C.c_int32),
        ("lin_is_lap", C.c_int32), ("column_sorted", C.c_int32), ("graph_launches", C.c_int32), ("dense_info", C.c_int32),
        ("cg_rel", C.c_double), ("loose_cg_rel", C.c_double), ("cg_tolerance", C.c_double), ("gmax", C.c_double), ("cost", C.c_double),
        ("step_sums", C.c_double * 5),
    ]


STEP_DENSE, STEP_PCG_TEXTBOOK, STEP_PCG_SINGLE_REDUCTION, STEP_COMPONENTS = range(4)


class PosOptions(C.Structure):
    """gsfm_pos_options (include/gsfm_pos.h)"""
    _fields_ = [
        ("max_num_iterations", C.c_int32), ("jacobi_scaling", C.c_int32),
        ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double),
        ("parameter_tolerance", C.c_double), ("initial_trust_region_radius", C.c_double),
        ("max_trust_region_radius", C.c_double), ("min_trust_region_radius", C.c_double),
        ("min_relative_decrease", C.c_double), ("min_lm_diagonal", C.c_double),
        ("max_lm_diagonal", C.c_double), ("dense_max_cams", C.c_int32),
        ("max_cg_iterations", C.c_int32), ("cg_relative_tolerance", C.c_double),
        ("cg_check_interval", C.c_int32), ("cg_stall_iterations", C.c_int32),
        ("remove_scale_gauge", C.c_int32), ("verbose", C.c_int32),
    ]


class PosSummary(C.Structure):
    """gsfm_pos_summary (include/gsfm_pos.h)"""
    _fields_ = [
        ("termination", C.c_int32), ("num_iterations", C.c_int32),
        ("num_successful_steps", C.c_int32), ("num_unsuccessful_steps", C.c_int32),
        ("num_cg_iterations", C.c_int32), ("num_dense_solves", C.c_int32),
        ("num_pcg_stalled_steps", C.c_int32), ("num_residual_sweeps", C.c_int32),
        ("num_linearizations", C.c_int32), ("nonfinite", C.c_int32),
        ("num_edges_used", C.c_uint64),
        ("initial_cost", C.c_double), ("final_cost", C.c_double),
        ("final_gradient_max_norm", C.c_double), ("final_radius", C.c_double),
        ("max_radius", C.c_double), ("t_total_ms", C.c_double),
    ]

    def as_dict(self):
        d = {name: getattr(self, name) for name, _ in self._fields_}
        d["termination_name"] = TERMINATION_NAMES[self.termination] if 0 <= self.termination < 5 else "?"
        return d


class PospSummary(C.Structure):
    """gsfm_posp_summary (include/gsfm_posp.h)"""
    _fields_ = [("pos", PosSummary), ("num_observations_used", C.c_uint64), ("num_active_points", C.c_uint64)]

    def as_dict(self):
        d = self.pos.as_dict()
        d["num_observations_used"] = self.num_observations_used
        d["num_active_points"] = self.num_active_points
        return d


class BaOptions(C.Structure):
    """gsfm_ba_options (include/gsfm_ba.h)"""
    _fields_ = [
        ("max_num_iterations", C.c_int32), ("jacobi_scaling", C.c_int32),
        ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double),
        ("parameter_tolerance", C.c_double), ("initial_trust_region_radius", C.c_double),
        ("max_trust_region_radius", C.c_double), ("min_trust_region_radius", C.c_double),
        ("min_relative_decrease", C.c_double), ("min_lm_diagonal", C.c_double),
        ("max_lm_diagonal", C.c_double), ("max_cg_iterations", C.c_int32),
        ("cg_check_interval", C.c_int32), ("cg_relative_tolerance", C.c_double),
        ("cg_stall_iterations", C.c_int32), ("remove_gauge", C.c_int32),
        ("verbose", C.c_int32), ("reserved_", C.c_int32),
    ]


class BaSummary(C.Structure):
    """gsfm_ba_summary (include/gsfm_ba.h)"""
    _fields_ = [
        ("termination", C.c_int32), ("num_iterations", C.c_int32),
        ("num_successful_steps", C.c_int32), ("num_unsuccessful_steps", C.c_int32),
        ("num_cg_iterations", C.c_int32), ("num_pcg_stalled_steps", C.c_int32),
        ("num_residual_sweeps", C.c_int32), ("num_linearizations", C.c_int32),
        ("nonfinite", C.c_int32), ("reserved_", C.c_int32),
        ("num_observations_used", C.c_uint64), ("num_active_cameras", C.c_uint64),
        ("num_active_points", C.c_uint64),
        ("initial_cost", C.c_double), ("final_cost", C.c_double),
        ("final_gradient_max_norm", C.c_double), ("final_radius", C.c_double),
        ("max_radius", C.c_double), ("t_total_ms", C.c_double),
    ]

    def as_dict(self):
        d = {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved_"}
        d["termination_name"] = TERMINATION_NAMES[self.termination] if 0 <= self.termination < 5 else "?"
        return d


ROT_L1L2_MAX_L1 = 8


class RotL1L2Options(C.Structure):
    """gsfm_rot_l1l2_options (include/gsfm_rot_l1l2.h)"""
    _fields_ = [
        ("max_num_l1_iterations", C.c_int32), ("max_num_irls_iterations", C.c_int32),
        ("l1_step_convergence_threshold", C.c_double), ("irls_step_convergence_threshold", C.c_double),
        ("irls_loss_parameter_sigma", C.c_double),
        ("admm_initial_iterations", C.c_int32), ("max_cg_iterations", C.c_int32),
        ("admm_rho", C.c_double), ("admm_alpha", C.c_double),
        ("admm_absolute_tolerance", C.c_double), ("admm_relative_tolerance", C.c_double),
        ("cg_relative_tolerance", C.c_double),
        ("cg_check_interval", C.c_int32), ("cg_stall_iterations", C.c_int32),
        ("verbose", C.c_int32), ("reserved_", C.c_int32),
    ]


class RotL1L2Summary(C.Structure):
    """gsfm_rot_l1l2_summary (include/gsfm_rot_l1l2.h)"""
    _fields_ = [
        ("num_l1_iterations", C.c_int32), ("num_admm_iterations", C.c_int32 * ROT_L1L2_MAX_L1),
        ("num_irls_iterations", C.c_int32), ("l1_converged", C.c_int32), ("irls_converged", C.c_int32),
        ("num_cg_iterations", C.c_int32), ("num_linear_solves", C.c_int32), ("num_pcg_stalled_solves", C.c_int32),
        ("nonfinite", C.c_int32),
        ("num_edges_used", C.c_uint64),
        ("l1_step", C.c_double * ROT_L1L2_MAX_L1), ("last_irls_step", C.c_double),
        ("worst_accepted_cg_residual", C.c_double), ("t_total_ms", C.c_double), ("kernel_ms", C.c_double),
    ]

    def as_dict(self):
        d = {name: getattr(self, name) for name, _ in self._fields_}
        n = min(self.num_l1_iterations, ROT_L1L2_MAX_L1)
        d["num_admm_iterations"] = [int(v) for v in self.num_admm_iterations[:n]]
        d["l1_step"] = [float(v) for v in self.l1_step[:n]]
        return d


class TrackRefineOptions(C.Structure):
    """gsfm_tracks_refine_options (include/gsfm_tracks.h)"""
    _fields_ = [
        ("refine", C.c_int32), ("max_num_iterations", C.c_int32),
        ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double),
        ("parameter_tolerance", C.c_double), ("min_relative_decrease", C.c_double),
        ("initial_trust_region_radius", C.c_double), ("max_trust_region_radius", C.c_double),
        ("min_trust_region_radius", C.c_double),
    ]


class TrackBuildOptions(C.Structure):
    """gsfm_tracks_build_options (include/gsfm_tracks.h)"""
    _fields_ = [("min_track_length", C.c_int32), ("max_track_length", C.c_int32), ("hash_capacity_log2", C.c_int32)]


ALL_GATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
ALL_REDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
LOSS_CALLBACK_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_double, C.POINTER(C.c_double))


SHARD_CAPTURABLE = 1
SHARD_DISCONNECTED = 2


class Shard(C.Structure):
    _fields_ = [
        ("rank", C.c_int32), ("world_size", C.c_int32),
        ("slice_width", C.c_uint32), ("flags", C.c_uint32),
        ("ctx", C.c_void_p), ("all_gather", ALL_GATHER_FN), ("all_reduce_sum", ALL_REDUCE_FN),
    ]


def make_program(nodes):
    """nodes: list of (kind, p0, p1, p2) -> (LossNode array, n)."""
    n = len(nodes)
    if n > LOSS_MAX_NODES:
        raise ValueError("loss program too long (%d > %d nodes)" % (n, LOSS_MAX_NODES))
    arr = (LossNode * max(n, 1))()
    for k, nd in enumerate(nodes):
        arr[k].kind = int(nd[0])
        arr[k].reserved = 0
        ps = list(nd[1:]) + [0.0] * (3 - len(nd[1:]))
        for c in range(3):
            arr[k].p[c] = float(ps[c])
    return arr, n


_DP = C.POINTER(C.c_double)
_U32P = C.POINTER(C.c_uint32)


def declare_solver_signatures(lib, prefix, problem_ptr=C.c_void_p):
    """Shared by the product library (prefix 'gsfm_rot_') and the oracle (prefix 'orc_'):
    the oracle deliberately mirrors the product's argument lists."""
    f = getattr(lib, prefix + "set_loss")
    f.argtypes = [problem_ptr, C.POINTER(LossNode), C.c_int32]; f.restype = C.c_int
    f = getattr(lib, prefix + "set_loss_callback")
    f.argtypes = [problem_ptr, LOSS_CALLBACK_FN, C.c_void_p]; f.restype = C.c_int
    f = getattr(lib, prefix + "set_edge_weights")
    f.argtypes = [problem_ptr, _DP]; f.restype = C.c_int
    f = getattr(lib, prefix + "residuals")
    f.argtypes = [problem_ptr, _DP, _DP, _DP, _DP, _DP]; f.restype = C.c_int
    f = getattr(lib, prefix + "linearize")
    f.argtypes = [problem_ptr, _DP, _DP, _DP, _DP]; f.restype = C.c_int
    f = getattr(lib, prefix + "normal_matvec")
    f.argtypes = [problem_ptr, _DP, _DP]; f.restype = C.c_int
    f = getattr(lib, prefix + "solve")
    f.argtypes = [problem_ptr, _DP, C.POINTER(Options), C.POINTER(Summary)]; f.restype = C.c_int
    f = getattr(lib, prefix + "solve_sigma_consensus")
    f.argtypes = [problem_ptr, _DP, C.c_int32, C.c_double, C.POINTER(Options), C.POINTER(Summary)]; f.restype = C.c_int
    f = getattr(lib, prefix + "get_trace")
    f.argtypes = [problem_ptr, _DP, C.c_int32]; f.restype = C.c_int32
    f = getattr(lib, prefix + "problem_destroy")
    f.argtypes = [problem_ptr]; f.restype = None


_lib = None


def preload_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so (soname libamdhip64.so.7) next to libtorch.  If the system
    runtime under /opt/rocm is mapped first (by libgsfm_rot.so) and torch is imported afterwards, torch maps its own copy
    as well, and the runtime that initialises second finds no device (measured on the MI355X box: `hipGetDeviceCount`
    fails in libgsfm_rot.so after `torch.cuda.is_available()`).  The other order is fine because the loader matches
    libgsfm_rot.so's NEEDED libamdhip64.so.7 against the soname of torch's copy.  So: when torch is installed and no HIP
    runtime is mapped yet, map torch's copy first.  torch itself is not imported.  Processes without torch (the C++
    consumers, scripts/sfm_pipeline.py) just get the system runtime."""
    try:
        with open("/proc/self/maps") as f:
            if "libamdhip64" in f.read():
                return None
    except OSError:
        pass
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return None
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if not os.path.exists(cand):
        return None
    C.CDLL(cand, mode=C.RTLD_GLOBAL)
    return cand


def load_library():
    """Load libgsfm_rot.so (built by __graft_entry__.build()). Fails loudly."""
    global _lib
    if _lib is not None:
        return _lib
    preload_hip_runtime()
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "globalsfmpy_amd: %s not found. The HIP extension is the product and has no CPU fallback; "
            "build it with `python -c 'import __graft_entry__ as g; g.build()'`." % LIB_PATH)
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    if lib.gsfm_rot_abi_version() != 4:
        raise ImportError("globalsfmpy_amd: ABI version mismatch in %s" % LIB_PATH)
    lib.gsfm_last_error.restype = C.c_char_p
    lib.gsfm_rot_options_default.argtypes = [C.POINTER(Options)]
    lib.gsfm_rot_problem_create.argtypes = [C.c_uint32, C.c_uint64, _U32P, _U32P, _DP, C.c_int32, _DP, _DP,
                                            C.POINTER(Shard), C.POINTER(C.c_void_p)]
    lib.gsfm_rot_problem_create.restype = C.c_int
    declare_solver_signatures(lib, "gsfm_rot_")
    lib.gsfm_rot_set_stream.argtypes = [C.c_void_p, C.c_void_p]; lib.gsfm_rot_set_stream.restype = C.c_int
    lib.gsfm_rot_solve_resident.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Options), C.POINTER(Summary)]; lib.gsfm_rot_solve_resident.restype = C.c_int
    lib.gsfm_rot_residual_dim.argtypes = [C.c_int32]; lib.gsfm_rot_residual_dim.restype = C.c_int32
    lib.gsfm_rot_time_sweep.argtypes = [C.c_void_p, _DP, C.c_int32, _DP]; lib.gsfm_rot_time_sweep.restype = C.c_int
    lib.gsfm_rot_time_kernels.argtypes = [C.c_void_p, _DP, C.c_int32, _DP]; lib.gsfm_rot_time_kernels.restype = C.c_int
    lib.gsfm_rot_time_sweep_variants.argtypes = [C.c_void_p, _DP, C.c_int32, _DP]; lib.gsfm_rot_time_sweep_variants.restype = C.c_int
    lib.gsfm_rot_matvec_bytes.argtypes = [C.c_void_p, _DP, _DP, C.POINTER(C.c_int32)]; lib.gsfm_rot_matvec_bytes.restype = C.c_int
    lib.gsfm_rot_sweep_bytes.argtypes = [C.c_void_p, _DP, _DP]; lib.gsfm_rot_sweep_bytes.restype = C.c_int
    lib.gsfm_rot_loss_eval.argtypes = [C.c_void_p, _DP, C.c_uint64, _DP, _DP, _DP]; lib.gsfm_rot_loss_eval.restype = C.c_int
    lib.gsfm_rot_edge_order.argtypes = [C.c_void_p, _U32P, C.c_uint64]; lib.gsfm_rot_edge_order.restype = C.c_int64
    lib.gsfm_rot_locality_order.argtypes = [C.c_uint32, C.c_uint64, _U32P, _U32P, _U32P]; lib.gsfm_rot_locality_order.restype = C.c_int32
    lib.gsfm_rot_edge_sq_norms.argtypes = [C.c_uint32, C.c_uint64, _U32P, _U32P, _DP, _DP, _DP, C.c_double, _DP, C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), _DP]
    lib.gsfm_rot_edge_sq_norms.restype = C.c_int
    lib.gsfm_rot_dense_factor_check.argtypes = [C.c_int32, C.c_uint32, _U32P, _DP, _DP, C.POINTER(C.c_int32), _DP, _DP, C.POINTER(C.c_int32)]
    lib.gsfm_rot_dense_factor_check.restype = C.c_int
    lib.gsfm_rot_step_check.argtypes = [C.c_void_p, _DP, C.c_double, C.c_double, C.POINTER(Options), _DP, _DP, _DP, _DP, _DP, _DP, _DP, C.POINTER(StepInfo)]
    lib.gsfm_rot_step_check.restype = C.c_int
    lib.gsfm_rot_init_spanning_tree.argtypes = [C.c_uint32, C.c_uint64, _U32P, _U32P, _DP, C.POINTER(C.c_int32), _DP, C.POINTER(C.c_int64),
                                                _U32P, _U32P, _U32P, _DP]
    lib.gsfm_rot_init_spanning_tree.restype = C.c_int
    lib.gsfm_rot_count_components.argtypes = [C.c_uint32, C.c_uint64, _U32P, _U32P]; lib.gsfm_rot_count_components.restype = C.c_int64
    lib.gsfm_cov_estimate.argtypes = [C.c_uint64, C.POINTER(C.c_uint64), _DP, _DP, _DP, _DP, C.c_int32, _DP, _DP, _DP,
                                      C.POINTER(C.c_int32), C.POINTER(C.c_int32), _DP]
    lib.gsfm_cov_estimate.restype = C.c_int
    lib.gsfm_magsac_table.argtypes = [C.c_int32, _DP, C.c_int32]; lib.gsfm_magsac_table.restype = C.c_int32
    lib.gsfm_magsac_constants.argtypes = [C.c_int32, _DP, _DP, _DP]; lib.gsfm_magsac_constants.restype = C.c_int
    declare_position_signatures(lib)
    declare_track_signatures(lib)
    declare_ba_signatures(lib)
    declare_ba6_signatures(lib)
    declare_ba7_signatures(lib)
    declare_posp_signatures(lib)
    declare_rot_l1l2_signatures(lib)
    _lib = lib
    return lib


def declare_rot_l1l2_signatures(lib):
    """include/gsfm_rot_l1l2.h"""
    opt = C.POINTER(RotL1L2Options)
    lib.gsfm_rot_l1l2_abi_version.restype = C.c_int
    lib.gsfm_rot_l1l2_options_default.argtypes = [opt]; lib.gsfm_rot_l1l2_options_default.restype = None
    lib.gsfm_rot_l1l2_solve.argtypes = [C.c_uint32, C.c_uint64, _U32P, _U32P, _DP, _DP, C.c_int32, opt, C.POINTER(RotL1L2Summary)]
    lib.gsfm_rot_l1l2_solve.restype = C.c_int
    lib.gsfm_rot_l1l2_residuals.argtypes = [C.c_uint32, C.c_uint64, _U32P, _U32P, _DP, _DP, opt, _DP, _DP, _DP]
    lib.gsfm_rot_l1l2_residuals.restype = C.c_int
    lib.gsfm_rot_l1l2_laplacian_solve.argtypes = [C.c_uint32, C.c_uint64, _U32P, _U32P, _DP, C.c_int32, _DP, opt, _DP, _DP]
    lib.gsfm_rot_l1l2_laplacian_solve.restype = C.c_int


def declare_position_signatures(lib):
    """include/gsfm_pos.h"""
    lib.gsfm_pos_abi_version.restype = C.c_int
    lib.gsfm_pos_options_default.argtypes = [C.POINTER(PosOptions)]; lib.gsfm_pos_options_default.restype = None
    lib.gsfm_pos_problem_create.argtypes = [C.c_uint32, C.c_uint64, _U32P, _U32P, _DP, _DP, C.POINTER(C.c_void_p)]
    lib.gsfm_pos_problem_create.restype = C.c_int
    lib.gsfm_pos_set_loss.argtypes = [C.c_void_p, C.POINTER(LossNode), C.c_int32]; lib.gsfm_pos_set_loss.restype = C.c_int
    lib.gsfm_pos_set_loss_callback.argtypes = [C.c_void_p, LOSS_CALLBACK_FN, C.c_void_p]; lib.gsfm_pos_set_loss_callback.restype = C.c_int
    lib.gsfm_pos_solve.argtypes = [C.c_void_p, _DP, C.c_int32, C.POINTER(PosOptions), C.POINTER(PosSummary)]; lib.gsfm_pos_solve.restype = C.c_int
    lib.gsfm_pos_residuals.argtypes = [C.c_void_p, _DP, _DP, _DP]; lib.gsfm_pos_residuals.restype = C.c_int
    lib.gsfm_pos_linearize.argtypes = [C.c_void_p, _DP, _DP, _DP, _DP]; lib.gsfm_pos_linearize.restype = C.c_int
    lib.gsfm_pos_normal_matvec.argtypes = [C.c_void_p, _DP, _DP]; lib.gsfm_pos_normal_matvec.restype = C.c_int
    lib.gsfm_pos_step_check.argtypes = [C.c_void_p, _DP, C.c_int32, C.c_double, C.POINTER(PosOptions), _DP, _DP, _DP, _DP, _DP,
                                        C.POINTER(C.c_int32)]
    lib.gsfm_pos_step_check.restype = C.c_int
    lib.gsfm_pos_problem_destroy.argtypes = [C.c_void_p]; lib.gsfm_pos_problem_destroy.restype = None
    lib.gsfm_pos_filter_relative_translations.argtypes = [C.c_uint32, C.c_uint64, _U32P, _U32P, _DP, _DP, C.c_int32, _DP, C.c_uint64, C.c_double,
                                                          _DP, C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), _DP, _DP, _DP, _U32P, _U32P, _DP]
    lib.gsfm_pos_filter_relative_translations.restype = C.c_int
    lib.gsfm_pos_refine_relative_translations.argtypes = [C.c_uint32, C.c_uint64, _U32P, _U32P, C.POINTER(C.c_uint64), _DP, _DP, _DP, _DP, _DP,
                                                          C.POINTER(C.c_int32), C.POINTER(C.c_int32), _DP, _DP]
    lib.gsfm_pos_refine_relative_translations.restype = C.c_int


def declare_track_signatures(lib):
    """include/gsfm_tracks.h"""
    u64p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    lib.gsfm_tracks_triangulate.argtypes = [C.c_uint32, _DP, _DP, _DP, C.POINTER(C.c_uint8), C.c_uint64, u64p, _U32P, _DP, C.c_double, C.c_double,
                                            _DP, i32p, i32p, _DP, u64p, _DP]
    lib.gsfm_tracks_triangulate.restype = C.c_int
    lib.gsfm_tracks_launch_order.argtypes = [C.c_uint64, u64p, _U32P, u64p]
    lib.gsfm_tracks_launch_order.restype = C.c_int
    lib.gsfm_tracks_refine_default_options.argtypes = [C.POINTER(TrackRefineOptions)]
    lib.gsfm_tracks_refine_default_options.restype = None
    lib.gsfm_tracks_triangulate_refine.argtypes = [C.c_uint32, _DP, _DP, _DP, C.POINTER(C.c_uint8), C.c_uint64, u64p, _U32P, _DP, C.c_double, C.c_double,
                                                   C.POINTER(TrackRefineOptions), C.POINTER(LossNode), C.c_int32,
                                                   _DP, i32p, i32p, _DP, i32p, _DP, _DP, i32p, u64p, _DP]
    lib.gsfm_tracks_triangulate_refine.restype = C.c_int
    lib.gsfm_tracks_outlier_tracks.argtypes = [C.c_uint32, _DP, _DP, _DP, C.POINTER(C.c_uint8), C.c_uint64, u64p, _U32P, _DP, _DP, C.POINTER(C.c_uint8),
                                               C.c_double, C.c_double, i32p, i32p, _DP, u64p, _DP]
    lib.gsfm_tracks_outlier_tracks.restype = C.c_int
    lib.gsfm_tracks_build_default_options.argtypes = [C.POINTER(TrackBuildOptions)]
    lib.gsfm_tracks_build_default_options.restype = None
    for build in (lib.gsfm_tracks_build, lib.gsfm_tracks_build_sequential):
        build.argtypes = [C.c_uint32, C.c_uint64, _U32P, _U32P, u64p, _DP, C.POINTER(TrackBuildOptions), u64p, _U32P, _DP, u64p, u64p, u64p, _DP]
        build.restype = C.c_int
    u8p = C.POINTER(C.c_uint8)
    lib.gsfm_tracks_select_good.argtypes = [C.c_uint32, _DP, _DP, _DP, u8p, C.c_uint64, u64p, _U32P, _DP, _DP, u8p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                            u8p, i32p, _DP, u64p, _DP, _DP]
    lib.gsfm_tracks_select_good.restype = C.c_int
    lib.gsfm_tracks_select_good_from_statistics.argtypes = [C.c_uint32, u8p, C.c_uint64, u64p, _U32P, _DP, u8p, i32p, _DP, C.c_int32, C.c_int32, C.c_int32,
                                                            u8p, u64p]
    lib.gsfm_tracks_select_good_from_statistics.restype = C.c_int


def declare_ba_signatures(lib):
    """include/gsfm_ba.h"""
    u8p, u64p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    lib.gsfm_ba_abi_version.restype = C.c_int
    lib.gsfm_ba_options_default.argtypes = [C.POINTER(BaOptions)]; lib.gsfm_ba_options_default.restype = None
    lib.gsfm_ba_problem_create.argtypes = [C.c_uint32, _DP, _DP, u8p, C.c_uint64, u64p, _U32P, _DP, u8p, C.POINTER(C.c_void_p)]
    lib.gsfm_ba_problem_create.restype = C.c_int
    lib.gsfm_ba_set_loss.argtypes = [C.c_void_p, C.POINTER(LossNode), C.c_int32]; lib.gsfm_ba_set_loss.restype = C.c_int
    lib.gsfm_ba_solve.argtypes = [C.c_void_p, _DP, _DP, C.POINTER(BaOptions), C.POINTER(BaSummary)]; lib.gsfm_ba_solve.restype = C.c_int
    lib.gsfm_ba_residuals.argtypes = [C.c_void_p, _DP, _DP, _DP, _DP]; lib.gsfm_ba_residuals.restype = C.c_int
    lib.gsfm_ba_linearize.argtypes = [C.c_void_p, _DP, _DP, _DP, _DP, _DP, _DP, _DP]; lib.gsfm_ba_linearize.restype = C.c_int
    lib.gsfm_ba_schur_matvec.argtypes = [C.c_void_p, _DP, C.c_double, C.POINTER(BaOptions), _DP]; lib.gsfm_ba_schur_matvec.restype = C.c_int
    lib.gsfm_ba_step_check.argtypes = [C.c_void_p, _DP, _DP, C.c_double, C.POINTER(BaOptions), _DP, _DP, _DP, _DP, _DP, _DP, i32p]
    lib.gsfm_ba_step_check.restype = C.c_int
    lib.gsfm_ba_time_kernels.argtypes = [C.c_void_p, _DP, _DP, C.c_double, C.c_int32, _DP]; lib.gsfm_ba_time_kernels.restype = C.c_int
    lib.gsfm_ba_problem_destroy.argtypes = [C.c_void_p]; lib.gsfm_ba_problem_destroy.restype = None


def declare_posp_signatures(lib):
    """include/gsfm_posp.h (the options are gsfm_pos.h's)"""
    u64p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    lib.gsfm_posp_abi_version.restype = C.c_int
    lib.gsfm_posp_problem_create.argtypes = [C.c_uint32, C.c_uint64, _U32P, _U32P, _DP, _DP, _DP, _DP, C.c_uint64, u64p, _U32P, _DP, C.c_double,
                                             C.POINTER(C.c_void_p)]
    lib.gsfm_posp_problem_create.restype = C.c_int
    lib.gsfm_posp_set_loss.argtypes = [C.c_void_p, C.POINTER(LossNode), C.c_int32]; lib.gsfm_posp_set_loss.restype = C.c_int
    lib.gsfm_posp_set_loss_callback.argtypes = [C.c_void_p, LOSS_CALLBACK_FN, C.c_void_p]; lib.gsfm_posp_set_loss_callback.restype = C.c_int
    lib.gsfm_posp_solve.argtypes = [C.c_void_p, _DP, _DP, C.c_int32, C.POINTER(PosOptions), C.POINTER(PospSummary)]; lib.gsfm_posp_solve.restype = C.c_int
    lib.gsfm_posp_residuals.argtypes = [C.c_void_p] + [_DP] * 7; lib.gsfm_posp_residuals.restype = C.c_int
    lib.gsfm_posp_linearize.argtypes = [C.c_void_p] + [_DP] * 7; lib.gsfm_posp_linearize.restype = C.c_int
    lib.gsfm_posp_schur_matvec.argtypes = [C.c_void_p, _DP, C.c_double, C.POINTER(PosOptions), _DP]; lib.gsfm_posp_schur_matvec.restype = C.c_int
    lib.gsfm_posp_step_check.argtypes = [C.c_void_p, _DP, _DP, C.c_int32, C.c_double, C.POINTER(PosOptions)] + [_DP] * 6 + [i32p]
    lib.gsfm_posp_step_check.restype = C.c_int
    lib.gsfm_posp_time_kernels.argtypes = [C.c_void_p, _DP, _DP, C.c_double, C.c_int32, _DP]; lib.gsfm_posp_time_kernels.restype = C.c_int
    lib.gsfm_posp_problem_destroy.argtypes = [C.c_void_p]; lib.gsfm_posp_problem_destroy.restype = None


def declare_ba6_signatures(lib):
    """include/gsfm_ba6.h (the options and the summary are gsfm_ba.h's)"""
    u8p, u64p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    lib.gsfm_ba6_abi_version.restype = C.c_int
    lib.gsfm_ba6_options_default.argtypes = [C.POINTER(BaOptions)]; lib.gsfm_ba6_options_default.restype = None
    lib.gsfm_ba6_problem_create.argtypes = [C.c_uint32, _DP, u8p, C.c_uint64, u64p, _U32P, _DP, u8p, C.POINTER(C.c_void_p)]
    lib.gsfm_ba6_problem_create.restype = C.c_int
    lib.gsfm_ba6_set_loss.argtypes = [C.c_void_p, C.POINTER(LossNode), C.c_int32]; lib.gsfm_ba6_set_loss.restype = C.c_int
    lib.gsfm_ba6_solve.argtypes = [C.c_void_p, _DP, _DP, _DP, C.POINTER(BaOptions), C.POINTER(BaSummary)]; lib.gsfm_ba6_solve.restype = C.c_int
    lib.gsfm_ba6_residuals.argtypes = [C.c_void_p, _DP, _DP, _DP, _DP, _DP]; lib.gsfm_ba6_residuals.restype = C.c_int
    lib.gsfm_ba6_linearize.argtypes = [C.c_void_p] + [_DP] * 9; lib.gsfm_ba6_linearize.restype = C.c_int
    lib.gsfm_ba6_schur_matvec.argtypes = [C.c_void_p, _DP, C.c_double, C.POINTER(BaOptions), _DP]; lib.gsfm_ba6_schur_matvec.restype = C.c_int
    lib.gsfm_ba6_step_check.argtypes = [C.c_void_p, _DP, _DP, _DP, C.c_double, C.POINTER(BaOptions)] + [_DP] * 8 + [i32p]
    lib.gsfm_ba6_step_check.restype = C.c_int
    lib.gsfm_ba6_time_kernels.argtypes = [C.c_void_p, _DP, _DP, _DP, C.c_double, C.c_int32, _DP]; lib.gsfm_ba6_time_kernels.restype = C.c_int
    lib.gsfm_ba6_problem_destroy.argtypes = [C.c_void_p]; lib.gsfm_ba6_problem_destroy.restype = None


def declare_ba7_signatures(lib):
    """include/gsfm_ba7.h (the options and the summary are gsfm_ba.h's)"""
    u8p, u64p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    lib.gsfm_ba7_abi_version.restype = C.c_int
    lib.gsfm_ba7_options_default.argtypes = [C.POINTER(BaOptions)]; lib.gsfm_ba7_options_default.restype = None
    lib.gsfm_ba7_problem_create.argtypes = [C.c_uint32, _DP, u8p, u8p, C.c_uint64, u64p, _U32P, _DP, u8p, C.POINTER(C.c_void_p)]
    lib.gsfm_ba7_problem_create.restype = C.c_int
    lib.gsfm_ba7_set_loss.argtypes = [C.c_void_p, C.POINTER(LossNode), C.c_int32]; lib.gsfm_ba7_set_loss.restype = C.c_int
    lib.gsfm_ba7_solve.argtypes = [C.c_void_p, _DP, _DP, _DP, _DP, C.POINTER(BaOptions), C.POINTER(BaSummary)]; lib.gsfm_ba7_solve.restype = C.c_int
    lib.gsfm_ba7_residuals.argtypes = [C.c_void_p] + [_DP] * 6; lib.gsfm_ba7_residuals.restype = C.c_int
    lib.gsfm_ba7_linearize.argtypes = [C.c_void_p] + [_DP] * 11; lib.gsfm_ba7_linearize.restype = C.c_int
    lib.gsfm_ba7_schur_matvec.argtypes = [C.c_void_p, _DP, C.c_double, C.POINTER(BaOptions), _DP]; lib.gsfm_ba7_schur_matvec.restype = C.c_int
    lib.gsfm_ba7_step_check.argtypes = [C.c_void_p, _DP, _DP, _DP, _DP, C.c_double, C.POINTER(BaOptions)] + [_DP] * 9 + [i32p]
    lib.gsfm_ba7_step_check.restype = C.c_int
    lib.gsfm_ba7_time_kernels.argtypes = [C.c_void_p, _DP, _DP, _DP, _DP, C.c_double, C.c_int32, _DP]; lib.gsfm_ba7_time_kernels.restype = C.c_int
    lib.gsfm_ba7_problem_destroy.argtypes = [C.c_void_p]; lib.gsfm_ba7_problem_destroy.restype = None
