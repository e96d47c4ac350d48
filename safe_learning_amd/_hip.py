"""ctypes binding of libslhip.so (``include/sl_hip.h``) - the only way into the HIP engine.

There is no CPU fallback: if the shared library is missing or no GPU is present the loader /
context raise.  Device memory is owned by torch tensors (plumbing only); this module passes
their ``data_ptr()`` across the C ABI.
"""

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# SL_LIB_PATH: another build of the same library (kernel A/B runs, tools/build_variant.sh)
LIB_PATH = os.environ.get("SL_LIB_PATH") or os.path.join(HERE, "libslhip.so")

MAX_STATE_DIM = 6
MAX_ACTION_DIM = 2
MAX_INPUT_DIM = 8
MAX_GP_HEADS = 6
MAX_NN_LAYERS = 4
MAX_SIMPLICES = 32

# error codes and enum values of include/sl_hip.h
OK, ERR_INVALID, ERR_HIP, ERR_UNSUPPORTED, ERR_NOMEM = 0, -1, -2, -3, -4
POLICY_LINEAR, POLICY_CONST, POLICY_TABLE, POLICY_TRI, POLICY_NETWORK = 1, 2, 3, 4, 5
DYN_LINEAR, DYN_PENDULUM, DYN_CARTPOLE, DYN_GP, DYN_POLYNOMIAL = 1, 2, 3, 4, 5
POLY_MAX_TERMS, POLY_MAX_DEGREE = 64, 8
V_QUADRATIC, V_TRI, V_NETWORK, V_POLYNOMIAL = 1, 2, 3, 4
POLYV_MAX_ENTRIES = 256
LIP_CONST, LIP_ABS_LINEAR, LIP_NORM_LINEAR, LIP_ABS_GRAD, LIP_NORM_GRAD = 0, 1, 2, 3, 4
LF_CONST, LF_AFFINE_NORM1 = 0, 1
EVAL_VALUE, EVAL_POLICY, EVAL_DYNAMICS, EVAL_DECREASE, EVAL_LV, EVAL_GRADIENT = 1, 2, 3, 4, 5, 6
NN_LOSS_ABS, NN_LOSS_ROA = 1, 2

c_double_p = C.POINTER(C.c_double)


class GridDesc(C.Structure):
    _fields_ = [("d", C.c_int32), ("reserved", C.c_int32),
                ("num_points", C.c_int64 * MAX_STATE_DIM),
                ("offset", C.c_double * MAX_STATE_DIM),
                ("unit_maxes", C.c_double * MAX_STATE_DIM),
                ("upper", C.c_double * MAX_STATE_DIM)]


class PolicyDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("m", C.c_int32), ("saturate", C.c_int32),
                ("reserved", C.c_int32),
                ("matrix", (C.c_double * MAX_STATE_DIM) * MAX_ACTION_DIM),
                ("lower", C.c_double * MAX_ACTION_DIM), ("upper", C.c_double * MAX_ACTION_DIM),
                ("constant", C.c_double * MAX_ACTION_DIM),
                ("d_table", C.c_void_p)]


class DynamicsDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("normalize", C.c_int32),
                ("matrix", (C.c_double * MAX_INPUT_DIM) * MAX_STATE_DIM),
                ("tx", C.c_double * MAX_STATE_DIM), ("tx_inv", C.c_double * MAX_STATE_DIM),
                ("tu", C.c_double * MAX_ACTION_DIM),
                ("coef", C.c_double * 16)]


class ValueDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("negate", C.c_int32),
                ("matrix", (C.c_double * MAX_INPUT_DIM) * MAX_INPUT_DIM)]


class LipschitzDesc(C.Structure):
    _fields_ = [("lv_kind", C.c_int32), ("lv_cols", C.c_int32), ("lv_const", C.c_double),
                ("lv_matrix", (C.c_double * MAX_STATE_DIM) * MAX_STATE_DIM),
                ("lf_const", C.c_double), ("tau", C.c_double),
                ("lf_kind", C.c_int32), ("lf_reserved", C.c_int32),
                ("lf_matrix", (C.c_double * MAX_STATE_DIM) * MAX_STATE_DIM)]


KERNEL_RBF, KERNEL_MATERN32, KERNEL_LINEAR = 0, 1, 2
KERNEL_MAX_FACTORS = 8


class GpKernelFactor(C.Structure):
    _fields_ = [("kind", C.c_int32), ("product", C.c_int32),
                ("variance", C.c_double * MAX_INPUT_DIM),
                ("inv_lengthscales", C.c_double * MAX_INPUT_DIM)]


class GpKernel(C.Structure):
    """``sl_gp_kernel``: a sum of products of RBF / Matern32 / Linear leaves."""
    _fields_ = [("nfactors", C.c_int32), ("reserved", C.c_int32),
                ("factor", GpKernelFactor * KERNEL_MAX_FACTORS)]


class ModelDesc(C.Structure):
    _fields_ = [("grid", GridDesc), ("policy", PolicyDesc), ("dynamics", DynamicsDesc),
                ("value", ValueDesc), ("lipschitz", LipschitzDesc), ("reward", ValueDesc),
                ("gamma", C.c_double)]


class Key(C.Structure):
    _fields_ = [("vbits", C.c_uint64), ("index", C.c_int64)]


class SuccessorCacheStats(C.Structure):
    """``sl_successor_cache_stats`` (include/sl_hip.h)."""
    _fields_ = [("bytes", C.c_int64), ("max_bytes", C.c_int64), ("lo", C.c_int64), ("hi", C.c_int64),
                ("valid", C.c_int32), ("n_actions", C.c_int32), ("fills", C.c_int64),
                ("hits", C.c_int64), ("policy_hits", C.c_int64)]


class ValueSolveStats(C.Structure):
    """``sl_value_solve_stats`` (include/sl_hip.h)."""
    _fields_ = [("iterations", C.c_int64), ("matvecs", C.c_int64), ("cycles", C.c_int64),
                ("jacobi_cycles", C.c_int64), ("residual_inf", C.c_double), ("bound", C.c_double),
                ("kappa", C.c_double), ("converged", C.c_int32), ("reserved", C.c_int32)]


SOLVE_GMRES, SOLVE_JACOBI = 0, 1
REDUCTIONS = {'mean': 0, 'sum': 1}          # enum sl_reduction


# sl_sweep_result as int64 words (a torch int64[8] tensor backs it on the device)
RESULT_WORDS = 8
R_FAIL_V, R_FAIL_I, R_LAST_V, R_LAST_I, R_MAX_V, R_MAX_I, R_BELOW, R_SAFE = range(8)
SORT_COUNT_WORDS = 256 * 2048          # uint32 scratch of sl_sort_pairs / sl_partition_by_digit
ADAPTIVE_ROW_WORDS = 6                 # vbits, index, decrease, threshold(tau = 1), refinement, flags
# sl_select_state as int64 words: prefix, remaining, key.vbits, key.index, rank, none, pad, pad
SELECT_WORDS = 8
S_PREFIX, S_REMAINING, S_KEY_V, S_KEY_I, S_RANK, S_NONE = range(6)

# ---- the C ABI: one entry per prototype of include/sl_hip.h, in its order: (return type, argument
# types), the context pointer included.  tests/test_abi.py compares every entry with the header.
_vp, _i64, _int, _dbl = C.c_void_p, C.c_int64, C.c_int, C.c_double
_int32_p = C.POINTER(C.c_int32)

SIGNATURES = {
    # context
    "sl_version": (_int, ()),
    "sl_ctx_create": (_int, (_int, _vp, C.POINTER(_vp))),
    "sl_ctx_destroy": (_int, (_vp,)),
    "sl_last_error": (C.c_char_p, (_vp,)),
    "sl_ctx_synchronize": (_int, (_vp,)),
    "sl_last_kernel": (C.c_char_p, (_vp,)),
    "sl_timing_configure": (_int, (_vp, _int)),
    "sl_timing_collect": (_int, (_vp, _int, c_double_p, _int, C.POINTER(_int))),
    # model upload
    "sl_model_set": (_int, (_vp, C.POINTER(ModelDesc))),
    "sl_policy_touch": (_int, (_vp,)),
    "sl_dynamics_polynomial_set": (_int, (_vp, _int, _int, _int, _int32_p, c_double_p, C.POINTER(C.c_uint8), _int,
                                          _dbl)),
    "sl_value_polynomial_set": (_int, (_vp, _int, _int, c_double_p, C.POINTER(C.c_uint8), _int, c_double_p)),
    "sl_gp_set_head": (_int, (_vp, _int, _int, _int, _int, _int, c_double_p, c_double_p, c_double_p, _dbl,
                              c_double_p)),
    "sl_gp_set_head_kernel": (_int, (_vp, _int, _int, _int, _int, _int, c_double_p, c_double_p, c_double_p,
                                     C.POINTER(GpKernel))),
    "sl_gp_append_point": (_int, (_vp, _int, c_double_p, c_double_p, c_double_p)),
    "sl_gp_variance_floor": (_int, (_vp, _int, c_double_p, _int)),
    "sl_gp_configure": (_int, (_vp, _int, _dbl)),
    "sl_gp4_early_configure": (_int, (_vp, _int)),
    "sl_gp4_workgroups_configure": (_int, (_vp, _int)),
    "sl_gp4_segment_configure": (_int, (_vp, _int)),
    "sl_gp4_halves_configure": (_int, (_vp, _int)),
    "sl_gp4_predecide_configure": (_int, (_vp, _int, _int)),
    "sl_gp4_open_list": (_int, (_vp, C.POINTER(C.c_uint32), _i64, C.POINTER(C.c_ulonglong), C.POINTER(_int))),
    "sl_tri_set": (_int, (_vp, _int, C.POINTER(GridDesc), _int, _int32_p, c_double_p, c_double_p, _int, _int,
                          _vp)),
    "sl_tri_set_table": (_int, (_vp, _int, _vp)),
    "sl_network_set": (_int, (_vp, _int, _int32_p, _int32_p, c_double_p)),
    "sl_policy_network_set": (_int, (_vp, _int, _int32_p, _int32_p, c_double_p, c_double_p, _int32_p, _dbl)),
    # Lyapunov passes
    "sl_values": (_int, (_vp, _i64, _i64, _vp)),
    "sl_lyap_sweep": (_int, (_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp)),
    # ... with every decision read from device memory
    "sl_values_implicit": (_int, (_vp, C.POINTER(_int))),
    "sl_fold_results": (_int, (_vp, _vp, _int, _vp)),
    "sl_lyap_finalize_dev": (_int, (_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp)),
    "sl_refinement_carry": (_int, (_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp)),
    "sl_select_begin": (_int, (_vp, _vp, _i64, _i64, _vp, _i64)),
    "sl_select_hist": (_int, (_vp, _i64, _i64, _vp, _int, _int, _vp, _vp)),
    "sl_select_digit": (_int, (_vp, _int, _int, _vp, _vp)),
    # sort / partition / the adaptive branch
    "sl_sort_pairs": (_int, (_vp, _i64, _vp, _vp, _vp, _vp, _vp)),
    "sl_partition_by_digit": (_int, (_vp, _i64, _vp, _vp, _vp, _vp)),
    "sl_gather_rows": (_int, (_vp, _i64, _int, _vp, _vp, _vp)),
    "sl_adaptive_pack": (_int, (_vp, _i64, _i64, _vp, _vp, _int, _vp, _vp, _vp, _vp)),
    "sl_adaptive_dest": (_int, (_vp, _i64, _vp, _vp, _int, _vp)),
    "sl_adaptive_sort_keys": (_int, (_vp, _i64, _vp, _vp, _vp)),
    "sl_adaptive_analyse": (_int, (_vp, _i64, _i64, _i64, _vp, _vp, _dbl, _dbl, _i64, _vp, _vp)),
    "sl_adaptive_apply": (_int, (_vp, _i64, _i64, _i64, _vp, _vp, _vp, _dbl, _dbl, _i64, _vp)),
    "sl_adaptive_scatter": (_int, (_vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp)),
    # get_safe_sample glue
    "sl_index_to_state": (_int, (_vp, _i64, _vp, _vp)),
    "sl_perturb_pairs": (_int, (_vp, _i64, _int, _int, _vp, _vp, _int, _vp, _vp, _vp)),
    "sl_rows_sort_key": (_int, (_vp, _i64, _int, _int, _vp, _vp, _vp)),
    "sl_rows_duplicate_flags": (_int, (_vp, _i64, _int, _vp, _vp, _vp)),
    "sl_sample_bounds": (_int, (_vp, _i64, _int, _int, _vp, _vp, _vp, _dbl, _vp, _vp)),
    "sl_state_membership": (_int, (_vp, _i64, _vp, _vp, _vp)),
    "sl_argmax_masked": (_int, (_vp, _i64, _vp, _vp, _vp)),
    "sl_argmax_rows_masked": (_int, (_vp, _i64, _int, _vp, _vp, _i64, _vp)),
    "sl_lyapunov_region": (_int, (_vp, _vp, _i64, _vp, _vp, C.POINTER(_int))),
    "sl_bits_to_bytes": (_int, (_vp, _i64, _vp, _vp)),
    "sl_bytes_to_bits": (_int, (_vp, _i64, _vp, _vp)),
    "sl_bits_count": (_int, (_vp, _i64, _vp, _vp, _vp, C.POINTER(_i64))),
    "sl_bits_to_indices": (_int, (_vp, _i64, _vp, _vp, _vp)),
    # dynamic programming, exact policy evaluation, the successor cache
    "sl_bellman_sweep": (_int, (_vp, _i64, _i64, _int, c_double_p, _vp, _vp, _vp, _vp)),
    "sl_policy_operator": (_int, (_vp, _i64, _i64, _vp, _vp, _vp, _vp)),
    "sl_value_solve": (_int, (_vp, _i64, _int, _vp, _vp, _vp, _dbl, _vp, _dbl, _i64, _int, _int,
                              C.POINTER(ValueSolveStats))),
    "sl_successor_cache_configure": (_int, (_vp, _i64)),
    "sl_successor_cache_info": (_int, (_vp, C.POINTER(SuccessorCacheStats))),
    # evaluation at arbitrary points
    "sl_eval_points": (_int, (_vp, _int, _i64, _vp, _vp)),
    # closed-loop rollouts
    "sl_rollout": (_int, (_vp, _i64, _i64, _vp, _int, _int, _vp, _vp, _vp)),
    "sl_rollout_mask": (_int, (_vp, _i64, _int, _vp, c_double_p, _dbl, _vp, _vp)),
    "sl_reward_rollout": (_int, (_vp, _i64, _i64, _vp, _int, _vp, _dbl, _int, _vp, _vp, C.POINTER(_i64),
                                 C.POINTER(_int))),
    # the posterior mean of GP dynamics as a deterministic model
    "sl_gp_mean_points": (_int, (_vp, _i64, _vp, _vp)),
    "sl_rollout_mean": (_int, (_vp, _i64, _i64, _vp, _int, _int, _vp, _vp, _vp)),
    "sl_reward_rollout_mean": (_int, (_vp, _i64, _i64, _vp, _int, _vp, _dbl, _int, _vp, _vp, C.POINTER(_i64),
                                      C.POINTER(_int))),
    # training a LyapunovNetwork
    "sl_nn_param_grad": (_int, (_vp, _i64, _int, _vp, _vp, _vp)),
    "sl_nn_loss": (_int, (_vp, _int, _i64, _int, _vp, _vp, _vp, _vp, _dbl, _dbl, _dbl, _vp, _vp, _vp)),
    # policy gradients of future_values
    "sl_action_gradient": (_int, (_vp, _i64, _vp, _vp, _vp, _vp, _vp)),
    "sl_policy_param_grad": (_int, (_vp, _i64, _int, _vp, _vp, _vp)),
    "sl_tri_param_grad": (_int, (_vp, _int, _i64, _vp, _vp, _vp)),
    # the Lyapunov penalty of future_values, differentiated
    "sl_decrease_gradient": (_int, (_vp, _i64, _vp, _vp, _vp, _vp, _vp)),
    # actor-critic with a NeuralNetwork value function
    "sl_critic_batch": (_int, (_vp, _int, _int32_p, _int32_p, _int32_p, _dbl, _vp, _i64, _vp, _vp, _int, _vp, _vp, _vp,
                               _vp, _vp, _vp)),
    "sl_dense_param_grad": (_int, (_vp, _int, _int32_p, _int32_p, _int32_p, _dbl, _vp, _i64, _int, _vp, _vp, _vp)),
    # GP sample paths: posterior covariance, Cholesky, triangular solves and products, sample functions
    "sl_gp_posterior_cov": (_int, (_vp, _int, _int, c_double_p, c_double_p, c_double_p, C.POINTER(GpKernel), c_double_p,
                                   _i64, _vp, _dbl, _vp, _vp, _i64)),
    "sl_cholesky": (_int, (_vp, _i64, _vp, _i64, _int32_p)),
    "sl_tri_solve": (_int, (_vp, _i64, _i64, _vp, _i64, _int, _vp)),
    "sl_tri_mult": (_int, (_vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp)),
    "sl_gp_sample_eval": (_int, (_vp, C.POINTER(GpKernel), c_double_p, _int, _i64, _vp, _i64, _vp, _i64, _vp, _vp)),
    # GP hyper-parameters: log marginal likelihood and gradient
    "sl_gp_likelihood": (_int, (_vp, _int, _int, _int, c_double_p, c_double_p, C.POINTER(GpKernel), _dbl, c_double_p,
                                c_double_p, c_double_p, c_double_p, _int32_p)),
    # RCCL collectives
    "sl_comm_unique_id": (_int, (C.c_char_p,)),
    "sl_comm_init": (_int, (_vp, C.c_char_p, _int, _int)),
    "sl_comm_destroy": (_int, (_vp,)),
    "sl_allreduce_result": (_int, (_vp, _vp)),
    "sl_allgather": (_int, (_vp, _vp, _vp, _i64)),
    "sl_allreduce_sum_u64": (_int, (_vp, _vp, _i64)),
    "sl_allreduce_max_f64": (_int, (_vp, _vp, _i64)),
    # diagnostics
    "sl_debug_mfma": (_int, (_vp, c_double_p, c_double_p, c_double_p)),
    "sl_debug_mfma4": (_int, (_vp, _int, c_double_p, c_double_p, c_double_p, _int, c_double_p)),
    "sl_debug_fp64_rate": (_int, (_vp, _int, _int, c_double_p)),
    "sl_debug_gp_lml_grad": (_int, (_vp, _int, _int, _int, c_double_p, c_double_p, c_double_p, C.POINTER(GpKernel),
                                    c_double_p, c_double_p, c_double_p)),
    "sl_debug_gp_inputs": (_int, (_vp, _int, c_double_p)),
    "sl_debug_nn_train_scratch": (_int, (_vp, C.POINTER(_i64), C.POINTER(_int))),
}
EXPORTS = list(SIGNATURES)

_lib = None


class HipEngineError(RuntimeError):
    """Raised for every failure of the HIP engine (no silent fallbacks)."""


# entry points whose status is an answer their caller reads, not an error
UNCHECKED = ("sl_ctx_destroy", "sl_gp_append_point")


def _raise(lib, handle, what, rc):
    msg = lib.sl_last_error(handle)
    raise HipEngineError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))


def _bind(lib):
    """Set ``argtypes`` / ``restype`` of every entry point of ``lib`` from ``SIGNATURES``, and have the
    ones that work on a context raise ``HipEngineError`` on a status other than 0 (ctypes' ``errcheck``:
    one check where the call returns, nothing between a method and its entry point).  The shipped
    library must export all of them (tests/test_abi.py checks it symbol by symbol); a development
    library of another revision (SL_LIB_PATH: A/B runs of the kernels both have) may lack some."""
    dev = bool(os.environ.get("SL_LIB_PATH"))

    def errcheck(rc, fn, args):
        if rc != 0:
            _raise(lib, args[0], fn.__name__, rc)
        return rc

    for name, (restype, argtypes) in SIGNATURES.items():
        if not hasattr(lib, name):
            if dev:
                continue
            raise HipEngineError("libslhip.so (%s) does not export %s" % (LIB_PATH, name))
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = list(argtypes)
        if restype is _int and argtypes[:1] == (_vp,) and name not in UNCHECKED:
            fn.errcheck = errcheck
    return lib


def load_library():
    """Load libslhip.so (built by ``python -m safe_learning_amd._build``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipEngineError(
            "libslhip.so is missing (%s). Build it with `python -m safe_learning_amd._build`; "
            "safe_learning_amd has no CPU fallback." % LIB_PATH)
    # torch first: libslhip.so must bind the HIP runtime that torch ships (loading the system
    # libamdhip64 before torch's copy leaves the process with two runtimes, one without devices)
    import torch  # noqa: F401
    _lib = _bind(C.CDLL(LIB_PATH))
    return _lib


def _as_c(array):
    array = np.ascontiguousarray(array, dtype=np.float64)
    return array, array.ctypes.data_as(c_double_p)


def _ptr(tensor):
    """Device pointer of a torch tensor (or None)."""
    if tensor is None:
        return None
    return C.c_void_p(tensor.data_ptr())


class Context(object):
    """One engine context = one GPU + one HIP stream (torch's current stream).  ``lib`` is the library
    as ``load_library`` binds it: a call of an entry point on a context, ``lib.sl_x(handle, ...)``,
    raises ``HipEngineError`` on a status other than 0 instead of returning it (``_bind``)."""

    def __init__(self, device=None):
        import torch
        if not torch.cuda.is_available():
            raise HipEngineError("no GPU visible to torch; safe_learning_amd has no CPU fallback")
        self.lib = load_library()
        if device is None:
            device = torch.cuda.current_device()
        self.device = int(device)
        self.torch_device = torch.device("cuda", self.device)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream().cuda_stream
        handle = C.c_void_p()
        rc = self.lib.sl_ctx_create(self.device, C.c_void_p(stream), C.byref(handle))
        if rc != 0:
            raise HipEngineError("sl_ctx_create failed: %s" % self.lib.sl_last_error(None).decode())
        self.handle = handle
        self._keepalive = {}        # slot -> the device table the engine currently points at
        # SL_GP4_EARLY=0 (A/B runs, the bit-identity tests): k_gp_sweep4 runs every variance panel of
        # every tile.  Read here, once per context; `roofline.kernel` / last_kernel() name what ran.
        if os.environ.get("SL_GP4_EARLY") == "0":
            self.lib.sl_gp4_early_configure(self.handle, 0)
        # SL_GP4_WORKGROUPS=N (tests): at most N workgroups of k_gp_sweep4, so that one workgroup of a
        # small grid draws many tiles.  Set by every new context (unset: no cap).
        if hasattr(self.lib, "sl_gp4_workgroups_configure"):
            self.lib.sl_gp4_workgroups_configure(self.handle, int(os.environ.get("SL_GP4_WORKGROUPS") or 0))
        # SL_GP4_SEGMENT_TILES=N (tests): every block-mode launch of k_gp_sweep4 runs k_gp_mean_blocks
        # first, in segments of N source tiles
        if hasattr(self.lib, "sl_gp4_segment_configure"):
            self.lib.sl_gp4_segment_configure(self.handle, int(os.environ.get("SL_GP4_SEGMENT_TILES") or 0))
        # SL_GP4_HALVES=0 (A/B runs, tests): block mode decides and queues whole 16-cell blocks, not
        # their 8-cell halves.  Same results bit for bit; last_kernel() names the granule.
        if os.environ.get("SL_GP4_HALVES") == "0":
            self.lib.sl_gp4_halves_configure(self.handle, 0)
        # SL_GP4_PREDECIDE=0 (A/B runs, tests): no deciding pass in front of k_gp_mean_blocks;
        # SL_GP4_PREDECIDE_SPACING=S: the lattice spacing of its reference cells (default 8).  Same
        # results bit for bit; last_kernel() reports the blocks the pass decided.
        self.lib.sl_gp4_predecide_configure(self.handle, 0 if os.environ.get("SL_GP4_PREDECIDE") == "0" else 1,
                                            int(os.environ.get("SL_GP4_PREDECIDE_SPACING") or 0))

    def close(self):
        if getattr(self, "handle", None):
            self.lib.sl_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc, what):
        if rc != 0:
            _raise(self.lib, self.handle, what, rc)

    # ---- model ---------------------------------------------------------------------------
    def model_set(self, desc):
        self.lib.sl_model_set(self.handle, C.byref(desc))

    def policy_touch(self):
        """``sl_policy_touch``: the policy table the model points at was overwritten in place."""
        self.lib.sl_policy_touch(self.handle)

    def dynamics_polynomial_set(self, d, m, rows, coef, exponents, substeps, h):
        """``sl_dynamics_polynomial_set``: the term table of ``DYN_POLYNOMIAL`` - ``rows [nterms]`` output rows,
        ``coef [nterms]``, ``exponents [nterms, d + m]`` (small non-negative integers)."""
        rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
        coef, pc = _as_c(np.reshape(coef, -1))
        given = np.asarray(exponents, dtype=np.int64).reshape(len(rows), -1)
        if len(coef) != len(rows) or given.shape[1] > MAX_INPUT_DIM or (given < 0).any() or (given > 255).any():
            raise ValueError("polynomial terms: %d rows, %d coefficients, exponents of shape %s (at most %d columns, "
                             "entries in 0..255)" % (len(rows), len(coef), given.shape, MAX_INPUT_DIM))
        expo = np.zeros((len(rows), MAX_INPUT_DIM), dtype=np.uint8)
        expo[:, :given.shape[1]] = given
        self.lib.sl_dynamics_polynomial_set(self.handle, int(d), int(m), len(rows),
                                            rows.ctypes.data_as(_int32_p), pc,
                                            expo.ctypes.data_as(C.POINTER(C.c_uint8)), int(substeps), float(h))

    def value_polynomial_set(self, d, coef, exponents, normalization=None):
        """``sl_value_polynomial_set``: the term table of ``V_POLYNOMIAL`` - ``coef [nterms]``, ``exponents
        [nterms, d]`` (small non-negative integers), ``normalization [d]`` (the scales ``T``) or ``None``."""
        coef, pc = _as_c(np.reshape(coef, -1))
        given = np.asarray(exponents, dtype=np.int64)
        given = given.reshape(len(coef), -1) if len(coef) else np.zeros((0, int(d)), dtype=np.int64)
        if given.shape[1] > MAX_STATE_DIM or (given < 0).any() or (given > 255).any():
            raise ValueError("polynomial terms: exponents of shape %s (at most %d columns, entries in 0..255)"
                             % (given.shape, MAX_STATE_DIM))
        expo = np.zeros((len(coef), MAX_STATE_DIM), dtype=np.uint8)
        expo[:, :given.shape[1]] = given
        tx, ptx = _as_c(np.ones(MAX_STATE_DIM))
        if normalization is not None:
            tx[:len(normalization)] = np.asarray(normalization, dtype=np.float64)
        self.lib.sl_value_polynomial_set(self.handle, int(d), len(coef), pc, expo.ctypes.data_as(C.POINTER(C.c_uint8)),
                                         0 if normalization is None else 1, ptx)

    def gp_set_head(self, head, X, Linv, alpha, col0, variance, lengthscales):
        X, pX = _as_c(X)
        Linv, pL = _as_c(Linv)
        alpha, pA = _as_c(alpha)
        ls, pls = _as_c(lengthscales)
        n, p = X.shape
        self.lib.sl_gp_set_head(self.handle, head, n, p, alpha.shape[1], col0, pX, pL, pA, float(variance),
                                pls)

    def gp_set_head_kernel(self, head, X, Linv, alpha, col0, factors):
        """``factors``: ``[(kind, product, variance[p], inv_lengthscales[p])]`` - a sum of products
        of leaf kernels (``sl_gp_kernel`` of include/sl_hip.h)."""
        X, pX = _as_c(X)
        Linv, pL = _as_c(Linv)
        alpha, pA = _as_c(alpha)
        n, p = X.shape
        if len(factors) > KERNEL_MAX_FACTORS:
            raise ValueError("kernel with %d leaf factors (engine limit %d)" % (len(factors), KERNEL_MAX_FACTORS))
        spec = GpKernel()
        spec.nfactors = len(factors)
        for f, (kind, product, variance, inv_ls) in enumerate(factors):
            spec.factor[f].kind, spec.factor[f].product = int(kind), int(product)
            for q in range(p):
                spec.factor[f].variance[q] = float(variance[q])
                spec.factor[f].inv_lengthscales[q] = float(inv_ls[q])
        self.lib.sl_gp_set_head_kernel(self.handle, head, n, p, alpha.shape[1], col0, pX, pL, pA,
                                       C.byref(spec))

    def gp_append_point(self, head, x, linv_row, alpha_new):
        """One more training point for an uploaded head; False if the head has to be re-packed."""
        x, px = _as_c(x)
        row, pr = _as_c(linv_row)
        a, pa = _as_c(alpha_new)
        rc = self.lib.sl_gp_append_point(self.handle, head, px, pr, pa)
        if rc == ERR_UNSUPPORTED:                      # capacity exhausted
            return False
        self.check(rc, "sl_gp_append_point")
        return True

    def gp_variance_floor(self, head, stages):
        """The variance-floor constants of an uploaded head, one per 256-row panel boundary, read back
        from the device (``sl_gp_variance_floor``); all zero after ``gp_append_point``.  Raises
        ``HipEngineError`` like every bound entry point (``_bind``): a head that is not set, more than
        32 stages."""
        out = np.zeros(stages, dtype=np.float64)
        self.lib.sl_gp_variance_floor(self.handle, head, out.ctypes.data_as(c_double_p), stages)
        return out

    def gp_inputs(self, head, n, p):
        """Scaled training inputs of an uploaded head as the kernels read them, ``[p, n]``."""
        out = np.empty((p, n), dtype=np.float64)
        self.lib.sl_debug_gp_inputs(self.handle, head, out.ctypes.data_as(c_double_p))
        return out

    def gp_configure(self, nheads, beta):
        self.lib.sl_gp_configure(self.handle, nheads, float(beta))

    def tri_set(self, slot, grid_desc, simplices, hyperplanes, discrete_points, project, ncols,
                table):
        simplices = np.ascontiguousarray(simplices, dtype=np.int32)
        hyper, ph = _as_c(hyperplanes)
        pts, pp = _as_c(np.concatenate(discrete_points))
        self._keepalive[slot] = table
        self.lib.sl_tri_set(self.handle, slot, C.byref(grid_desc), len(simplices),
                            simplices.ctypes.data_as(C.POINTER(C.c_int32)), ph, pp, int(bool(project)),
                            ncols, _ptr(table))

    def tri_set_table(self, slot, table):
        self._keepalive[slot] = table
        self.lib.sl_tri_set_table(self.handle, slot, _ptr(table))

    def network_set(self, dims, activations, kernels):
        dims = np.ascontiguousarray(dims, dtype=np.int32)
        acts = np.ascontiguousarray(activations, dtype=np.int32)
        flat, pk = _as_c(np.concatenate([np.asarray(k, dtype=np.float64).ravel() for k in kernels]))
        self.lib.sl_network_set(self.handle, len(acts), dims.ctypes.data_as(C.POINTER(C.c_int32)),
                                acts.ctypes.data_as(C.POINTER(C.c_int32)), pk)

    def policy_network_set(self, dims, activations, kernels, biases, output_scale):
        """``sl_policy_network_set``: ``kernels[l]`` is ``[in, out]``, ``biases[l]`` an ``[out]`` array or None."""
        dims = np.ascontiguousarray(dims, dtype=np.int32)
        acts = np.ascontiguousarray(activations, dtype=np.int32)
        flat, pk = _as_c(np.concatenate([np.asarray(k, dtype=np.float64).ravel() for k in kernels]))
        has = np.ascontiguousarray([0 if b is None else 1 for b in biases], dtype=np.int32)
        present = [np.asarray(b, dtype=np.float64).ravel() for b in biases if b is not None]
        bflat, pb = _as_c(np.concatenate(present) if present else np.zeros(1))
        self.lib.sl_policy_network_set(self.handle, len(acts), dims.ctypes.data_as(C.POINTER(C.c_int32)),
                                       acts.ctypes.data_as(C.POINTER(C.c_int32)), pk, pb,
                                       has.ctypes.data_as(C.POINTER(C.c_int32)), float(output_scale))

    # ---- passes --------------------------------------------------------------------------
    def values(self, lo, hi, d_values):
        self.lib.sl_values(self.handle, lo, hi, _ptr(d_values))

    def lyap_sweep(self, lo, hi, d_init_bits, d_values, d_neg_bits, d_result, d_dbg=None):
        self.lib.sl_lyap_sweep(self.handle, lo, hi, _ptr(d_init_bits), _ptr(d_values), _ptr(d_neg_bits),
                               _ptr(d_result), _ptr(d_dbg))

    # ---- the same passes with every decision read from device memory (sl_level.hip) -------
    def values_implicit(self):
        """True when ``d_values=None`` is allowed: quadratic V whose ordering keys the passes
        recompute from the cell index (``sl_values_implicit``)."""
        out = C.c_int(0)
        self.lib.sl_values_implicit(self.handle, C.byref(out))
        return bool(out.value)

    def fold_results(self, d_records, count, d_out):
        self.lib.sl_fold_results(self.handle, _ptr(d_records), count, _ptr(d_out))

    def lyap_finalize_dev(self, lo, hi, d_values, d_init_bits, d_prev_bits, d_folded, d_keep,
                          d_safe_bits, d_result):
        self.lib.sl_lyap_finalize_dev(self.handle, lo, hi, _ptr(d_values), _ptr(d_init_bits),
                                      _ptr(d_prev_bits), _ptr(d_folded), _ptr(d_keep), _ptr(d_safe_bits),
                                      _ptr(d_result))

    def refinement_carry(self, lo, hi, d_values, d_init_bits, d_neg_bits, d_folded, d_keep, d_refinement):
        self.lib.sl_refinement_carry(self.handle, lo, hi, _ptr(d_values), _ptr(d_init_bits),
                                     _ptr(d_neg_bits), _ptr(d_folded), _ptr(d_keep), _ptr(d_refinement))

    def select_begin(self, d_state, k, batch, d_folded, n_total):
        self.lib.sl_select_begin(self.handle, _ptr(d_state), k, batch, _ptr(d_folded), n_total)

    def select_hist(self, lo, hi, d_values, which, byte, d_state, d_hist):
        self.lib.sl_select_hist(self.handle, lo, hi, _ptr(d_values), which, byte, _ptr(d_state),
                                _ptr(d_hist))

    def select_digit(self, which, byte, d_hist, d_state):
        self.lib.sl_select_digit(self.handle, which, byte, _ptr(d_hist), _ptr(d_state))

    # ---- sort / partition / the adaptive branch (sl_adaptive.hip) --------------------------
    def sort_pairs(self, n, d_keys, d_vals, d_keys_tmp, d_vals_tmp, d_counts):
        self.lib.sl_sort_pairs(self.handle, n, _ptr(d_keys), _ptr(d_vals), _ptr(d_keys_tmp),
                               _ptr(d_vals_tmp), _ptr(d_counts))

    def partition_by_digit(self, n, d_digits, d_perm, d_bucket_counts, d_counts):
        self.lib.sl_partition_by_digit(self.handle, n, _ptr(d_digits), _ptr(d_perm), _ptr(d_bucket_counts),
                                       _ptr(d_counts))

    def gather_rows(self, count, words, d_perm, d_rows_in, d_rows_out):
        self.lib.sl_gather_rows(self.handle, count, words, _ptr(d_perm), _ptr(d_rows_in), _ptr(d_rows_out))

    def adaptive_pack(self, lo, hi, d_values, d_records, stride, d_init_bits, d_prior_bits,
                      d_prior_ref, d_rows):
        self.lib.sl_adaptive_pack(self.handle, lo, hi, _ptr(d_values), _ptr(d_records), stride,
                                  _ptr(d_init_bits), _ptr(d_prior_bits), _ptr(d_prior_ref), _ptr(d_rows))

    def adaptive_dest(self, count, d_rows, d_splitters, nsplit, d_dest):
        self.lib.sl_adaptive_dest(self.handle, count, _ptr(d_rows), _ptr(d_splitters), nsplit, _ptr(d_dest))

    def adaptive_sort_keys(self, m, d_rows, d_keys, d_vals):
        self.lib.sl_adaptive_sort_keys(self.handle, m, _ptr(d_rows), _ptr(d_keys), _ptr(d_vals))

    def adaptive_analyse(self, m, pos0, batch, d_rows, d_order, tau, safety_factor, max_refinement,
                         d_info, d_first_break):
        self.lib.sl_adaptive_analyse(self.handle, m, pos0, batch, _ptr(d_rows), _ptr(d_order), float(tau),
                                     float(safety_factor), int(max_refinement), _ptr(d_info),
                                     _ptr(d_first_break))

    def adaptive_apply(self, m, pos0, batch, d_rows, d_order, d_info, tau, safety_factor, b_star,
                       d_out_rows):
        self.lib.sl_adaptive_apply(self.handle, m, pos0, batch, _ptr(d_rows), _ptr(d_order), _ptr(d_info),
                                   float(tau), float(safety_factor), int(b_star), _ptr(d_out_rows))

    def adaptive_scatter(self, lo, hi, m, d_out_rows, d_init_bits, d_safe_bits, d_refinement,
                         d_safe_count):
        self.lib.sl_adaptive_scatter(self.handle, lo, hi, m, _ptr(d_out_rows), _ptr(d_init_bits),
                                     _ptr(d_safe_bits), _ptr(d_refinement), _ptr(d_safe_count))

    # ---- get_safe_sample glue (sl_sample.hip) ----------------------------------------------
    def index_to_state(self, count, d_indices, d_states):
        self.lib.sl_index_to_state(self.handle, count, _ptr(d_indices), _ptr(d_states))

    def perturb_pairs(self, count, d, m, d_states, d_actions, nperturb, d_perturbations, d_limits,
                      d_pairs):
        self.lib.sl_perturb_pairs(self.handle, count, d, m, _ptr(d_states), _ptr(d_actions), nperturb,
                                  _ptr(d_perturbations), _ptr(d_limits), _ptr(d_pairs))

    def rows_sort_key(self, count, words, column, d_rows, d_order, d_keys):
        self.lib.sl_rows_sort_key(self.handle, count, words, column, _ptr(d_rows), _ptr(d_order),
                                  _ptr(d_keys))

    def rows_duplicate_flags(self, count, words, d_rows, d_order, d_flags):
        self.lib.sl_rows_duplicate_flags(self.handle, count, words, _ptr(d_rows), _ptr(d_order),
                                         _ptr(d_flags))

    def sample_bounds(self, count, d, lv_cols, d_std, d_lv, d_value, c_max, d_bound, d_inside):
        self.lib.sl_sample_bounds(self.handle, count, d, lv_cols, _ptr(d_std), _ptr(d_lv), _ptr(d_value),
                                  float(c_max), _ptr(d_bound), _ptr(d_inside))

    def state_membership(self, count, d_points, d_safe_bits, d_inout):
        self.lib.sl_state_membership(self.handle, count, _ptr(d_points), _ptr(d_safe_bits), _ptr(d_inout))

    def argmax_masked(self, count, d_values, d_mask, d_out):
        self.lib.sl_argmax_masked(self.handle, count, _ptr(d_values), _ptr(d_mask), _ptr(d_out))

    def argmax_rows_masked(self, count, n_actions, d_q, d_allowed_bits, words_per_action, d_best):
        self.lib.sl_argmax_rows_masked(self.handle, count, n_actions, _ptr(d_q), _ptr(d_allowed_bits),
                                       words_per_action, _ptr(d_best))

    def lyapunov_region(self, d_values, start, d_work, d_region):
        """-> relaxation passes used (``sl_lyapunov_region``)."""
        sweeps = C.c_int(0)
        self.lib.sl_lyapunov_region(self.handle, _ptr(d_values), int(start), _ptr(d_work), _ptr(d_region),
                                    C.byref(sweeps))
        return sweeps.value

    def bits_to_bytes(self, n, d_bits, d_bytes):
        self.lib.sl_bits_to_bytes(self.handle, n, _ptr(d_bits), _ptr(d_bytes))

    def bits_count(self, n, d_bits, d_block_counts, d_offsets):
        """-> number of set bits among the first ``n`` (``sl_bits_count``; fills the two scratch arrays)."""
        total = C.c_int64(0)
        self.lib.sl_bits_count(self.handle, n, _ptr(d_bits), _ptr(d_block_counts), _ptr(d_offsets),
                               C.byref(total))
        return total.value

    def bits_to_indices(self, n, d_bits, d_offsets, d_indices):
        if d_indices.numel() == 0:               # no bit set: nothing to write
            return
        self.lib.sl_bits_to_indices(self.handle, n, _ptr(d_bits), _ptr(d_offsets), _ptr(d_indices))

    def bytes_to_bits(self, n, d_bytes, d_bits):
        self.lib.sl_bytes_to_bits(self.handle, n, _ptr(d_bytes), _ptr(d_bits))

    def bellman_sweep(self, lo, hi, actions, d_v_new, d_argmax, d_q, d_stats):
        if actions is None:
            n_act, pa = 0, None
        else:
            actions, pa = _as_c(actions)
            n_act = actions.shape[0]
        self.lib.sl_bellman_sweep(self.handle, lo, hi, n_act, pa, _ptr(d_v_new), _ptr(d_argmax), _ptr(d_q),
                                  _ptr(d_stats))

    def policy_operator(self, lo, hi, d_cols, d_w, d_r, d_stats):
        """``sl_policy_operator``: ELL rows ``[d + 1][hi - lo]`` of the current policy's operator."""
        self.lib.sl_policy_operator(self.handle, lo, hi, _ptr(d_cols), _ptr(d_w), _ptr(d_r), _ptr(d_stats))

    def value_solve(self, n, k, d_cols, d_w, d_r, gamma, d_v, tol, max_matvecs, restart, method):
        """``sl_value_solve``: solves ``(I - gamma P) v = r`` in place of ``d_v``; the stats as a dict."""
        stats = ValueSolveStats()
        self.lib.sl_value_solve(self.handle, int(n), int(k), _ptr(d_cols), _ptr(d_w), _ptr(d_r),
                                float(gamma), _ptr(d_v), float(tol), int(max_matvecs), int(restart),
                                int(method), C.byref(stats))
        out = {name: getattr(stats, name) for name, _ in ValueSolveStats._fields_ if name != "reserved"}
        out["converged"] = bool(out["converged"])
        return out

    def successor_cache_configure(self, max_bytes):
        """Budget of the Bellman sweeps' successor cache (``sl_successor_cache_configure``):
        negative = default (a quarter of the device's memory), 0 = no cache."""
        self.lib.sl_successor_cache_configure(self.handle, int(max_bytes))

    def successor_cache_info(self):
        """``sl_successor_cache_info`` as a dict."""
        stats = SuccessorCacheStats()
        self.lib.sl_successor_cache_info(self.handle, C.byref(stats))
        return {name: int(getattr(stats, name)) for name, _ in SuccessorCacheStats._fields_}

    def eval_points(self, what, n, d_points, d_out):
        self.lib.sl_eval_points(self.handle, what, n, _ptr(d_points), _ptr(d_out))

    def rollout(self, lo, hi, d_start, steps, d_state, d_traj=None, d_actions=None, steps_per_launch=0):
        """``sl_rollout``: ``steps`` closed-loop steps of the trajectories ``[lo, hi)`` under the model
        (``d_start=None``: from the grid points)."""
        self.lib.sl_rollout(self.handle, lo, hi, _ptr(d_start), int(steps), int(steps_per_launch),
                            _ptr(d_state), _ptr(d_traj), _ptr(d_actions))

    def rollout_mask(self, n, d, d_state, equilibrium, tol, d_bits, d_count):
        """``sl_rollout_mask``: bit i = ``||state_i - equilibrium||_2 <= tol`` (``None``: the origin)."""
        pe = None
        if equilibrium is not None:
            equilibrium, pe = _as_c(np.ravel(equilibrium))
            if equilibrium.size != d:
                raise ValueError("equilibrium has %d entries, the states %d" % (equilibrium.size, d))
        self.lib.sl_rollout_mask(self.handle, int(n), int(d), _ptr(d_state), pe, float(tol), _ptr(d_bits),
                                 _ptr(d_count))

    def reward_rollout(self, lo, hi, d_start, horizon, d_weights, tol, d_sum, d_state, steps_per_launch=0):
        """``sl_reward_rollout``: the discounted returns of the trajectories ``[lo, hi)`` under the model
        and its quadratic reward, with the reference's stopping rule -> ``(steps, converged)``."""
        steps, converged = _i64(0), _int(0)
        self.lib.sl_reward_rollout(self.handle, lo, hi, _ptr(d_start), int(horizon), _ptr(d_weights), float(tol),
                                   int(steps_per_launch), _ptr(d_sum), _ptr(d_state), C.byref(steps),
                                   C.byref(converged))
        return int(steps.value), bool(converged.value)

    def gp_mean_points(self, n, d_inputs, d_mean):
        """``sl_gp_mean_points``: the mean of the model's GP dynamics at ``n`` explicit ``[x, u]`` rows."""
        self.lib.sl_gp_mean_points(self.handle, int(n), _ptr(d_inputs), _ptr(d_mean))

    def rollout_mean(self, lo, hi, d_start, steps, d_state, d_traj=None, d_actions=None, steps_per_launch=0):
        """``sl_rollout_mean``: :meth:`rollout` with the posterior mean of the model's GP dynamics."""
        self.lib.sl_rollout_mean(self.handle, lo, hi, _ptr(d_start), int(steps), int(steps_per_launch),
                                 _ptr(d_state), _ptr(d_traj), _ptr(d_actions))

    def reward_rollout_mean(self, lo, hi, d_start, horizon, d_weights, tol, d_sum, d_state, steps_per_launch=0):
        """``sl_reward_rollout_mean``: :meth:`reward_rollout` with the posterior mean of the model's GP
        dynamics -> ``(steps, converged)``."""
        steps, converged = _i64(0), _int(0)
        self.lib.sl_reward_rollout_mean(self.handle, lo, hi, _ptr(d_start), int(horizon), _ptr(d_weights),
                                        float(tol), int(steps_per_launch), _ptr(d_sum), _ptr(d_state),
                                        C.byref(steps), C.byref(converged))
        return int(steps.value), bool(converged.value)

    def nn_param_grad(self, m, d, d_points, d_coeff, d_grad_kernels):
        """``sl_nn_param_grad``: ``sum_i coeff_i dV(p_i)/dK_l`` of every layer of the uploaded network,
        concatenated ``[out_l][in_l]`` (the layout of ``network_set``)."""
        self.lib.sl_nn_param_grad(self.handle, int(m), int(d), _ptr(d_points), _ptr(d_coeff), _ptr(d_grad_kernels))

    def nn_loss(self, kind, m, d, d_states, d_next, d_labels_or_targets, d_class_weights, safe_level, lagrange,
                eps, d_losses, d_coeff, d_points=None):
        """``sl_nn_loss``: the three means into ``d_losses``, the coefficients of ``[x; x+]`` into
        ``d_coeff`` and that point list into ``d_points``."""
        self.lib.sl_nn_loss(self.handle, int(kind), int(m), int(d), _ptr(d_states), _ptr(d_next),
                            _ptr(d_labels_or_targets), _ptr(d_class_weights), float(safe_level), float(lagrange),
                            float(eps), _ptr(d_losses), _ptr(d_coeff), _ptr(d_points))

    def action_gradient(self, n, d_points, d_actions, d_grad, d_q=None, d_next=None):
        """``sl_action_gradient``: ``dQ/du`` of ``Q = r + gamma V(mean f)`` at ``n`` points under the
        uploaded model (``d_points=None``: the grid points, ``d_actions=None``: the policy's actions)."""
        self.lib.sl_action_gradient(self.handle, int(n), _ptr(d_points), _ptr(d_actions), _ptr(d_grad), _ptr(d_q),
                                    _ptr(d_next))

    def policy_param_grad(self, n, d, d_points, d_coeff, d_grad):
        """``sl_policy_param_grad``: ``sum_i sum_o coeff[i][o] d pi_o(p_i)/d theta`` of the uploaded network
        policy, flat in the order ``W_0, b_0, W_1, b_1, ..., W_out``."""
        self.lib.sl_policy_param_grad(self.handle, int(n), int(d), _ptr(d_points), _ptr(d_coeff), _ptr(d_grad))

    def tri_param_grad(self, slot, n, d_points, d_coeff, d_grad):
        """``sl_tri_param_grad``: the same sum for the vertex table of slot ``slot`` -> ``[nindex, cols]``."""
        self.lib.sl_tri_param_grad(self.handle, int(slot), int(n), _ptr(d_points), _ptr(d_coeff), _ptr(d_grad))

    def decrease_gradient(self, n, d_points, d_actions, d_grad, d_constraint=None, d_terms=None):
        """``sl_decrease_gradient``: ``dC/du`` of the Lyapunov constraint ``C = decrease bound - threshold``
        at ``n`` points under the uploaded model (``d_actions=None``: the policy's actions)."""
        self.lib.sl_decrease_gradient(self.handle, int(n), _ptr(d_points), _ptr(d_actions), _ptr(d_grad),
                                      _ptr(d_constraint), _ptr(d_terms))

    @staticmethod
    def _dense_description(dims, activations, has_bias):
        """The host arrays of a dense network's description (kept alive by the caller for the call)."""
        arrays = [np.ascontiguousarray(v, dtype=np.int32) for v in (dims, activations, has_bias)]
        if len(arrays[0]) != len(arrays[1]) + 1 or len(arrays[2]) != len(arrays[1]):
            raise ValueError('a network of %d layers needs %d widths and %d bias flags'
                             % (len(arrays[1]), len(arrays[1]) + 1, len(arrays[1])))
        return arrays, [a.ctypes.data_as(_int32_p) for a in arrays]

    def critic_batch(self, dims, activations, has_bias, output_scale, d_params, n, d_states, d_actions, reduction,
                     d_value, d_q, d_sums, d_next=None, d_dq_du=None, d_coeff=None):
        """``sl_critic_batch``: per sample ``V(x)``, ``q = r + gamma V(x+)``, optionally ``x+``, ``dq/du`` and the
        TD coefficient ``w sign(V(x) - q)``, and ``d_sums = (sum |V(x) - q|, sum q)`` under the uploaded model,
        for the value network ``(dims, activations, has_bias, output_scale)`` with its packed parameters in
        ``d_params``.  ``reduction``: ``'mean'`` or ``'sum'``."""
        keep, (pd, pa, pb) = self._dense_description(dims, activations, has_bias)
        self.lib.sl_critic_batch(self.handle, len(keep[1]), pd, pa, pb, float(output_scale), _ptr(d_params), int(n),
                                 _ptr(d_states), _ptr(d_actions), REDUCTIONS[reduction], _ptr(d_next), _ptr(d_value),
                                 _ptr(d_q), _ptr(d_dq_du), _ptr(d_coeff), _ptr(d_sums))

    def dense_param_grad(self, dims, activations, has_bias, output_scale, d_params, n, d, d_points, d_coeff, d_out):
        """``sl_dense_param_grad``: ``sum_i sum_o coeff[i][o] d net_o(p_i)/d theta`` of the network described by the
        arguments, flat in the order of ``d_params`` (``W_0, b_0, W_1, b_1, ...``)."""
        keep, (pd, pa, pb) = self._dense_description(dims, activations, has_bias)
        self.lib.sl_dense_param_grad(self.handle, len(keep[1]), pd, pa, pb, float(output_scale), _ptr(d_params),
                                     int(n), int(d), _ptr(d_points), _ptr(d_coeff), _ptr(d_out))

    # ---- GP sample paths (sl_gp_sample.hip) ---------------------------------------------------
    @staticmethod
    def _kernel_spec(factors, p):
        """``sl_gp_kernel`` of ``[(kind, product, variance[p], inv_lengthscales[p])]`` (``Kern._factors``)."""
        if len(factors) > KERNEL_MAX_FACTORS:
            raise ValueError("kernel with %d leaf factors (engine limit %d)" % (len(factors), KERNEL_MAX_FACTORS))
        if not 1 <= p <= MAX_INPUT_DIM:
            raise ValueError("input dimension %d (engine limit %d)" % (p, MAX_INPUT_DIM))
        spec = GpKernel()
        spec.nfactors = len(factors)
        for f, (kind, product, variance, inv_ls) in enumerate(factors):
            spec.factor[f].kind, spec.factor[f].product = int(kind), int(product)
            for q in range(p):
                spec.factor[f].variance[q] = float(variance[q])
                spec.factor[f].inv_lengthscales[q] = float(inv_ls[q])
        return spec

    def gp_posterior_cov(self, X, Linv, alpha, factors, prior, d_Z, jitter, d_mean, d_cov):
        """``sl_gp_posterior_cov``: mean ``[N]`` and covariance ``[N, N]`` (plus ``jitter`` on the diagonal) of a
        one-output GP with the host factors ``X [n, p]``, ``Linv [n, n]``, ``alpha [n]`` at the device points
        ``d_Z [N, p]``; ``prior [p]`` (the row of a linear mean function) or ``None``."""
        N, p = d_Z.shape
        X, pX = _as_c(np.reshape(X, (-1, p)))
        Linv, pL = _as_c(Linv)
        alpha, pA = _as_c(np.reshape(alpha, -1))
        spec = self._kernel_spec(factors, p)
        pp = None
        if prior is not None:
            prior, pp = _as_c(np.reshape(prior, -1))
        self.lib.sl_gp_posterior_cov(self.handle, len(X), p, pX, pL, pA, C.byref(spec), pp, N, _ptr(d_Z),
                                     float(jitter), _ptr(d_mean), _ptr(d_cov), d_cov.stride(0))

    def cholesky(self, d_A):
        """``sl_cholesky`` in place of the square device matrix ``d_A`` -> 0, or the 1-based index of the first
        pivot that is not positive (the engine's error for that case is the answer here, not an exception)."""
        info = C.c_int32(0)
        try:
            self.lib.sl_cholesky(self.handle, d_A.shape[0], _ptr(d_A), d_A.stride(0), C.byref(info))
        except HipEngineError:
            if info.value == 0:
                raise
        return int(info.value)

    def tri_solve(self, d_L, d_B, transpose=False):
        """``sl_tri_solve``: ``d_B [N, k]`` becomes ``L^-1 d_B`` (``transpose``: ``L^-T d_B``)."""
        self.lib.sl_tri_solve(self.handle, d_B.shape[0], d_B.shape[1], _ptr(d_L), d_L.stride(0), int(bool(transpose)),
                              _ptr(d_B))

    def tri_mult(self, d_L, d_Zn, d_mean, d_out):
        """``sl_tri_mult``: ``d_out [N, k] = d_mean [N] + L d_Zn`` (``d_mean=None``: no mean)."""
        self.lib.sl_tri_mult(self.handle, d_Zn.shape[0], d_Zn.shape[1], _ptr(d_L), d_L.stride(0), _ptr(d_Zn),
                             _ptr(d_mean), _ptr(d_out))

    def gp_sample_eval(self, factors, prior, d_D, d_alpha, d_points, d_out):
        """``sl_gp_sample_eval``: ``d_out [M, k] = d_points prior + K(d_points, d_D) d_alpha``."""
        N, p = d_D.shape
        spec = self._kernel_spec(factors, p)
        pp = None
        if prior is not None:
            prior, pp = _as_c(np.reshape(prior, -1))
        self.lib.sl_gp_sample_eval(self.handle, C.byref(spec), pp, p, N, _ptr(d_D), d_alpha.shape[1], _ptr(d_alpha),
                                   d_points.shape[0], _ptr(d_points), _ptr(d_out))

    # ---- GP hyper-parameters (sl_gp_likelihood.hip) --------------------------------------------
    GP_LIKELIHOOD_MAX_TRAIN = 4096          # SL_GP_SAMPLE_MAX_TRAIN

    def gp_likelihood(self, X, R, factors, noise_variance, gradient=True):
        """``sl_gp_likelihood`` -> ``(lml, grad_variance [nfactors, p], grad_inv_ls [nfactors, p], grad_noise,
        pivot)``: the log marginal likelihood of the residuals ``R [n, D]`` at the inputs ``X [n, p]`` and its
        derivatives with respect to ``variance[q]`` / ``inv_lengthscales[q]`` of every factor of ``factors``
        (``Kern._factors``) and to ``noise_variance`` (``gradient=False``: ``None`` for the three).  ``pivot`` is 0,
        or the 1-based index of the first pivot of ``K`` that is not positive; ``lml`` is then ``None``."""
        X = np.asarray(X, dtype=np.float64)
        n, p = X.shape
        if n > self.GP_LIKELIHOOD_MAX_TRAIN:
            raise ValueError("gp_likelihood: %d observations (engine limit %d)" % (n, self.GP_LIKELIHOOD_MAX_TRAIN))
        X, pX = _as_c(X)
        R, pR = _as_c(np.reshape(R, (n, 1)) if np.ndim(R) < 2 else R)
        spec = self._kernel_spec(factors, p)
        lml, noise, info = _dbl(0.0), _dbl(0.0), C.c_int32(0)
        gv = np.zeros((KERNEL_MAX_FACTORS, MAX_INPUT_DIM))
        gl = np.zeros((KERNEL_MAX_FACTORS, MAX_INPUT_DIM))
        grads = (gv.ctypes.data_as(c_double_p), gl.ctypes.data_as(c_double_p), C.byref(noise)) if gradient \
            else (None, None, None)
        try:
            self.lib.sl_gp_likelihood(self.handle, n, p, R.shape[1], pX, pR, C.byref(spec), float(noise_variance),
                                      C.byref(lml), grads[0], grads[1], grads[2], C.byref(info))
        except HipEngineError:
            if info.value == 0:
                raise
            return None, None, None, None, int(info.value)
        if not gradient:
            return float(lml.value), None, None, None, 0
        return float(lml.value), gv[:len(factors), :p].copy(), gl[:len(factors), :p].copy(), float(noise.value), 0

    def gp_lml_grad_stage(self, X, B, Kinv, factors):
        """``sl_debug_gp_lml_grad``: the tile sum of ``sl_gp_likelihood`` on a given ``B [n, D]`` and ``K^-1 [n, n]``
        -> ``(grad_variance, grad_inv_ls, grad_noise)``."""
        X = np.asarray(X, dtype=np.float64)
        n, p = X.shape
        X, pX = _as_c(X)
        B, pB = _as_c(np.reshape(B, (n, 1)) if np.ndim(B) < 2 else B)
        Kinv, pK = _as_c(np.reshape(Kinv, (n, n)))
        spec = self._kernel_spec(factors, p)
        noise = _dbl(0.0)
        gv = np.zeros((KERNEL_MAX_FACTORS, MAX_INPUT_DIM))
        gl = np.zeros((KERNEL_MAX_FACTORS, MAX_INPUT_DIM))
        self.lib.sl_debug_gp_lml_grad(self.handle, n, p, B.shape[1], pX, pB, pK, C.byref(spec),
                                      gv.ctypes.data_as(c_double_p), gl.ctypes.data_as(c_double_p), C.byref(noise))
        return gv[:len(factors), :p].copy(), gl[:len(factors), :p].copy(), float(noise.value)

    def nn_train_scratch(self):
        """``sl_debug_nn_train_scratch`` -> (bytes of the scratch area, its guard zones are intact)."""
        nbytes, intact = _i64(0), _int(0)
        self.lib.sl_debug_nn_train_scratch(self.handle, C.byref(nbytes), C.byref(intact))
        return int(nbytes.value), bool(intact.value)

    def synchronize(self):
        self.lib.sl_ctx_synchronize(self.handle)

    TIMING_LYAP_SWEEP, TIMING_FINALIZE, TIMING_BELLMAN = 0, 1, 2

    def timing_configure(self, slots):
        """``sl_timing_configure``: the library records HIP events around up to ``slots`` calls of
        each of its sweep entry points (0: off)."""
        self.lib.sl_timing_configure(self.handle, int(slots))
        self._timing_slots = int(slots)

    def timing_collect(self, channel):
        """Durations (ms) of the calls recorded on ``channel`` since the last collect."""
        slots = getattr(self, "_timing_slots", 0)
        if not slots:
            return []
        out = (C.c_double * slots)()
        count = C.c_int(0)
        self.lib.sl_timing_collect(self.handle, int(channel), out, slots, C.byref(count))
        return [float(out[i]) for i in range(count.value)]

    def last_kernel(self):
        """Name of the kernel(s) the last sweep of this context launched (``sl_last_kernel``)."""
        name = self.lib.sl_last_kernel(self.handle)
        return name.decode() if name else ""

    def gp4_open_list(self, entries=True):
        """``(list, used)`` of the last sweep (``sl_gp4_open_list``): the 16-cell blocks its deciding pass
        left open as a ``uint32`` array of block numbers (``entries=False``: only their number, an int), and
        whether the mean pass ran from that list."""
        import numpy as np
        count, used = C.c_ulonglong(0), C.c_int(0)
        self.lib.sl_gp4_open_list(self.handle, None, 0, C.byref(count), C.byref(used))
        if not entries:
            return int(count.value), bool(used.value)
        out = np.zeros(int(count.value), dtype=np.uint32)
        if len(out):
            self.lib.sl_gp4_open_list(self.handle, out.ctypes.data_as(C.POINTER(C.c_uint32)), len(out),
                                      C.byref(count), C.byref(used))
        return out, bool(used.value)

    # ---- RCCL collectives of the C ABI (the package itself uses torch.distributed) ---------
    @staticmethod
    def comm_unique_id():
        lib = load_library()
        buf = C.create_string_buffer(128)
        rc = lib.sl_comm_unique_id(buf)
        if rc != 0:
            raise HipEngineError("sl_comm_unique_id failed: %s" % lib.sl_last_error(None).decode())
        return buf.raw

    def comm_init(self, unique_id, rank, world):
        self.lib.sl_comm_init(self.handle, unique_id, rank, world)

    def comm_destroy(self):
        self.lib.sl_comm_destroy(self.handle)

    def allreduce_result(self, d_result):
        self.lib.sl_allreduce_result(self.handle, _ptr(d_result))

    def allgather(self, d_send, d_recv, nbytes):
        self.lib.sl_allgather(self.handle, _ptr(d_send), _ptr(d_recv), nbytes)

    def allreduce_sum_u64(self, d_values, count):
        self.lib.sl_allreduce_sum_u64(self.handle, _ptr(d_values), count)

    def allreduce_max_f64(self, d_values, count):
        self.lib.sl_allreduce_max_f64(self.handle, _ptr(d_values), count)

    # ---- diagnostics ---------------------------------------------------------------------
    def debug_mfma(self, a, b):
        a, pa = _as_c(a)
        b, pb = _as_c(b)
        out = np.zeros((16, 16))
        self.lib.sl_debug_mfma(self.handle, pa, pb, out.ctypes.data_as(c_double_p))
        return out

    def debug_mfma4(self, a, b, c, mode=0):
        """v_mfma_f64_4x4x4_4b_f64 on per-lane operands of shape (nwaves, 64)."""
        a, pa = _as_c(np.atleast_2d(a))
        b, pb = _as_c(np.atleast_2d(b))
        c, pc = _as_c(np.atleast_2d(c))
        out = np.zeros_like(a)
        self.lib.sl_debug_mfma4(self.handle, a.shape[0], pa, pb, pc, mode, out.ctypes.data_as(c_double_p))
        return out

    def debug_fp64_rate(self, which, iters=20000):
        out = (C.c_double * 3)()
        self.lib.sl_debug_fp64_rate(self.handle, which, iters, out)
        return {"tflops": out[0], "shader_mhz": out[1], "cycles_per_slot": out[2]}


_default_context = None


def default_context():
    """Process-wide context on torch's current device."""
    global _default_context
    if _default_context is None:
        _default_context = Context()
    return _default_context
