"""Python binding of libipmz (the MI355X Newton-step library) over its C ABI
(include/ipmz.h), via ctypes.

Mirrors the reference's NumericalOptimization interface for the hot path:

    LinearSolvers.ldlt_decomposition(A)        -> (L, D)   LinearSolvers.h:11
    LinearSolvers.overwriting_solve_ldlt(L, D, b)  (b overwritten)  LinearSolvers.h:16-17
    Data / build_environment / Optimizer(...).solve()     EnvironmentBuilder.h:7-20,
                                                           Optimizer.h:15-20

Errors raise AssertionError (a subclass of the reference's
Utils::AssertionError -> std::logic_error convention, Assert.h:7-12, maps to
Python's AssertionError/ValueError family here).  There is no CPU fallback:
loading fails loudly when lib/libipmz.so is missing, and every computing
call fails when no gfx950 device is visible.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(HERE), "lib", "libipmz.so")

IPMZ_OK = 0
ERR = {-1: "invalid argument", -2: "HIP error", -3: "out of device memory", -4: "no gfx950 device",
       -5: "bad state"}
SC = dict(f=0, res=1, mu=2, alpha_aff=3, mu_aff=4, sigma=5, alpha=6, converged=7, mu_new=8, restarts=9,
          ir_ratio_aff=10, ir_iters_aff=11, ir_ratio=12, ir_iters=13, steps=14)
SC_COUNT = 16
PH = dict(step=0, assemble=1, factor=2, solve=3, trailing=4, eval=5)
STEP_RESTART_IF_CONVERGED = 1
STEP_GRAPH = 2
STEP_SKIP_CONVERGED = 4  # include/ipmz.h IPMZ_STEP_SKIP_CONVERGED: converged QPs of a batch take no part in the step
SET_STATE_UNCHECKED = 1  # include/ipmz.h IPMZ_SET_STATE_UNCHECKED
SLOTS = ["x", "lambda_A", "lambda_C", "s", "p", "lambda_g", "lambda_h", "lambda_y", "lambda_z", "g", "h", "y", "z"]

EXPORTS = [
    "ipmz_ctx_create", "ipmz_ctx_destroy", "ipmz_ctx_set_stream", "ipmz_ctx_reset_stream", "ipmz_ctx_sync", "ipmz_last_error",
    "ipmz_ctx_set_blocking", "ipmz_ctx_get_blocking", "ipmz_ldlt_workspace_bytes", "ipmz_ldlt_factor", "ipmz_ldlt_solve",
    "ipmz_ldlt_prepare_solve", "ipmz_ldlt_decomposition", "ipmz_overwriting_solve_ldlt", "ipmz_qp_create",
    "ipmz_qp_destroy", "ipmz_qp_load_host", "ipmz_qp_generate", "ipmz_qp_step", "ipmz_qp_scalars",
    "ipmz_qp_device_scalars", "ipmz_qp_copy_scalars", "ipmz_qp_solve", "ipmz_qp_state_len", "ipmz_qp_get_state", "ipmz_qp_set_state",
    "ipmz_qp_get_kkt", "ipmz_qp_kkt_dim", "ipmz_qp_set_timing", "ipmz_qp_phase_times",
    "ipmz_batch_create", "ipmz_batch_size", "ipmz_batch_load_host", "ipmz_batch_initialize", "ipmz_batch_scalars",
    "ipmz_batch_get_state", "ipmz_batch_set_state", "ipmz_batch_solve",
    "ipmz_mixed_workspace_bytes", "ipmz_mixed_factor", "ipmz_mixed_solve", "ipmz_qp_set_mixed_precision",
    "ipmz_batch_copy_scalars", "ipmz_normal_workspace_bytes", "ipmz_normal_factor", "ipmz_normal_solve",
    "ipmz_qp_set_reduction", "ipmz_bk_factor", "ipmz_bk_factor_ex", "ipmz_bk_solve", "ipmz_symmetric_indefinite_factorization",
    "ipmz_overwriting_solve_bunch_kaufman", "ipmz_debug_inject", "ipmz_batch_summary", "ipmz_batch_set_factor_kernel",
    "ipmz_qp_last_step_graph", "ipmz_ldlt_solve_multi", "ipmz_overwriting_solve_ldlt_multi", "ipmz_qp_kkt_solve",
    "ipmz_mixed_multi_workspace_bytes", "ipmz_mixed_solve_multi", "ipmz_sym_residual_multi", "ipmz_qp_kkt_solve_mixed",
    "ipmz_bk_solve_workspace_bytes", "ipmz_bk_prepare_solve", "ipmz_bk_solve_multi",
    "ipmz_overwriting_solve_bunch_kaufman_multi", "ipmz_normal_solve_multi", "ipmz_qp_kkt_solve_bk",
    "ipmz_batch_get_kkt", "ipmz_batch_kkt_solve",
    "ipmz_bk_factor_batch", "ipmz_bk_batch_solve_workspace_bytes", "ipmz_bk_prepare_solve_batch",
    "ipmz_bk_solve_multi_batch", "ipmz_batch_kkt_solve_bk",
    "ipmz_qp_newton_solve_multi", "ipmz_batch_newton_solve_multi",
    "ipmz_qp_newton_adjoint_multi", "ipmz_batch_newton_adjoint_multi",
    "ipmz_batch_load_device", "ipmz_batch_copy_state", "ipmz_batch_data_vjp", "ipmz_batch_data_jvp",
    "ipmz_batch_data_vjp_multi", "ipmz_batch_set_state_device", "ipmz_qp_get_factor",
    "ipmz_batch_solve_ex", "ipmz_batch_can_skip_converged", "ipmz_batch_center",
]
SOLVE_MULTI_PANEL = 256  # include/ipmz.h IPMZ_SOLVE_MULTI_PANEL: column panel of the blocked multi-rhs solve
REDUCTION_AUGMENTED, REDUCTION_NORMAL = 0, 1

_P = ctypes.POINTER(ctypes.c_double)
_VP = ctypes.c_void_p
_I = ctypes.c_int
_I64 = ctypes.c_int64


class IpmzError(AssertionError):
    """A failed libipmz call (the reference throws Utils::AssertionError)."""


EQ_REGULARIZATION = 0  # Settings::EqualityHandling::Regularization (include/ipmz.h IPMZ_EQ_*)
EQ_NONE = 1            # zero (lambda_C, lambda_C) block, Bunch-Kaufman factor
EQ_PENALTY = 2         # PenaltyFunction: -mu (lambda_C, lambda_C) block, LDL^T
EQ_PENALTY_EXTRA_DUAL = 3  # PenaltyFunctionWithExtraDual: the same Newton system (reference-derived)
EQ_SLACKED_SLACKS = 4  # t, v = t - d, w = d - t with duals lambda_v, lambda_w (SlackedSlacks inequalities)
EQ_NAIVE_SLACKS = 5    # C x - v = d, C x + w = d, lambda_v / lambda_w as KKT rows (NaiveSlacks inequalities)
INEQ_SLACKED_SLACKS = 0  # Settings::InequalityHandling (include/ipmz.h IPMZ_INEQ_*)
INEQ_SLACKS = 1          # no g/h/y/z slacks (the reference's corrector defect reproduced)
INEQ_NAIVE_SLACKS = 2    # no s; lambda_g, lambda_h as KKT rows (N = n + 2m + p)
BOUNDS_BOTH = 0          # Settings::Bounds (include/ipmz.h IPMZ_BOUNDS_*)
BOUNDS_LOWER = 1
BOUNDS_UPPER = 2
BOUNDS_NONE = 3


class _QPConfig(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int), ("m", ctypes.c_int), ("p", ctypes.c_int), ("delta", ctypes.c_double),
                ("equality_handling", ctypes.c_int), ("inequality_handling", ctypes.c_int),
                ("inequality_bounds", ctypes.c_int), ("variable_bounds", ctypes.c_int)]


class _QPDeviceData(ctypes.Structure):
    """include/ipmz.h ipmz_qp_device_data: device pointers, strides in elements."""
    _fields_ = [("Q", _VP), ("ldq", _I64), ("sQ", _I64), ("A", _VP), ("lda", _I64), ("sA", _I64),
                ("C", _VP), ("ldc", _I64), ("sC", _I64), ("c", _VP), ("l_x", _VP), ("u_x", _VP),
                ("sc", _I64), ("slx", _I64), ("sux", _I64), ("l_A", _VP), ("u_A", _VP), ("slA", _I64), ("suA", _I64),
                ("d", _VP), ("sd", _I64)]


class _QPDeviceGrad(_QPDeviceData):
    """include/ipmz.h ipmz_qp_device_grad: the same layout, the blocks written (ipmz_batch_data_vjp)."""


class _QPDeviceGradMulti(ctypes.Structure):
    """include/ipmz.h ipmz_qp_device_grad_multi: the blocks plus a cotangent-row stride each
    (ipmz_batch_data_vjp_multi)."""
    _fields_ = [("g", _QPDeviceGrad)] + [(k, _I64) for k in ("tQ", "tA", "tC", "tc", "tlx", "tux", "tlA", "tuA", "td")]


class _QPDeviceTangent(ctypes.Structure):
    """include/ipmz.h ipmz_qp_device_tangent: the blocks plus a tangent stride each (ipmz_batch_data_jvp)."""
    _fields_ = [("d", _QPDeviceData)] + [(k, _I64) for k in ("tQ", "tA", "tC", "tc", "tlx", "tux", "tlA", "tuA", "td")]


# load_tensors' names -> (ipmz_qp_device_data pointer, row stride or None, QP stride, rows or None, columns);
# rows / columns name the solver's dimensions.  The order is csrc/kernels.h DATA_BLOCKS'; ipmz_qp_device_tangent's
# tangent stride of block X is its QP stride's name sX with a t (_set_block)
_BLOCKS = (("Q", "Q", "ldq", "sQ", "n", "n"), ("A_ineq", "A", "lda", "sA", "m", "n"), ("A_eq", "C", "ldc", "sC", "p", "n"),
           ("c", "c", None, "sc", None, "n"), ("l_x", "l_x", None, "slx", None, "n"), ("u_x", "u_x", None, "sux", None, "n"),
           ("l_A_ineq", "l_A", None, "slA", None, "m"), ("u_A_ineq", "u_A", None, "suA", None, "m"),
           ("b_eq", "d", None, "sd", None, "p"))


def _tensor_block(t, batch, rows, cols, tangent=False):
    """A torch tensor as one block of ipmz_qp_device_data: (data_ptr, row stride, QP stride), strides in elements.

    rows is None for a vector block -- t of shape (batch, cols), or (cols,) shared by every QP -- else the block is
    a matrix: (batch, rows, cols), or (rows, cols) shared.  A shared block, and one expanded along the batch
    dimension (batch stride 0), has QP stride 0.  Nothing is copied: the strides go to the kernel as they are.
    tangent: one block of ipmz_qp_device_tangent -- the same rules with a tangent dimension after the batch's,
    (batch, ntan, ...) per QP or (ntan, ...) shared -- as (data_ptr, row stride, QP stride, tangent stride, ntan).
    ValueError for a dtype other than float64, another shape, or an inner stride other than 1."""
    import torch
    name, what = "matrix" if rows is not None else "vector", "tangent" if tangent else "block"
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64:
        raise ValueError(f"{name} {what}: a float64 torch tensor is needed, got {getattr(t, 'dtype', type(t))}")
    inner = (cols,) if rows is None else (rows, cols)
    shape = tuple(t.shape)
    lead = len(shape) - len(inner)  # the dimensions before the block's: [batch][ntan]
    per_qp = lead == tangent + 1
    if not (per_qp or lead == tangent) or shape[lead:] != inner or (per_qp and shape[0] != batch):
        tan = ("ntan",) if tangent else ()
        raise ValueError(f"{name} {what}: shape {shape} is neither {(batch,) + tan + inner} nor {tan + inner}")
    strides = t.stride()
    sq = strides[0] if per_qp and batch > 1 else 0
    if cols > 1 and strides[-1] != 1:
        raise ValueError(f"{name} {what}: inner stride {strides[-1]}, must be 1 (elements of a row adjacent)")
    # (the stride of a dimension of size 1 means nothing: a single row is given the row length)
    ld = 0 if rows is None else (strides[lead] if rows > 1 else max(strides[lead], cols))
    if not tangent:
        return t.data_ptr(), ld, sq
    ntan = shape[lead - 1]
    return t.data_ptr(), ld, sq, (strides[lead - 1] if ntan > 1 else 0), ntan


def _set_block(d, fields, blk, tan=None):
    """One block -- fields: its row of _BLOCKS, blk: _tensor_block's tuple -- into the ipmz_qp_device_data d, and
    its tangent stride into tan: block X's tangent stride tX is its QP stride sX renamed."""
    _, ptr, ld, sq, _, _ = fields
    setattr(d, ptr, blk[0])
    if ld:
        setattr(d, ld, blk[1])
    setattr(d, sq, blk[2])
    if tan is not None:
        setattr(tan, "t" + sq[1:], blk[3])


def _load():
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64, and
    # a second copy loaded next to it cannot open the device.  Loading torch
    # first makes libipmz bind to torch's copy (same soname), so device
    # pointers and streams are shared.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"libipmz not built: {LIB_PATH} missing (run __graft_entry__.build()); "
                          "there is no CPU fallback")
    lib = ctypes.CDLL(LIB_PATH)
    sig = {
        "ipmz_ctx_create": ([ctypes.POINTER(_VP), _I], _I),
        "ipmz_ctx_destroy": ([_VP], _I),
        "ipmz_ctx_set_stream": ([_VP, _VP], _I),
        "ipmz_ctx_reset_stream": ([_VP], _I),
        "ipmz_ctx_sync": ([_VP], _I),
        "ipmz_last_error": ([], ctypes.c_char_p),
        "ipmz_ctx_set_blocking": ([_VP, _I, _I], _I),
        "ipmz_ctx_get_blocking": ([_VP, _I, ctypes.POINTER(_I), ctypes.POINTER(_I)], _I),
        "ipmz_ldlt_workspace_bytes": ([_VP, _I], _I64),
        "ipmz_ldlt_factor": ([_VP, _I, _VP, _I64, _VP, _VP, _I64], _I),
        "ipmz_ldlt_solve": ([_VP, _I, _VP, _I64, _VP, _VP, _VP], _I),
        "ipmz_ldlt_prepare_solve": ([_VP, _I, _VP, _I64, _VP, _I64], _I),
        "ipmz_ldlt_decomposition": ([_VP, _I, _P, _P, _P], _I),
        "ipmz_overwriting_solve_ldlt": ([_VP, _I, _P, _P, _P], _I),
        "ipmz_qp_create": ([_VP, ctypes.POINTER(_QPConfig), ctypes.POINTER(_VP)], _I),
        "ipmz_qp_destroy": ([_VP], _I),
        "ipmz_qp_load_host": ([_VP] + [_P] * 9, _I),
        "ipmz_qp_generate": ([_VP, ctypes.c_uint64], _I),
        "ipmz_qp_step": ([_VP, _I], _I),
        "ipmz_qp_scalars": ([_VP, _P], _I),
        "ipmz_qp_device_scalars": ([_VP, ctypes.POINTER(_VP)], _I),
        "ipmz_qp_copy_scalars": ([_VP, _VP], _I),
        "ipmz_qp_solve": ([_VP, _I, _P, ctypes.POINTER(_I)], _I),
        "ipmz_qp_state_len": ([_VP], _I64),
        "ipmz_qp_get_state": ([_VP, _I, _P], _I),
        "ipmz_qp_set_state": ([_VP, _P], _I),
        "ipmz_qp_get_kkt": ([_VP, _P], _I),
        "ipmz_qp_kkt_dim": ([_VP], _I),
        "ipmz_qp_get_factor": ([_VP, _P, _P, _P, ctypes.POINTER(_I64)], _I),
        "ipmz_qp_set_timing": ([_VP, _I], _I),
        "ipmz_qp_phase_times": ([_VP, _P, _P, ctypes.POINTER(_I64)], _I),
        "ipmz_batch_create": ([_VP, ctypes.POINTER(_QPConfig), _I, ctypes.POINTER(_VP)], _I),
        "ipmz_batch_size": ([_VP], _I),
        "ipmz_batch_load_host": ([_VP, _I] + [_P] * 9, _I),
        "ipmz_batch_initialize": ([_VP], _I),
        "ipmz_batch_scalars": ([_VP, _P], _I),
        "ipmz_batch_get_state": ([_VP, _I, _I, _P], _I),
        "ipmz_batch_set_state": ([_VP, _I, _P], _I),
        "ipmz_batch_solve": ([_VP, _I, ctypes.POINTER(_I), ctypes.POINTER(_I)], _I),
        "ipmz_mixed_workspace_bytes": ([_VP, _I], _I64),
        "ipmz_mixed_factor": ([_VP, _I, _VP, _I64, _VP, _I64], _I),
        "ipmz_mixed_solve": ([_VP, _I, _VP, _I64, _VP, _VP, ctypes.c_double, _I, _P], _I),
        "ipmz_qp_set_mixed_precision": ([_VP, _I, ctypes.c_double, _I], _I),
        "ipmz_batch_copy_scalars": ([_VP, _VP], _I),
        "ipmz_normal_workspace_bytes": ([_VP, _I, _I], _I64),
        "ipmz_normal_factor": ([_VP, _I, _I, _VP, _I64, _VP, _VP, _I64], _I),
        "ipmz_normal_solve": ([_VP, _I, _I, _VP, _I64, _VP, _VP, _VP], _I),
        "ipmz_qp_set_reduction": ([_VP, _I], _I),
        "ipmz_bk_factor": ([_VP, _I, _VP, _I64, _VP, _I], _I),
        "ipmz_bk_factor_ex": ([_VP, _I, _VP, _I64, _VP, _I, _I], _I),
        "ipmz_bk_solve": ([_VP, _I, _VP, _I64, _VP, _VP], _I),
        "ipmz_symmetric_indefinite_factorization": ([_VP, _I, _P, _P, ctypes.POINTER(ctypes.c_int)], _I),
        "ipmz_overwriting_solve_bunch_kaufman": ([_VP, _I, _P, ctypes.POINTER(ctypes.c_int), _P], _I),
        "ipmz_debug_inject": ([_I], _I),
        "ipmz_batch_summary": ([_VP, _VP], _I),
        "ipmz_batch_set_factor_kernel": ([_VP, _I], _I),
        "ipmz_qp_last_step_graph": ([_VP], _I),
        "ipmz_ldlt_solve_multi": ([_VP, _I, _VP, _I64, _VP, _VP, _VP, _I64, _I], _I),
        "ipmz_overwriting_solve_ldlt_multi": ([_VP, _I, _P, _P, _P, _I], _I),
        "ipmz_qp_kkt_solve": ([_VP, _I, _VP, _I64], _I),
        "ipmz_mixed_multi_workspace_bytes": ([_VP, _I, _I], _I64),
        "ipmz_mixed_solve_multi": ([_VP, _I, _VP, _I64, _VP, _VP, _I64, _I, ctypes.c_double, _I, _VP, _I64, _P], _I),
        "ipmz_sym_residual_multi": ([_VP, _I, _VP, _I64, _VP, _I64, _VP, _I64, _VP, _I64, _I], _I),
        "ipmz_qp_kkt_solve_mixed": ([_VP, _I, _VP, _I64, ctypes.c_double, _I, _P], _I),
        "ipmz_bk_solve_workspace_bytes": ([_VP, _I], _I64),
        "ipmz_bk_prepare_solve": ([_VP, _I, _VP, _I64, _VP, _VP, _I64], _I),
        "ipmz_bk_solve_multi": ([_VP, _I, _VP, _I64, _VP, _VP, _VP, _I64, _I], _I),
        "ipmz_overwriting_solve_bunch_kaufman_multi": ([_VP, _I, _P, ctypes.POINTER(ctypes.c_int), _P, _I], _I),
        "ipmz_normal_solve_multi": ([_VP, _I, _I, _VP, _I64, _VP, _VP, _VP, _I64, _I], _I),
        "ipmz_qp_kkt_solve_bk": ([_VP, _I, _VP, _I64], _I),
        "ipmz_batch_get_kkt": ([_VP, _I, _P], _I),
        "ipmz_batch_kkt_solve": ([_VP, _I, _VP, _I64, _I64], _I),
        "ipmz_bk_factor_batch": ([_VP, _I, _I, _VP, _I64, _I64, _VP, _I64, _I, ctypes.POINTER(_I)], _I),
        "ipmz_bk_batch_solve_workspace_bytes": ([_VP, _I, _I], _I64),
        "ipmz_bk_prepare_solve_batch": ([_VP, _I, _I, _VP, _I64, _I64, _VP, _I64, _VP, _I64], _I),
        "ipmz_bk_solve_multi_batch": ([_VP, _I, _I, _VP, _I64, _I64, _VP, _I64, _VP, _VP, _I64, _I64, _I], _I),
        "ipmz_batch_kkt_solve_bk": ([_VP, _I, _VP, _I64, _I64, ctypes.POINTER(_I)], _I),
        "ipmz_qp_newton_solve_multi": ([_VP, _I, _VP, _I64, _VP, _I64, _VP], _I),
        "ipmz_batch_newton_solve_multi": ([_VP, _I, _VP, _I64, _I64, _VP, _I64, _I64, _VP, ctypes.POINTER(_I)], _I),
        "ipmz_qp_newton_adjoint_multi": ([_VP, _I, _VP, _I64, _VP, _I64], _I),
        "ipmz_batch_newton_adjoint_multi": ([_VP, _I, _VP, _I64, _I64, _VP, _I64, _I64, ctypes.POINTER(_I)], _I),
        "ipmz_batch_load_device": ([_VP, ctypes.POINTER(_QPDeviceData)], _I),
        "ipmz_batch_copy_state": ([_VP, _I, _VP, _I64], _I),
        "ipmz_batch_data_vjp": ([_VP, _VP, _I64, ctypes.POINTER(_QPDeviceGrad)], _I),
        "ipmz_batch_data_jvp": ([_VP, _I, ctypes.POINTER(_QPDeviceTangent), _VP, _I64, _I64], _I),
        "ipmz_batch_data_vjp_multi": ([_VP, _I, _VP, _I64, _I64, ctypes.POINTER(_QPDeviceGradMulti)], _I),
        "ipmz_batch_set_state_device": ([_VP, _VP, _I64, _VP, ctypes.c_double, _I], _I),
        "ipmz_batch_solve_ex": ([_VP, _I, _I, _I, ctypes.POINTER(_I), ctypes.POINTER(_I)], _I),
        "ipmz_batch_can_skip_converged": ([_VP], _I),
        "ipmz_batch_center": ([_VP, ctypes.c_double, ctypes.c_double, _I, ctypes.POINTER(_I), ctypes.POINTER(_I)], _I),
    }
    for name, (args, res) in sig.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    return lib


lib = _load()


def _check(rc, what):
    if rc < 0:
        msg = lib.ipmz_last_error().decode(errors="replace")
        raise IpmzError(f"{what}: {ERR.get(rc, rc)}: {msg}")
    return rc


def _dp(a):
    return a.ctypes.data_as(_P)


class Context:
    """A device + HIP stream (one per GPU / process)."""

    def __init__(self, device=0, stream=None, nbo=None, nbi=None):
        h = _VP()
        _check(lib.ipmz_ctx_create(ctypes.byref(h), device), "ipmz_ctx_create")
        self.h = h
        self.device = device
        self.stream = None  # None: the context's own (non-blocking) stream
        if stream is not None:
            self.set_stream(stream)
        if nbo or nbi:  # nbo 0 / None: by matrix order (libipmz's default)
            self.set_blocking(nbo or 0, nbi or 64)

    def set_stream(self, stream):
        """Enqueue on an external HIP stream handle (0 = the null stream,
        which is PyTorch's default stream); None = the context's own stream."""
        if stream is None:
            _check(lib.ipmz_ctx_reset_stream(self.h), "ipmz_ctx_reset_stream")
        else:
            _check(lib.ipmz_ctx_set_stream(self.h, _VP(stream)), "ipmz_ctx_set_stream")
        self.stream = stream

    def on_stream(self, stream):
        """True when work enqueued on this context is ordered before later
        work on the HIP stream handle `stream` (the same stream)."""
        return self.stream is not None and int(self.stream) == int(stream)

    def set_blocking(self, nbo, nbi):
        _check(lib.ipmz_ctx_set_blocking(self.h, nbo, nbi), "ipmz_ctx_set_blocking")

    def blocking(self, N):
        """(nbo, nbi) an order-N factor uses with this context."""
        nbo, nbi = _I(0), _I(0)
        _check(lib.ipmz_ctx_get_blocking(self.h, N, ctypes.byref(nbo), ctypes.byref(nbi)), "ipmz_ctx_get_blocking")
        return nbo.value, nbi.value

    def sync(self):
        """Synchronize; raises IpmzError when the last device-memory factor /
        solve hit a hand-off timeout (its sticky error words)."""
        _check(lib.ipmz_ctx_sync(self.h), "ipmz_ctx_sync")

    def close(self):
        if getattr(self, "h", None):
            lib.ipmz_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- device-memory LinearSolvers (pointers, e.g. torch tensor data_ptr()) --
    def workspace_bytes(self, N):
        return lib.ipmz_ldlt_workspace_bytes(self.h, N)

    def ldlt_factor(self, N, K_ptr, ld, D_ptr, ws_ptr, ws_bytes):
        return _check(lib.ipmz_ldlt_factor(self.h, N, _VP(K_ptr), ld, _VP(D_ptr), _VP(ws_ptr), ws_bytes),
                      "ipmz_ldlt_factor")

    def ldlt_solve(self, N, K_ptr, ld, D_ptr, ws_ptr, b_ptr):
        return _check(lib.ipmz_ldlt_solve(self.h, N, _VP(K_ptr), ld, _VP(D_ptr), _VP(ws_ptr), _VP(b_ptr)),
                      "ipmz_ldlt_solve")

    def ldlt_solve_multi(self, N, K_ptr, ld, D_ptr, ws_ptr, B_ptr, ldb, nrhs):
        """Every row of B (nrhs rows of length N, stride ldb, device) <- K^{-1} row, in place."""
        return _check(lib.ipmz_ldlt_solve_multi(self.h, N, _VP(K_ptr), ld, _VP(D_ptr), _VP(ws_ptr), _VP(B_ptr), ldb,
                                                nrhs), "ipmz_ldlt_solve_multi")

    # -- mixed precision (C5): fp32 factor of S K S + fp64 refinement --
    def mixed_workspace_bytes(self, N):
        return lib.ipmz_mixed_workspace_bytes(self.h, N)

    def mixed_factor(self, N, K_ptr, ld, ws_ptr, ws_bytes):
        return _check(lib.ipmz_mixed_factor(self.h, N, _VP(K_ptr), ld, _VP(ws_ptr), ws_bytes), "ipmz_mixed_factor")

    def mixed_solve(self, N, K_ptr, ld, ws_ptr, b_ptr, tol=1e-12, max_refine=10):
        """b <- K^{-1} b (device pointers); returns (ratio reached, corrections)."""
        stat = np.zeros(2)
        _check(lib.ipmz_mixed_solve(self.h, N, _VP(K_ptr), ld, _VP(ws_ptr), _VP(b_ptr), tol, max_refine, _dp(stat)),
               "ipmz_mixed_solve")
        return float(stat[0]), int(stat[1])

    def mixed_multi_workspace_bytes(self, N, nrhs):
        return lib.ipmz_mixed_multi_workspace_bytes(self.h, N, nrhs)

    def mixed_solve_multi(self, N, K_ptr, ld, ws_ptr, B_ptr, ldb, nrhs, mws_ptr, mws_bytes, tol=1e-12, max_refine=10):
        """Every row of B (nrhs rows of length N, stride ldb, device) <- K^{-1} row through the
        fp32 factor in ws; mws: mixed_multi_workspace_bytes(N, nrhs) bytes.  Blocks the host.
        Returns an (nrhs, 2) array of {ratio reached, corrections applied} per row."""
        stat = np.zeros((max(nrhs, 0), 2))
        _check(lib.ipmz_mixed_solve_multi(self.h, N, _VP(K_ptr), ld, _VP(ws_ptr), _VP(B_ptr), ldb, nrhs, tol,
                                          max_refine, _VP(mws_ptr), mws_bytes, _dp(stat)), "ipmz_mixed_solve_multi")
        return stat

    def sym_residual_multi(self, N, K_ptr, ld, X_ptr, ldx, B_ptr, ldb, R_ptr, ldr, nrhs):
        """R = B - X K for nrhs rows (device, asynchronous), K symmetric from its lower triangle;
        R may alias B."""
        return _check(lib.ipmz_sym_residual_multi(self.h, N, _VP(K_ptr), ld, _VP(X_ptr), ldx, _VP(B_ptr), ldb,
                                                  _VP(R_ptr), ldr, nrhs), "ipmz_sym_residual_multi")

    # -- Bunch-Kaufman on device memory (f3) --
    BK_AUTO, BK_WORKGROUP, BK_GRID = 0, 1, 2

    def bk_factor(self, N, A_ptr, ld, ipiv_ptr, fix_kp=False, algo=0):
        """symmetric_indefinite_factorization in place (LinearSolvers.cpp:76-207);
        algo: BK_AUTO, BK_WORKGROUP (one workgroup, N <= 4096) or BK_GRID (every CU)."""
        return _check(lib.ipmz_bk_factor_ex(self.h, N, _VP(A_ptr), ld, _VP(ipiv_ptr), int(fix_kp), int(algo)),
                      "ipmz_bk_factor")

    def bk_solve(self, N, F_ptr, ld, ipiv_ptr, b_ptr):
        return _check(lib.ipmz_bk_solve(self.h, N, _VP(F_ptr), ld, _VP(ipiv_ptr), _VP(b_ptr)), "ipmz_bk_solve")

    def bk_solve_workspace_bytes(self, N):
        return lib.ipmz_bk_solve_workspace_bytes(self.h, N)

    def bk_prepare_solve(self, N, F_ptr, ld, ipiv_ptr, ws_ptr, ws_bytes):
        """Once per factor: the prepared solve of bk_solve_multi, built in ws from bk_factor's F and ipiv."""
        return _check(lib.ipmz_bk_prepare_solve(self.h, N, _VP(F_ptr), ld, _VP(ipiv_ptr), _VP(ws_ptr), ws_bytes),
                      "ipmz_bk_prepare_solve")

    def bk_solve_multi(self, N, F_ptr, ld, ipiv_ptr, ws_ptr, B_ptr, ldb, nrhs):
        """Every row of B (device, nrhs rows, stride ldb) <- A^{-1} row, from the prepared solve in ws."""
        return _check(lib.ipmz_bk_solve_multi(self.h, N, _VP(F_ptr), ld, _VP(ipiv_ptr), _VP(ws_ptr), _VP(B_ptr), ldb,
                                              nrhs), "ipmz_bk_solve_multi")

    # -- batches of Bunch-Kaufman systems of one order (N <= 4096, one workgroup per matrix) --
    def bk_factor_batch(self, N, batch, A_ptr, ld, sA, ipiv_ptr, sP, fix_kp=False):
        """bk_factor(algo=BK_WORKGROUP) of every matrix A + q * sA (pivots at ipiv + q * sP) in one
        launch; returns (the smallest non-zero info word or 0, the per-matrix info words)."""
        info = np.zeros(max(batch, 0), dtype=np.int32)
        rc = _check(lib.ipmz_bk_factor_batch(self.h, N, batch, _VP(A_ptr), ld, sA, _VP(ipiv_ptr), sP, int(fix_kp),
                                             info.ctypes.data_as(ctypes.POINTER(_I))), "ipmz_bk_factor_batch")
        return rc, info

    def bk_batch_solve_workspace_bytes(self, N, batch):
        return lib.ipmz_bk_batch_solve_workspace_bytes(self.h, N, batch)

    def bk_prepare_solve_batch(self, N, batch, F_ptr, ld, sA, ipiv_ptr, sP, ws_ptr, ws_bytes):
        """Once per batch of factors: the prepared solves of bk_solve_multi_batch, built in ws."""
        return _check(lib.ipmz_bk_prepare_solve_batch(self.h, N, batch, _VP(F_ptr), ld, sA, _VP(ipiv_ptr), sP,
                                                      _VP(ws_ptr), ws_bytes), "ipmz_bk_prepare_solve_batch")

    def bk_solve_multi_batch(self, N, batch, F_ptr, ld, sA, ipiv_ptr, sP, ws_ptr, B_ptr, ldb, sB, nrhs):
        """For every system q: the nrhs rows at B + q * sB (device, row stride ldb) <- A_q^{-1} row,
        from the prepared solves in ws; in place, asynchronous."""
        return _check(lib.ipmz_bk_solve_multi_batch(self.h, N, batch, _VP(F_ptr), ld, sA, _VP(ipiv_ptr), sP,
                                                    _VP(ws_ptr), _VP(B_ptr), ldb, sB, nrhs),
                      "ipmz_bk_solve_multi_batch")

    # -- normal equations (C2) --
    def normal_workspace_bytes(self, n, mp):
        return lib.ipmz_normal_workspace_bytes(self.h, n, mp)

    def normal_factor(self, n, mp, K_ptr, ld, D_ptr, ws_ptr, ws_bytes):
        return _check(lib.ipmz_normal_factor(self.h, n, mp, _VP(K_ptr), ld, _VP(D_ptr), _VP(ws_ptr), ws_bytes),
                      "ipmz_normal_factor")

    def normal_solve(self, n, mp, K_ptr, ld, D_ptr, ws_ptr, b_ptr):
        return _check(lib.ipmz_normal_solve(self.h, n, mp, _VP(K_ptr), ld, _VP(D_ptr), _VP(ws_ptr), _VP(b_ptr)),
                      "ipmz_normal_solve")

    def normal_solve_multi(self, n, mp, K_ptr, ld, D_ptr, ws_ptr, B_ptr, ldb, nrhs):
        """normal_solve for every row of B (device, nrhs rows, stride ldb)."""
        return _check(lib.ipmz_normal_solve_multi(self.h, n, mp, _VP(K_ptr), ld, _VP(D_ptr), _VP(ws_ptr), _VP(B_ptr),
                                                  ldb, nrhs), "ipmz_normal_solve_multi")


def debug_inject(mask):
    """Test hook (ipmz_debug_inject): 1 = drop the persistent solve's first
    hand-off, 2 = the outer-panel factor's; 0 = normal operation."""
    _check(lib.ipmz_debug_inject(int(mask)), "ipmz_debug_inject")


INJECT_SOLVE, INJECT_PANEL, INJECT_GRAPH_FORKS = 1, 2, 4
# csrc/kernels.h: the forked single-QP step in its serial order (no work in the factor's idle edges)
DEBUG_SERIAL_EDGES = 8388608


def debug_edge_rows(rows):
    """Debug-mask bits that make the forked step's early forward sweep cover `rows` rows (a multiple
    of 128 up to 62 * 128; 0 and anything from N - 128 on: no early sweep)."""
    assert rows % 128 == 0 and 0 <= rows // 128 <= 62
    return (rows // 128 + 1) << 24

_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


class LinearSolvers:
    """NumericalOptimization::LinearSolvers with the reference's value semantics
    (LinearSolvers.h:11-17): fresh L and D returned, b overwritten."""

    @staticmethod
    def ldlt_decomposition(A, ctx=None):
        A = np.ascontiguousarray(A, dtype=np.float64)
        if A.ndim != 2 or A.shape[0] != A.shape[1]:
            raise IpmzError("ldlt_decomposition: matrix must be square")  # LinearSolvers.cpp:16-17
        N = A.shape[0]
        L = np.zeros((N, N))
        D = np.zeros(N)
        info = _check(lib.ipmz_ldlt_decomposition((ctx or default_context()).h, N, _dp(A), _dp(L), _dp(D)),
                      "ipmz_ldlt_decomposition")
        return L, D, info

    @staticmethod
    def overwriting_solve_ldlt(L, D, b, ctx=None):
        L = np.ascontiguousarray(L, dtype=np.float64)
        D = np.ascontiguousarray(D, dtype=np.float64)
        if not (isinstance(b, np.ndarray) and b.dtype == np.float64 and b.flags.c_contiguous):
            raise IpmzError("overwriting_solve_ldlt: b must be a contiguous float64 array")
        N = b.shape[0]
        if N and (D.shape[0] != N or L.shape != (N, N)):
            raise IpmzError("overwriting_solve_ldlt: size mismatch")  # LinearSolvers.cpp:50-53
        _check(lib.ipmz_overwriting_solve_ldlt((ctx or default_context()).h, N, _dp(L), _dp(D), _dp(b)),
               "ipmz_overwriting_solve_ldlt")
        return b

    @staticmethod
    def overwriting_solve_ldlt_multi(L, D, B, ctx=None):
        """overwriting_solve_ldlt for a block of right-hand sides: B is a
        C-contiguous float64 (nrhs, N) array, one right-hand side per row,
        overwritten with the solutions and returned."""
        L = np.ascontiguousarray(L, dtype=np.float64)
        D = np.ascontiguousarray(D, dtype=np.float64)
        if not (isinstance(B, np.ndarray) and B.dtype == np.float64 and B.ndim == 2 and B.flags.c_contiguous):
            raise IpmzError("overwriting_solve_ldlt_multi: B must be a C-contiguous float64 (nrhs, N) array")
        nrhs, N = B.shape
        if D.shape != (N,) or L.shape != (N, N):
            raise IpmzError("overwriting_solve_ldlt_multi: size mismatch")  # LinearSolvers.cpp:50-53
        _check(lib.ipmz_overwriting_solve_ldlt_multi((ctx or default_context()).h, N, _dp(L), _dp(D), _dp(B), nrhs),
               "ipmz_overwriting_solve_ldlt_multi")
        return B


def _ip(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def symmetric_indefinite_factorization(A, ctx=None):
    """LinearSolvers::symmetric_indefinite_factorization (LinearSolvers.h:23-26):
    returns (F, ipiv) -- F is A with its lower triangle factored."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    if A.ndim != 2 or A.shape[0] != A.shape[1]:
        raise IpmzError("symmetric_indefinite_factorization: matrix must be square")
    N = A.shape[0]
    F = np.zeros((N, N))
    ipiv = np.zeros(N, dtype=np.int32)
    _check(lib.ipmz_symmetric_indefinite_factorization((ctx or default_context()).h, N, _dp(A), _dp(F), _ip(ipiv)),
           "ipmz_symmetric_indefinite_factorization")
    return F, ipiv


def overwriting_solve_bunch_kaufman(F, ipiv, b, ctx=None):
    """LinearSolvers::overwriting_solve_bunch_kaufman (LinearSolvers.h:28-31): b overwritten."""
    F = np.ascontiguousarray(F, dtype=np.float64)
    ipiv = np.ascontiguousarray(ipiv, dtype=np.int32)
    if b.dtype != np.float64 or not b.flags.c_contiguous:
        raise IpmzError("overwriting_solve_bunch_kaufman: b must be a contiguous float64 array")
    _check(lib.ipmz_overwriting_solve_bunch_kaufman((ctx or default_context()).h, len(b), _dp(F), _ip(ipiv), _dp(b)),
           "ipmz_overwriting_solve_bunch_kaufman")


def overwriting_solve_bunch_kaufman_multi(F, ipiv, B, ctx=None):
    """overwriting_solve_bunch_kaufman for a block of right-hand sides: B is a
    C-contiguous float64 (nrhs, N) array, one right-hand side per row,
    overwritten with the solutions and returned."""
    F = np.ascontiguousarray(F, dtype=np.float64)
    ipiv = np.ascontiguousarray(ipiv, dtype=np.int32)
    if not (isinstance(B, np.ndarray) and B.dtype == np.float64 and B.ndim == 2 and B.flags.c_contiguous):
        raise IpmzError("overwriting_solve_bunch_kaufman_multi: B must be a C-contiguous float64 (nrhs, N) array")
    nrhs, N = B.shape
    if F.shape != (N, N) or ipiv.shape != (N,):
        raise IpmzError("overwriting_solve_bunch_kaufman_multi: size mismatch")
    _check(lib.ipmz_overwriting_solve_bunch_kaufman_multi((ctx or default_context()).h, N, _dp(F), _ip(ipiv), _dp(B),
                                                          nrhs), "ipmz_overwriting_solve_bunch_kaufman_multi")
    return B


LinearSolvers.symmetric_indefinite_factorization = staticmethod(symmetric_indefinite_factorization)
LinearSolvers.overwriting_solve_bunch_kaufman = staticmethod(overwriting_solve_bunch_kaufman)
LinearSolvers.overwriting_solve_bunch_kaufman_multi = staticmethod(overwriting_solve_bunch_kaufman_multi)


class Data:
    """NumericalOptimization::Data (EnvironmentBuilder.h:7-17)."""

    def __init__(self, Q, c, l_x, u_x, A_ineq=None, l_A_ineq=None, u_A_ineq=None, A_eq=None, b_eq=None):
        self.Q = np.ascontiguousarray(Q, dtype=np.float64)
        self.c = np.ascontiguousarray(c, dtype=np.float64)
        self.l_x = np.ascontiguousarray(l_x, dtype=np.float64)
        self.u_x = np.ascontiguousarray(u_x, dtype=np.float64)
        n = self.Q.shape[0]
        self.A_ineq = np.zeros((0, n)) if A_ineq is None else np.ascontiguousarray(A_ineq, dtype=np.float64)
        self.l_A_ineq = np.zeros(0) if l_A_ineq is None else np.ascontiguousarray(l_A_ineq, dtype=np.float64)
        self.u_A_ineq = np.zeros(0) if u_A_ineq is None else np.ascontiguousarray(u_A_ineq, dtype=np.float64)
        self.A_eq = np.zeros((0, n)) if A_eq is None else np.ascontiguousarray(A_eq, dtype=np.float64)
        self.b_eq = np.zeros(0) if b_eq is None else np.ascontiguousarray(b_eq, dtype=np.float64)


class Optimizer:
    """The Newton-step solver: build_environment + Optimizer (Optimizer.h:15-20).

    Formulation (Settings, SymbolicOptimization.h:28-64): by default
    InequalityHandling::SlackedSlacks with Bounds::Both, and
    EqualityHandling::Regularization (delta = 1e-4) when equalities exist.
    equality_handling=EQ_NONE: the zero (lambda_C, lambda_C) block the
    reference routes to solve_indefinite_ (Optimizer.cpp:63-75), factored
    with Bunch-Kaufman (any N; N <= 4096 per QP in batches); EQ_PENALTY: PenaltyFunction.
    inequality_handling=INEQ_SLACKS, inequality_bounds / variable_bounds =
    BOUNDS_LOWER / UPPER / NONE select the other Newton systems (absent
    blocks dropped from the Newton order, as the reference does).
    """

    def __init__(self, n, m=0, p=0, ctx=None, delta=1e-4, equality_handling=0, inequality_handling=0,
                 inequality_bounds=0, variable_bounds=0):
        self.ctx = ctx or default_context()
        cfg = _QPConfig(n, m, p, delta, equality_handling, inequality_handling, inequality_bounds, variable_bounds)
        self.equality_handling = equality_handling
        self.form = (inequality_handling, inequality_bounds, variable_bounds)
        h = _VP()
        _check(lib.ipmz_qp_create(self.ctx.h, ctypes.byref(cfg), ctypes.byref(h)), "ipmz_qp_create")
        self.h = h
        self.n, self.m, self.p = n, m, p
        self.N = lib.ipmz_qp_kkt_dim(h)  # n + m + p, or n + 2m + p (NaiveSlacks)
        self.state_len = lib.ipmz_qp_state_len(h)

    @classmethod
    def from_data(cls, data, ctx=None, **form):
        n, m, p = data.Q.shape[0], data.A_ineq.shape[0], data.A_eq.shape[0]
        o = cls(n, m, p, ctx, **form)
        o.load(data)
        return o

    def load(self, data):
        self._bump()
        keep = [data.Q, data.c, data.A_ineq, data.l_A_ineq, data.u_A_ineq, data.A_eq, data.b_eq, data.l_x, data.u_x]
        keep = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1) if np.size(a) else np.zeros(1) for a in keep]
        _check(lib.ipmz_qp_load_host(self.h, *[_dp(a) for a in keep]), "ipmz_qp_load_host (build_environment)")

    def _bump(self):
        """The generation counter: every call that moves the iterate or the data bumps it (ipmz_amd.layer's
        backward refuses to differentiate at another iterate than its forward's)."""
        self._generation = getattr(self, "_generation", 0) + 1

    def generate(self, seed):
        self._bump()
        _check(lib.ipmz_qp_generate(self.h, seed), "ipmz_qp_generate")

    # -- device-resident load and read-back (torch CUDA tensors; nothing passes through host memory) --
    def _order_torch_stream(self, torch):
        """Work already enqueued on torch's current stream comes before what the context enqueues next: nothing to
        do when the context runs on that stream, else that stream is synchronized."""
        cur = torch.cuda.current_stream(self.ctx.device)
        if not self.ctx.on_stream(cur.cuda_stream):
            cur.synchronize()

    def _on_device(self, t, name):
        if not t.is_cuda or t.device.index != self.ctx.device:
            raise ValueError(f"{name}: tensor on {t.device}, the context is on cuda:{self.ctx.device}")

    def load_tensors(self, Q=None, c=None, l_x=None, u_x=None, A_ineq=None, l_A_ineq=None, u_A_ineq=None, A_eq=None,
                     b_eq=None):
        """build_environment for every QP of the solver from float64 CUDA tensors (Data's names), then a fresh
        iterate: ipmz_batch_load_device.  Matrices are (batch, rows, n) or (rows, n) shared by every QP, vectors
        (batch, len) or (len,) shared; any row / batch strides (views, .expand), inner stride 1; nothing is copied.
        None keeps the block the solver holds (e.g. load_tensors(c=c2, b_eq=d2) for a parametric re-load)."""
        self._bump()
        import torch
        batch = lib.ipmz_batch_size(self.h)
        dims = dict(n=self.n, m=self.m, p=self.p)
        given = dict(Q=Q, c=c, l_x=l_x, u_x=u_x, A_ineq=A_ineq, l_A_ineq=l_A_ineq, u_A_ineq=u_A_ineq, A_eq=A_eq, b_eq=b_eq)
        d = _QPDeviceData()
        for fields in _BLOCKS:  # (`given` keeps the tensors referenced until the call returns)
            name, _, _, _, rows, cols = fields
            t, r, k = given[name], (None if rows is None else dims[rows]), dims[cols]
            if t is None or k == 0 or r == 0:
                continue
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{name}: a torch tensor is needed")
            self._on_device(t, name)
            _set_block(d, fields, _tensor_block(t, batch, r, k))
        self._order_torch_stream(torch)
        _check(lib.ipmz_batch_load_device(self.h, ctypes.byref(d)), "ipmz_batch_load_device")

    def state_tensor(self, which=0, out=None):
        """The state `which` (0 iterate, 1 affine direction, 2 direction, 3 residuals) of every QP as a
        (batch, state_len) float64 CUDA tensor, row q what state(q, which) returns: ipmz_batch_copy_state.
        out: a 2-D float64 tensor on the context's device with batch rows, inner stride 1 and row stride >=
        state_len (its columns from state_len on are not written).  Returns after ctx.sync()."""
        import torch
        batch, L = lib.ipmz_batch_size(self.h), self.state_len
        if out is None:
            out = torch.empty((batch, L), dtype=torch.float64, device=f"cuda:{self.ctx.device}")
        else:
            self._on_device(out, "out")
            if out.dtype != torch.float64 or out.dim() != 2 or out.shape[0] != batch or \
                    (out.shape[1] > 1 and out.stride(1) != 1):
                raise ValueError(f"out: a float64 ({batch}, >= {L}) tensor with inner stride 1 is needed")
        # (too few columns: the library refuses the row stride; the stride of a single row means nothing)
        ld = out.shape[1] if out.shape[1] < L or batch == 1 else out.stride(0)
        self._order_torch_stream(torch)
        _check(lib.ipmz_batch_copy_state(self.h, which, _VP(out.data_ptr()), ld), "ipmz_batch_copy_state")
        self.ctx.sync()
        return out[:, :L]

    def set_state_tensor(self, V, take=None, floor=0.0, check=True):
        """The iterate of every QP from a float64 CUDA tensor, state_tensor(0)'s inverse -- a warm start:
        ipmz_batch_set_state_device.  V: (batch, >= state_len) with inner stride 1 and any row stride, row q the
        iterate of QP q in the order of vars() / state(q); columns from state_len on are not read.  take: None
        (every QP), or a (batch,) bool or integer tensor -- QP q is set only where take[q] != 0, and the rows of
        the others are not read.  floor >= 0: every slack and inequality multiplier of a taken row (the slots the
        step length keeps non-negative) below floor becomes floor; a converged iterate lies on the boundary, so a
        warm start normally wants floor > 0.  check=True: a NaN, a non-positive slack or multiplier after the
        push, or (INEQ_SLACKS, and m == 0) x or s not strictly inside its bounds raises IpmzError naming the first
        (QP, index), nothing written, and costs one synchronize; check=False only enqueues (and may be captured
        into a graph on the context's stream).  On the context's stream, ordered after torch's current stream like
        load_tensors; then every QP is evaluated, as set_state does."""
        import torch
        batch, L = lib.ipmz_batch_size(self.h), self.state_len
        if not isinstance(V, torch.Tensor) or V.dtype != torch.float64 or V.dim() != 2 or V.shape[0] != batch or \
                (V.shape[1] > 1 and V.stride(1) != 1):
            raise ValueError(f"V: a float64 ({batch}, >= {L}) tensor with inner stride 1 is needed")
        self._on_device(V, "V")
        if take is not None:
            if not isinstance(take, torch.Tensor) or take.shape != (batch,) or take.is_floating_point() or \
                    take.is_complex():
                raise ValueError(f"take: a bool or integer ({batch},) tensor is needed")
            self._on_device(take, "take")
            take = (take != 0).to(torch.int32).contiguous()
        # (too few columns: the library refuses the row stride; the stride of a single row means nothing)
        ld = V.shape[1] if V.shape[1] < L or batch == 1 else V.stride(0)
        self._bump()
        self._order_torch_stream(torch)
        _check(lib.ipmz_batch_set_state_device(self.h, _VP(V.data_ptr()), ld, _VP(take.data_ptr()) if take is not None
                                               else None, float(floor), 0 if check else SET_STATE_UNCHECKED),
               "ipmz_batch_set_state_device")
        if not self.ctx.on_stream(torch.cuda.current_stream(self.ctx.device).cuda_stream):
            self.ctx.sync()  # (V and take may be freed or rewritten on torch's stream once this returns)

    def data_grad_tensors(self, W, shared=(), symmetrize=False, only=None):
        """The gradient with respect to the problem data from the cotangent with respect to the residuals:
        ipmz_batch_data_vjp.  W: a (batch, >= state_len) float64 CUDA tensor, row q the cotangent of QP q in the
        order of residuals() -- row 0 of newton_adjoint(_all)'s Out.  Returns a dict with load_tensors' names
        (Q, c, l_x, u_x, A_ineq, l_A_ineq, u_A_ineq, A_eq, b_eq; blocks of dimension 0 omitted), each a fresh
        tensor: (batch, ...) per QP, or, for the names in `shared`, (...) summed over the batch -- the gradient of
        a block that load_tensors was given once for every QP.  only: the names wanted (default: all).
        Q's n^2 entries are independent: gQ = w_x x^T; symmetrize=True returns (gQ + gQ^T) / 2.  Asynchronous on
        the context's stream, ordered after torch's current stream like load_tensors; when the context runs on
        another stream, the call returns after ctx.sync()."""
        import torch
        batch, L = lib.ipmz_batch_size(self.h), self.state_len
        if not isinstance(W, torch.Tensor) or W.dtype != torch.float64 or W.dim() != 2 or W.shape[0] != batch or \
                W.shape[1] < L or (W.shape[1] > 1 and W.stride(1) != 1):
            raise ValueError(f"W: a float64 ({batch}, >= {L}) tensor with inner stride 1 is needed")
        self._on_device(W, "W")
        names = [b[0] for b in _BLOCKS]
        for k in list(shared) + list(only or ()):
            if k not in names:
                raise ValueError(f"unknown block {k!r}: one of {names}")
        dims = dict(n=self.n, m=self.m, p=self.p)
        g = _QPDeviceGrad()
        out = {}
        for fields in _BLOCKS:
            name, _, _, _, rows, cols = fields
            r, c = (None if rows is None else dims[rows]), dims[cols]
            if c == 0 or r == 0 or (only is not None and name not in only):
                continue
            inner = (c,) if r is None else (r, c)
            t = torch.empty(inner if name in shared else (batch,) + inner, dtype=torch.float64, device=W.device)
            # (a batch of one has no shared blocks: the library ignores the QP stride there)
            _set_block(g, fields, _tensor_block(t, batch, r, c)[:2] + (0 if name in shared else t.stride(0),))
            out[name] = t
        self._order_torch_stream(torch)
        sW = W.stride(0) if batch > 1 else W.shape[1]
        _check(lib.ipmz_batch_data_vjp(self.h, _VP(W.data_ptr()), sW, ctypes.byref(g)), "ipmz_batch_data_vjp")
        if not self.ctx.on_stream(torch.cuda.current_stream(self.ctx.device).cuda_stream):
            self.ctx.sync()
        if symmetrize and "Q" in out:
            out["Q"] = 0.5 * (out["Q"] + out["Q"].transpose(-1, -2))
        return out

    def data_grad_tensors_multi(self, W, shared=(), symmetrize=False, only=None):
        """data_grad_tensors for a block of cotangent rows per QP: ipmz_batch_data_vjp_multi.  W: a
        (batch, ncot, >= state_len) float64 CUDA tensor with inner stride 1, row (q, r) cotangent r of QP q in the
        order of residuals() -- newton_adjoint(_all)'s Out of nrhs = ncot rows as it is.  Returns a dict with
        load_tensors' names (blocks of dimension 0 omitted), each a fresh tensor: (batch, ncot, ...) per QP, or,
        for the names in `shared`, (ncot, ...), row r summed over the batch.  Row r of every block has the bits
        data_grad_tensors gives for W[:, r] alone.  only, symmetrize and the stream ordering: as in
        data_grad_tensors."""
        import torch
        batch, L = lib.ipmz_batch_size(self.h), self.state_len
        if not isinstance(W, torch.Tensor) or W.dtype != torch.float64 or W.dim() != 3 or W.shape[0] != batch or \
                W.shape[2] < L or (W.shape[2] > 1 and W.stride(2) != 1):
            raise ValueError(f"W: a float64 ({batch}, ncot, >= {L}) tensor with inner stride 1 is needed")
        self._on_device(W, "W")
        ncot = W.shape[1]
        names = [b[0] for b in _BLOCKS]
        for k in list(shared) + list(only or ()):
            if k not in names:
                raise ValueError(f"unknown block {k!r}: one of {names}")
        dims = dict(n=self.n, m=self.m, p=self.p)
        g = _QPDeviceGradMulti()
        out = {}
        for fields in _BLOCKS:
            name, _, _, _, rows, cols = fields
            r, c = (None if rows is None else dims[rows]), dims[cols]
            if c == 0 or r == 0 or (only is not None and name not in only):
                continue
            inner = (c,) if r is None else (r, c)
            t = torch.empty((ncot,) + inner if name in shared else (batch, ncot) + inner, dtype=torch.float64,
                            device=W.device)
            # (a batch of one has no shared blocks: the library ignores the QP stride there)
            _set_block(g.g, fields, _tensor_block(t, batch, r, c, tangent=True), g)
            out[name] = t
        if ncot == 0:  # (nothing to write, and an empty W has no address to hand over)
            return out
        self._order_torch_stream(torch)
        # (the stride of a dimension of size 1 means nothing)
        ldw = W.stride(1) if ncot > 1 else W.shape[2]
        sW = W.stride(0) if batch > 1 else max(ncot, 1) * ldw
        _check(lib.ipmz_batch_data_vjp_multi(self.h, ncot, _VP(W.data_ptr()), ldw, sW, ctypes.byref(g)),
               "ipmz_batch_data_vjp_multi")
        if not self.ctx.on_stream(torch.cuda.current_stream(self.ctx.device).cuda_stream):
            self.ctx.sync()
        if symmetrize and "Q" in out:
            out["Q"] = 0.5 * (out["Q"] + out["Q"].transpose(-1, -2))
        return out

    def data_jvp_tensors(self, tangents, out=None):
        """The tangents of the residual vectors from tangents of the problem data: ipmz_batch_data_jvp, the
        forward-mode counterpart of data_grad_tensors.  tangents: a dict under load_tensors' names of float64 CUDA
        tensors with a tangent dimension after the batch's -- matrices (batch, ntan, rows, n) per QP or
        (ntan, rows, n) shared by every QP (the tangent of a block load_tensors was given once), vectors
        (batch, ntan, len) or (ntan, len); inner stride 1, any outer strides, nothing copied.  A missing name (or
        None) is a zero tangent, blocks of dimension 0 are ignored; all given tensors agree on ntan (ValueError).
        Returns R, (batch, ntan, even(state_len)): row (q, t) in the order of residuals(), the block
        newton_solve / newton_solve_all take as it is (nrhs = ntan, ldr = R.stride(1), sR = R.stride(0)).  out:
        such a tensor to write into (16-byte aligned, inner stride 1, even strides; columns from state_len on keep
        their bits).  mu is a constant of the call.  Asynchronous on the context's stream, ordered after torch's
        current stream like load_tensors; when the context runs on another stream, the call returns after
        ctx.sync()."""
        import torch
        batch, L = lib.ipmz_batch_size(self.h), self.state_len
        names = [b[0] for b in _BLOCKS]
        for k in tangents:
            if k not in names:
                raise ValueError(f"unknown block {k!r}: one of {names}")
        dims = dict(n=self.n, m=self.m, p=self.p)
        tan = _QPDeviceTangent()
        ntan = None
        for fields in _BLOCKS:
            name, _, _, _, rows, cols = fields
            t = tangents.get(name)
            if t is None:
                continue
            r, c = (None if rows is None else dims[rows]), dims[cols]
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{name}: a torch tensor is needed")
            self._on_device(t, name)
            blk = _tensor_block(t, batch, r, c, tangent=True)
            if ntan is not None and blk[4] != ntan:
                raise ValueError(f"{name}: {blk[4]} tangents, the blocks before it have {ntan}")
            ntan = blk[4]
            if c != 0 and r != 0:
                _set_block(tan.d, fields, blk, tan)
        if ntan is None:
            raise ValueError("data_jvp_tensors: no tangent given (ntan is taken from the tensors)")
        ldr = L + (L & 1)
        if out is None:
            out = torch.empty((batch, ntan, ldr), dtype=torch.float64, device=f"cuda:{self.ctx.device}")
        else:
            self._on_device(out, "out")
            if out.dtype != torch.float64 or out.dim() != 3 or tuple(out.shape[:2]) != (batch, ntan) or \
                    out.shape[2] < L or (out.shape[2] > 1 and out.stride(2) != 1):
                raise ValueError(f"out: a float64 ({batch}, {ntan}, >= {L}) tensor with inner stride 1 is needed")
        # (the stride of a dimension of size 1 means nothing)
        ld_out = out.stride(1) if ntan > 1 else out.shape[2] + (out.shape[2] & 1)
        s_out = out.stride(0) if batch > 1 else ntan * ld_out
        self._order_torch_stream(torch)
        _check(lib.ipmz_batch_data_jvp(self.h, ntan, ctypes.byref(tan), _VP(out.data_ptr()), ld_out, s_out),
               "ipmz_batch_data_jvp")
        if not self.ctx.on_stream(torch.cuda.current_stream(self.ctx.device).cuda_stream):
            self.ctx.sync()
        return out

    def solution_tensor(self):
        """x of every QP, (batch, n): x leads the Newton order in every formulation."""
        return self.state_tensor(0)[:, :self.n]

    def step(self, flags=0):
        self._bump()
        _check(lib.ipmz_qp_step(self.h, flags), "ipmz_qp_step")

    def can_skip_converged(self):
        """Does step(STEP_SKIP_CONVERGED) serve this solver under the context's current blocking?  Batches
        (batch > 1) of small systems (N <= 1024) with inner block 64; never a solver of one QP."""
        return bool(lib.ipmz_batch_can_skip_converged(self.h))

    def last_step_graph(self):
        """True when the last step replayed a captured hipGraph."""
        return bool(lib.ipmz_qp_last_step_graph(self.h))

    def set_reduction(self, reduction):
        """REDUCTION_AUGMENTED (default) or REDUCTION_NORMAL (config C2)."""
        _check(lib.ipmz_qp_set_reduction(self.h, reduction), "ipmz_qp_set_reduction")

    def set_mixed_precision(self, enable=True, tol=1e-12, max_refine=10):
        """Newton directions via the fp32 factor + fp64 refinement (config C5)."""
        _check(lib.ipmz_qp_set_mixed_precision(self.h, int(enable), tol, max_refine), "ipmz_qp_set_mixed_precision")

    def center(self, kappa, tol=1e-10, max_iter=30):
        """Newton iterations from the current iterate onto the central path at the fixed barrier parameter kappa,
        r(z; mu = kappa) = 0, for every QP of the solver: ipmz_batch_center.  Returns (iterations, centered): the
        updates each QP received (an int ndarray, one entry per QP) and how many QPs reached
        |r(z; kappa)|inf <= tol within max_iter updates; a centered QP is frozen.  Call it after a solve: the
        derivative calls (newton_adjoint, data_grad_tensors, data_jvp_tensors, ipmz_amd.layer) then return the
        exact derivative of data -> z(data; kappa), duals included, at any active set.  Afterwards every QP is
        evaluated as set_state does (scalars()["mu"] is about kappa) and steps continue from there.  tol and
        max_iter are parameters; their defaults come from a CPU prototype of the loop (include/ipmz.h; the device's
        counts and the cost of an iteration: DESIGN.md "Centering on the central path")."""
        self._bump()
        batch = lib.ipmz_batch_size(self.h)
        its = np.zeros(batch, dtype=np.int32)
        nc = ctypes.c_int(0)
        _check(lib.ipmz_batch_center(self.h, float(kappa), float(tol), int(max_iter),
                                     its.ctypes.data_as(ctypes.POINTER(_I)), ctypes.byref(nc)), "ipmz_batch_center")
        return its, nc.value

    def scalars(self):
        out = np.zeros(SC_COUNT)
        _check(lib.ipmz_qp_scalars(self.h, _dp(out)), "ipmz_qp_scalars")
        # (QP 0's block without SC["steps"]: only a batch's skip steps count there -- Batch.step_counts() -- and the
        # dict keeps the entries it always had)
        return {k: out[i] for k, i in SC.items() if k != "steps"}

    def device_scalars_ptr(self):
        p = _VP()
        _check(lib.ipmz_qp_device_scalars(self.h, ctypes.byref(p)), "ipmz_qp_device_scalars")
        return p.value

    def copy_scalars(self, dst_ptr):
        """Async device-to-device copy of the scalar block (ctx stream)."""
        _check(lib.ipmz_qp_copy_scalars(self.h, _VP(dst_ptr)), "ipmz_qp_copy_scalars")

    def solve(self, max_iter=100):
        self._bump()
        trace = np.zeros((max_iter + 1, 8))
        it = ctypes.c_int(0)
        _check(lib.ipmz_qp_solve(self.h, max_iter, _dp(trace), ctypes.byref(it)), "ipmz_qp_solve")
        rows = min(it.value + 1, max_iter)
        keys = ("f", "res", "mu", "alpha_aff", "mu_aff", "sigma", "alpha", "converged")
        return it.value, [dict(zip(keys, r)) for r in trace[:rows]]

    def _state(self, which):
        out = np.zeros(self.state_len)
        _check(lib.ipmz_qp_get_state(self.h, which, _dp(out)), "ipmz_qp_get_state")
        return out

    def vars(self):
        return self._state(0)

    def daff(self):
        return self._state(1)

    def dir(self):
        return self._state(2)

    def residuals(self):
        return self._state(3)

    def set_vars(self, v):
        self._bump()
        v = np.ascontiguousarray(v, dtype=np.float64)
        _check(lib.ipmz_qp_set_state(self.h, _dp(v)), "ipmz_qp_set_state")

    def kkt(self):
        K = np.zeros((self.N, self.N))
        _check(lib.ipmz_qp_get_kkt(self.h, _dp(K)), "ipmz_qp_get_kkt")
        return K

    def factor(self):
        """(L, D, P) the last step's factor left: the lower triangle as stored, the pivots and the
        persistent solve's prepared operators (ipmz_qp_get_factor; parity tests)."""
        n = _I64(0)
        _check(lib.ipmz_qp_get_factor(self.h, None, None, None, ctypes.byref(n)), "ipmz_qp_get_factor")
        L, D, P = np.zeros((self.N, self.N)), np.zeros(self.N), np.zeros(n.value)
        _check(lib.ipmz_qp_get_factor(self.h, _dp(L), _dp(D), _dp(P), ctypes.byref(n)), "ipmz_qp_get_factor")
        return L, D, P

    def kkt_solve(self, B_ptr, nrhs, ldb):
        """Every row of B (device, nrhs rows in Newton order, stride ldb) <-
        K^{-1} row with the KKT matrix of the current iterate (kkt()); returns
        the factor's info.  Single QPs on the fp64 augmented LDL^T only."""
        return _check(lib.ipmz_qp_kkt_solve(self.h, nrhs, _VP(B_ptr), ldb), "ipmz_qp_kkt_solve")

    def kkt_solve_bk(self, B_ptr, nrhs, ldb):
        """kkt_solve for single QPs with EqualityHandling::None: the step's Bunch-Kaufman
        factor, then bk_solve_multi on the rows of B; returns the factor's info."""
        return _check(lib.ipmz_qp_kkt_solve_bk(self.h, nrhs, _VP(B_ptr), ldb), "ipmz_qp_kkt_solve_bk")

    def kkt_solve_mixed(self, B_ptr, nrhs, ldb, tol=1e-12, max_refine=10):
        """kkt_solve through the fp32 factor + fp64 refinement, whether or not the steps use mixed
        precision; returns (the factor's info, (nrhs, 2) array of {ratio, corrections} per row)."""
        stat = np.zeros((max(nrhs, 0), 2))
        info = _check(lib.ipmz_qp_kkt_solve_mixed(self.h, nrhs, _VP(B_ptr), ldb, tol, max_refine, _dp(stat)),
                      "ipmz_qp_kkt_solve_mixed")
        return info, stat

    def newton_solve(self, R_ptr, D_ptr, nrhs, ldr, ldd, alpha_ptr=None):
        """compute_search_direction_ for a block of residual vectors: row r of R (device, nrhs rows
        of state_len doubles in the order of residuals(), stride ldr) -> the full Newton direction
        of J d = -r at the current iterate in row r of D (the order of daff(), stride ldd; D may
        be R), and get_max_step_ of it in alpha[r] (device, optional).  One factor for all rows;
        returns the factor's info.  fp64 LDL^T or Bunch-Kaufman (EQ_NONE) by the formulation."""
        return _check(lib.ipmz_qp_newton_solve_multi(self.h, nrhs, _VP(R_ptr), ldr, _VP(D_ptr), ldd, _VP(alpha_ptr)),
                      "ipmz_qp_newton_solve_multi")

    def newton_adjoint(self, G_ptr, Out_ptr, nrhs, ldg, ldo):
        """The transpose of newton_solve at the current iterate: row r of G (device, nrhs rows of
        state_len doubles in the order of daff(), stride ldg), the cotangent of a direction -> the
        cotangent with respect to the residual row, J^T out = -g, in row r of Out (the order of
        residuals(), stride ldo; Out may be G).  <g, newton_solve(r)> = <newton_adjoint(g), r>.
        The same factor and blocked solves; returns the factor's info."""
        return _check(lib.ipmz_qp_newton_adjoint_multi(self.h, nrhs, _VP(G_ptr), ldg, _VP(Out_ptr), ldo),
                      "ipmz_qp_newton_adjoint_multi")

    def set_timing(self, on=True):
        _check(lib.ipmz_qp_set_timing(self.h, 1 if on else 0), "ipmz_qp_set_timing")

    def phase_times(self):
        ms = np.zeros(8)
        fl = ctypes.c_double(0)
        nl = ctypes.c_int64(0)
        _check(lib.ipmz_qp_phase_times(self.h, _dp(ms), ctypes.byref(fl), ctypes.byref(nl)), "ipmz_qp_phase_times")
        out = {k: ms[i] for k, i in PH.items()}
        out["trailing_flops"] = fl.value
        out["trailing_launches"] = nl.value
        return out

    def close(self):
        if getattr(self, "h", None):
            lib.ipmz_qp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Batch(Optimizer):
    """A batch of independent QPs with identical (n, m, p) (config C4): every
    kernel launch serves the whole batch.  QP i of generate(seed) uses
    seed + i."""

    def __init__(self, n, m=0, p=0, batch=1, ctx=None, delta=1e-4, equality_handling=0, inequality_handling=0,
                 inequality_bounds=0, variable_bounds=0):
        self.ctx = ctx or default_context()
        cfg = _QPConfig(n, m, p, delta, equality_handling, inequality_handling, inequality_bounds, variable_bounds)
        self.equality_handling = equality_handling
        self.form = (inequality_handling, inequality_bounds, variable_bounds)
        h = _VP()
        _check(lib.ipmz_batch_create(self.ctx.h, ctypes.byref(cfg), batch, ctypes.byref(h)), "ipmz_batch_create")
        self.h = h
        self.n, self.m, self.p = n, m, p
        self.N = lib.ipmz_qp_kkt_dim(h)  # n + m + p, or n + 2m + p (NaiveSlacks)
        self.batch = batch
        self.state_len = lib.ipmz_qp_state_len(h)

    def load_one(self, index, data):
        self._bump()
        keep = [data.Q, data.c, data.A_ineq, data.l_A_ineq, data.u_A_ineq, data.A_eq, data.b_eq, data.l_x, data.u_x]
        keep = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1) if np.size(a) else np.zeros(1) for a in keep]
        _check(lib.ipmz_batch_load_host(self.h, index, *[_dp(a) for a in keep]), "ipmz_batch_load_host")

    def initialize(self):
        self._bump()
        _check(lib.ipmz_batch_initialize(self.h), "ipmz_batch_initialize")

    def copy_batch_scalars(self, dst_ptr):
        """Async device copy of all batch x SC_COUNT scalars (ctx stream)."""
        _check(lib.ipmz_batch_copy_scalars(self.h, _VP(dst_ptr)), "ipmz_batch_copy_scalars")

    def summary(self, dst_ptr):
        """Enqueue the convergence summary {max res, max mu, unconverged}
        into 3 device doubles at dst_ptr (one kernel, ctx stream)."""
        _check(lib.ipmz_batch_summary(self.h, _VP(dst_ptr)), "ipmz_batch_summary")

    def summary_into(self, t):
        """Device tensor t (>= 3 float64): the summary (the stepper protocol
        of ipmz_amd.dist.solve_sharded).  It is ordered before anything later
        on torch's current stream: enqueued there when the context runs on
        that stream, otherwise the context's stream is synchronized after it,
        so an all-reduce or .tolist() on torch's stream never reads a stale
        buffer."""
        self.summary(t.data_ptr())
        import torch
        if not self.ctx.on_stream(torch.cuda.current_stream(t.device).cuda_stream):
            self.ctx.sync()

    FACTOR_AUTO, FACTOR_ONE, FACTOR_PAIR, FACTOR_LEFT = 0, 1, 2, 3  # include/ipmz.h IPMZ_BATCH_FACTOR_*

    def set_factor_kernel(self, kernel):
        """FACTOR_AUTO, FACTOR_ONE (right-looking, one workgroup per QP),
        FACTOR_PAIR (right-looking, two per QP; needs 2 * batch <= #CU) or
        FACTOR_LEFT (left-looking, one per QP): the small batched LDL^T kernel."""
        _check(lib.ipmz_batch_set_factor_kernel(self.h, int(kernel)), "ipmz_batch_set_factor_kernel")

    def kkt_of(self, index):
        """kkt() of QP `index`: the (N, N) KKT matrix of its current iterate, lower triangle."""
        K = np.zeros((self.N, self.N))
        _check(lib.ipmz_batch_get_kkt(self.h, index, _dp(K)), "ipmz_batch_get_kkt")
        return K

    def kkt_solve_all(self, B_ptr, nrhs, ldb, sB):
        """For every QP q: the nrhs rows at B + q * sB (device, Newton order, row stride ldb) <-
        K_q^{-1} row with the KKT matrix of its current iterate (kkt_of(q)); returns the batched
        factor's info word.  A contiguous (batch, nrhs, ldb) torch tensor has sB = nrhs * ldb.
        fp64 LDL^T batches only (not EQ_NONE); the inherited kkt_solve stays for single QPs."""
        return _check(lib.ipmz_batch_kkt_solve(self.h, nrhs, _VP(B_ptr), ldb, sB), "ipmz_batch_kkt_solve")

    def kkt_solve_all_bk(self, B_ptr, nrhs, ldb, sB):
        """kkt_solve_all for EQ_NONE batches: the step's batched Bunch-Kaufman factor, then
        bk_solve_multi_batch on the rows of every QP; returns (the smallest non-zero per-QP
        info word or 0, the per-QP info words)."""
        info = np.zeros(self.batch, dtype=np.int32)
        rc = _check(lib.ipmz_batch_kkt_solve_bk(self.h, nrhs, _VP(B_ptr), ldb, sB,
                                                info.ctypes.data_as(ctypes.POINTER(_I))), "ipmz_batch_kkt_solve_bk")
        return rc, info

    def newton_solve_all(self, R_ptr, D_ptr, nrhs, ldr, sR, ldd, sD, alpha_ptr=None):
        """newton_solve for every QP of the batch at once: QP q's rows at R + q * sR and D + q * sD,
        its step lengths at alpha[q * nrhs ..].  Returns the batched factor's info word, or for
        EQ_NONE batches (Bunch-Kaufman) (the smallest non-zero per-QP info word or 0, the per-QP
        words), like kkt_solve_all_bk."""
        info = np.zeros(self.batch, dtype=np.int32)
        rc = _check(lib.ipmz_batch_newton_solve_multi(self.h, nrhs, _VP(R_ptr), ldr, sR, _VP(D_ptr), ldd, sD,
                                                      _VP(alpha_ptr), info.ctypes.data_as(ctypes.POINTER(_I))),
                    "ipmz_batch_newton_solve_multi")
        return (rc, info) if self.equality_handling == EQ_NONE else rc

    def newton_adjoint_all(self, G_ptr, Out_ptr, nrhs, ldg, sG, ldo, sO):
        """newton_adjoint for every QP of the batch at once: QP q's rows at G + q * sG and
        Out + q * sO.  Returns what newton_solve_all returns."""
        info = np.zeros(self.batch, dtype=np.int32)
        rc = _check(lib.ipmz_batch_newton_adjoint_multi(self.h, nrhs, _VP(G_ptr), ldg, sG, _VP(Out_ptr), ldo, sO,
                                                        info.ctypes.data_as(ctypes.POINTER(_I))),
                    "ipmz_batch_newton_adjoint_multi")
        return (rc, info) if self.equality_handling == EQ_NONE else rc

    def batch_scalars(self):
        out = np.zeros(self.batch * SC_COUNT)
        _check(lib.ipmz_batch_scalars(self.h, _dp(out)), "ipmz_batch_scalars")
        return out.reshape(self.batch, SC_COUNT)

    def state(self, index, which=0):
        out = np.zeros(self.state_len)
        _check(lib.ipmz_batch_get_state(self.h, index, which, _dp(out)), "ipmz_batch_get_state")
        return out

    def set_state(self, index, v):
        self._bump()
        v = np.ascontiguousarray(v, dtype=np.float64)
        _check(lib.ipmz_batch_set_state(self.h, index, _dp(v)), "ipmz_batch_set_state")

    def solve_all(self, max_iter=100, skip_converged=False, check_every=1, graph=False):
        """Step until every QP converged or max_iter: (steps enqueued, QPs converged).  skip_converged: the steps
        carry STEP_SKIP_CONVERGED, so a converged QP costs nothing in any launch (can_skip_converged() says
        whether the solver serves it; the iterates are bitwise those of the plain solve, step_counts() each QP's
        own count).  check_every: steps enqueued between two looks at the device.  graph: the steps replay a
        captured hipGraph.  The defaults are ipmz_batch_solve; anything else is ipmz_batch_solve_ex."""
        self._bump()
        it = ctypes.c_int(0)
        nc = ctypes.c_int(0)
        if not skip_converged and check_every == 1 and not graph:
            _check(lib.ipmz_batch_solve(self.h, max_iter, ctypes.byref(it), ctypes.byref(nc)), "ipmz_batch_solve")
        else:
            flags = (STEP_SKIP_CONVERGED if skip_converged else 0) | (STEP_GRAPH if graph else 0)
            _check(lib.ipmz_batch_solve_ex(self.h, max_iter, flags, int(check_every), ctypes.byref(it),
                                           ctypes.byref(nc)), "ipmz_batch_solve_ex")
        return it.value, nc.value

    def step_counts(self):
        """Per QP: the steps with STEP_SKIP_CONVERGED it took part in since the last load (SC["steps"])."""
        return self.batch_scalars()[:, SC["steps"]].astype(np.int64)
