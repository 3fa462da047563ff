"""CPU-side checks of ipmz_batch_center at the C boundary: include/ipmz.h declares the call, the library exports it,
the binding lists it with Optimizer.center and the layer's barrier option on top, and a null qp is refused before
any device use."""
import ctypes
import inspect
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ipmz.h")
LIB = os.path.join(REPO, "ipm-zoo_amd", "lib", "libipmz.so")
NAME = "ipmz_batch_center"
IPMZ_ERR_INVALID = -1


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_call():
    txt = _header()
    assert re.search(r"\bint\s+" + NAME + r"\s*\(\s*ipmz_qp\s*\*\s*qp\s*,\s*double\s+kappa\s*,\s*double\s+tol\s*,"
                     r"\s*int\s+max_iter\s*,\s*int\s*\*\s*iterations\s*,\s*int\s*\*\s*centered_count\s*\)\s*;", txt)
    # no new scalar slot: the centered flags and the counts live in a buffer of the solver
    assert re.search(r"IPMZ_SC_COUNT\s*=\s*16\b", txt)
    # the top comment's line for the entry point
    assert re.search(r"\*\s+" + NAME + r"\s+<-", open(HEADER).read())


def test_library_exports_the_call():
    assert os.path.exists(LIB), "build first: __graft_entry__.build()"
    assert hasattr(ctypes.CDLL(LIB), NAME)


def test_binding_lists_the_call():
    import ipmz_amd as I
    assert NAME in I.EXPORTS
    fn = getattr(I.lib, NAME)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 6
    assert fn.argtypes[1] is ctypes.c_double and fn.argtypes[2] is ctypes.c_double and fn.argtypes[3] is ctypes.c_int
    assert hasattr(I.Optimizer, "center") and I.Batch.center is I.Optimizer.center
    sig = inspect.signature(I.Optimizer.center)
    assert [p for p in sig.parameters] == ["self", "kappa", "tol", "max_iter"]
    assert sig.parameters["tol"].default == 1e-10 and sig.parameters["max_iter"].default == 30


def test_layer_has_the_barrier_option():
    import ipmz_amd.layer as layer
    sig = inspect.signature(layer.solve_qp)
    assert sig.parameters["barrier"].default is None
    assert sig.parameters["barrier_tol"].default == 1e-10 and sig.parameters["barrier_max_iter"].default == 30
    for fn in (layer.solve_qp, layer.solution_jvp, layer.solution_vjp, layer.solution_jacobian):
        assert "central path" in fn.__doc__, fn.__name__


def test_null_qp_is_refused_before_any_device_use():
    import ipmz_amd as I
    its, count = (ctypes.c_int * 1)(), ctypes.c_int(0)
    rc = I.lib.ipmz_batch_center(None, 1e-2, 1e-10, 30, its, ctypes.byref(count))
    assert rc == IPMZ_ERR_INVALID, rc
    msg = I.lib.ipmz_last_error()
    msg = msg.decode() if isinstance(msg, bytes) else str(msg)
    assert NAME in msg and "null" in msg, msg
