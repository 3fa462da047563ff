"""CPU-side checks of ipmz_batch_set_state_device at the C boundary: include/ipmz.h declares the call and its flag,
the library exports it, the binding lists it, and a null qp is refused before any device use -- and the self-test
of the numpy restatement the GPU tests judge the push and the check by (tests/warm_start_cases.py)."""
import ctypes
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ipmz.h")
LIB = os.path.join(REPO, "ipm-zoo_amd", "lib", "libipmz.so")
NAME = "ipmz_batch_set_state_device"
IPMZ_ERR_INVALID = -1


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_call_and_its_flag():
    txt = _header()
    assert re.search(r"\bint\s+" + NAME + r"\s*\(\s*ipmz_qp\s*\*\s*qp\s*,\s*const\s+double\s*\*\s*src\s*,\s*int64_t\s+ld\s*,"
                     r"\s*const\s+int32_t\s*\*\s*take\s*,\s*double\s+floor\s*,\s*int\s+flags\s*\)\s*;", txt)
    assert re.search(r"#\s*define\s+IPMZ_SET_STATE_UNCHECKED\s+1\b", txt)


def test_library_exports_the_call():
    assert os.path.exists(LIB), "build first: __graft_entry__.build()"
    assert hasattr(ctypes.CDLL(LIB), NAME)


def test_binding_lists_the_call():
    import ipmz_amd as I
    assert NAME in I.EXPORTS
    assert I.SET_STATE_UNCHECKED == 1
    fn = getattr(I.lib, NAME)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 6 and fn.argtypes[4] is ctypes.c_double
    assert hasattr(I.Optimizer, "set_state_tensor") and I.Batch.set_state_tensor is I.Optimizer.set_state_tensor


def test_null_qp_is_refused_before_any_device_use():
    import ipmz_amd as I
    err = I.IPMZ_ERR_INVALID if hasattr(I, "IPMZ_ERR_INVALID") else IPMZ_ERR_INVALID
    w = (ctypes.c_double * 4)()
    rc = I.lib.ipmz_batch_set_state_device(None, ctypes.cast(w, ctypes.c_void_p), 4, None, 0.0, 0)
    assert rc == err, rc
    msg = I.lib.ipmz_last_error()
    msg = msg.decode() if isinstance(msg, bytes) else str(msg)
    assert NAME in msg and "null" in msg, msg


def test_numpy_restatement_of_the_push_and_the_check():
    import warm_start_cases as wc
    wc.self_test()
