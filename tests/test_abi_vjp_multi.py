"""CPU-side checks of ipmz_batch_data_vjp_multi at the C boundary: include/ipmz.h declares it, the library exports
it, and a null qp is refused before any device use (as ipmz_batch_data_vjp refuses it)."""
import ctypes
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ipmz.h")
LIB = os.path.join(REPO, "ipm-zoo_amd", "lib", "libipmz.so")
NAME = "ipmz_batch_data_vjp_multi"
IPMZ_ERR_INVALID = -1


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_call_and_its_structure():
    txt = _header()
    assert re.search(r"\bint\s+" + NAME + r"\s*\(\s*ipmz_qp\s*\*\s*qp\s*,\s*int\s+ncot\s*,", txt)
    m = re.search(r"typedef\s+struct\s+ipmz_qp_device_grad_multi\s*\{(.*?)\}\s*ipmz_qp_device_grad_multi\s*;", txt, re.S)
    assert m, "ipmz_qp_device_grad_multi is not declared"
    body = m.group(1)
    assert re.search(r"\bipmz_qp_device_grad\s+g\s*;", body)
    strides = re.search(r"int64_t\s+([^;]*);", body).group(1)
    assert [k.strip() for k in strides.split(",")] == ["tQ", "tA", "tC", "tc", "tlx", "tux", "tlA", "tuA", "td"]


def test_library_exports_the_call():
    assert os.path.exists(LIB), "build first: __graft_entry__.build()"
    assert hasattr(ctypes.CDLL(LIB), NAME)


def test_binding_structure_has_the_header_layout():
    import ipmz_amd as I
    assert NAME in I.EXPORTS
    assert [f[0] for f in I._QPDeviceGradMulti._fields_] == ["g", "tQ", "tA", "tC", "tc", "tlx", "tux", "tlA", "tuA", "td"]
    assert ctypes.sizeof(I._QPDeviceGradMulti) == ctypes.sizeof(I._QPDeviceGrad) + 9 * 8
    assert I._QPDeviceGradMulti.tQ.offset == ctypes.sizeof(I._QPDeviceData)


def test_null_qp_is_refused_before_any_device_use():
    import ipmz_amd as I
    err = I.IPMZ_ERR_INVALID if hasattr(I, "IPMZ_ERR_INVALID") else IPMZ_ERR_INVALID
    g = I._QPDeviceGradMulti()
    w = (ctypes.c_double * 4)()
    rc = I.lib.ipmz_batch_data_vjp_multi(None, 1, ctypes.cast(w, ctypes.c_void_p), 4, 4, ctypes.byref(g))
    assert rc == err, rc
    msg = I.lib.ipmz_last_error()
    msg = msg.decode() if isinstance(msg, bytes) else str(msg)
    assert "ipmz_batch_data_vjp_multi" in msg and "null" in msg, msg
