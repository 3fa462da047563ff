"""CPU-side checks of IPMZ_STEP_SKIP_CONVERGED at the C boundary: include/ipmz.h declares the flag, the scalar slot
and the two calls, the library exports the calls, the binding lists them with the header's values, and a null qp is
answered before any device use."""
import ctypes
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ipmz.h")
LIB = os.path.join(REPO, "ipm-zoo_amd", "lib", "libipmz.so")
NAMES = ("ipmz_batch_solve_ex", "ipmz_batch_can_skip_converged")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _define(txt, name):
    m = re.search(r"#\s*define\s+" + name + r"\s+(\d+)\b", txt)
    assert m, name
    return int(m.group(1))


def _scalar_slots(txt):
    """name -> index of enum ipmz_scalar, counted as a C compiler counts."""
    body = re.search(r"enum\s+ipmz_scalar\s*\{(.*?)\}", txt, flags=re.S).group(1)
    slots, nxt = {}, 0
    for item in (i.strip() for i in body.split(",")):
        if not item:
            continue
        name, _, val = (x.strip() for x in item.partition("="))
        nxt = int(val) if val else nxt
        slots[name] = nxt
        nxt += 1
    return slots


def test_header_declares_the_flag_the_slot_and_the_calls():
    txt = _header()
    assert _define(txt, "IPMZ_STEP_SKIP_CONVERGED") == 4
    flags = [_define(txt, n) for n in ("IPMZ_STEP_RESTART_IF_CONVERGED", "IPMZ_STEP_GRAPH", "IPMZ_STEP_SKIP_CONVERGED")]
    assert sorted(flags) == [1, 2, 4], "the step flags are distinct bits"
    slots = _scalar_slots(txt)
    assert slots["IPMZ_SC_STEPS"] == 14 and slots["IPMZ_SC_COUNT"] == 16
    assert slots["IPMZ_SC_CONVERGED"] == 7 and slots["IPMZ_SC_IR_ITERS"] == 13
    assert len(set(v for k, v in slots.items() if k != "IPMZ_SC_COUNT")) == len(slots) - 1, "no slot is used twice"
    assert re.search(r"\bint\s+ipmz_batch_solve_ex\s*\(\s*ipmz_qp\s*\*\s*qp\s*,\s*int\s+max_iter\s*,\s*int\s+step_flags\s*,"
                     r"\s*int\s+check_every\s*,\s*int\s*\*\s*iterations\s*,\s*int\s*\*\s*converged_count\s*\)\s*;", txt)
    assert re.search(r"\bint\s+ipmz_batch_can_skip_converged\s*\(\s*ipmz_qp\s*\*\s*qp\s*\)\s*;", txt)


def test_library_exports_the_calls():
    assert os.path.exists(LIB), "build first: __graft_entry__.build()"
    lib = ctypes.CDLL(LIB)
    for name in NAMES:
        assert hasattr(lib, name), name


def test_binding_matches_the_header():
    import ipmz_amd as I
    txt = _header()
    assert I.STEP_SKIP_CONVERGED == _define(txt, "IPMZ_STEP_SKIP_CONVERGED")
    slots = _scalar_slots(txt)
    assert I.SC["steps"] == slots["IPMZ_SC_STEPS"] and I.SC_COUNT == slots["IPMZ_SC_COUNT"]
    for k, v in I.SC.items():
        assert slots["IPMZ_SC_" + k.upper()] == v, k
    for name in NAMES:
        assert name in I.EXPORTS
    ex = I.lib.ipmz_batch_solve_ex
    assert ex.restype is ctypes.c_int and len(ex.argtypes) == 6
    assert all(a is ctypes.c_int for a in ex.argtypes[1:4])
    can = I.lib.ipmz_batch_can_skip_converged
    assert can.restype is ctypes.c_int and len(can.argtypes) == 1
    for name in ("can_skip_converged", "solve_all", "step_counts"):
        assert hasattr(I.Batch, name), name


def test_null_qp_is_answered_before_any_device_use():
    import ipmz_amd as I
    assert I.lib.ipmz_batch_can_skip_converged(None) == 0
    rc = I.lib.ipmz_batch_solve_ex(None, 10, I.STEP_SKIP_CONVERGED, 1, None, None)
    assert rc == -1, rc
    msg = I.lib.ipmz_last_error()
    msg = msg.decode() if isinstance(msg, bytes) else str(msg)
    assert "null" in msg, msg
