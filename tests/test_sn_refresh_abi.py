"""CPU checks of the export the value refresh of direct factors adds (no GPU needed): ddm_ilu0_refresh_count is declared in
include/ddm_hip.h, has a prototype in the Python binding, is exported, and answers 0 for a NULL factor; ddm_ilu0_refresh and
ddm_schwarz_refresh reject NULL arguments before they touch a device."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_refresh_count_is_declared_exported_and_bound(ddm):
    header = open(os.path.join(ROOT, "include", "ddm_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+ddm_ilu0_refresh_count\s*\(\s*const\s+ddm_ilu0\s*\*\s*F\s*\)\s*;", code)
    res, args = ddm.SYMBOLS["ddm_ilu0_refresh_count"]
    assert res is ctypes.c_int and args == [ctypes.c_void_p]
    lib = ddm.load_library()
    assert hasattr(lib, "ddm_ilu0_refresh_count")
    assert hasattr(ddm.Ilu0, "refresh_count") and hasattr(ddm.SchwarzPreconditioner, "refresh_count")


def test_null_arguments(ddm):
    lib = ddm.load_library()
    assert lib.ddm_ilu0_refresh_count(None) == 0
    assert lib.ddm_ilu0_refresh(None, None) == ddm.DDM_EINVAL
    assert lib.ddm_schwarz_refresh(None, None) == ddm.DDM_EINVAL


def test_the_header_says_what_is_refreshed_and_what_is_refused():
    header = open(os.path.join(ROOT, "include", "ddm_hip.h")).read()
    block = header[header.index("Refactorises from the CURRENT values"):header.index("int ddm_ilu0_refresh(")]
    for phrase in ("HOST-engine sparse direct factor", "box engine", "DEVICE supernodal direct factor", "invalid", "create a new"):
        assert phrase in block, phrase
