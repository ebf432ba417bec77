"""The C++ adaptors' value refresh (dune-ddm_amd/dune/ddm/hip/twolevel_schwarz.hh: TwoLevelSchwarzCore keeps its two levels between
solves and refreshes them from the refilled overlapping matrix), driven by tests/cpp/twolevel_refresh.cc on the DG problem of
tests/test_cpp_adaptor.py: two solves through one core with the values changed in between against a core built on the new values."""
import os
import subprocess

import numpy as np
import pytest

from tests import refresh_cases as rc
from tests.cpp_harness import CPP, ddm_symbols_used, dump_csr, run


def build_refresh_program():
    """through the pattern rule of tests/cpp/Makefile"""
    p = subprocess.run(["make", "-C", CPP, "build/twolevel_refresh"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    return os.path.join(CPP, "build", "twolevel_refresh")


def test_refresh_program_compiles_and_links(ddm):
    ddm.load_library()
    used = ddm_symbols_used(build_refresh_program())
    assert {"ddm_csr_set_values", "ddm_schwarz_refresh", "ddm_galerkin_set_inverse"} <= set(used)
    assert all(u in ddm.SYMBOLS for u in used), [u for u in used if u not in ddm.SYMBOLS]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [("multiplicative", "ilu0", "restartedgmressolver"), ("additive", "ilu0", "bicgstabsolver"),
                                 ("multiplicative", "umfpack", "restartedgmressolver")])
def test_core_refreshes_its_levels(ddm, tmp_path, cfg):
    """second solve: same `fine` and `coarse` objects, iterations and solution bytes of a fresh core on the changed matrix (ilu0: the
    device refactorisation; umfpack: the local solver is dropped and built again inside the same adaptor object)"""
    from dune_ddm_amd import synth
    from dune_ddm_amd.problem import build_structured
    mode, local, krylov = cfg
    exe = build_refresh_program()
    grid = synth.StructuredDG2D((16, 16), (1, 1))
    sd = build_structured(grid, overlap=1).subs[0]
    A = sd.A.tocsr()
    A.sort_indices()
    A2 = rc.new_values(A, 13)
    rc.assert_dominant(A2)
    assert rc.same_pattern(A, A2)
    dump_csr(tmp_path, A)
    np.asarray(A2.data, dtype=np.float64).tofile(tmp_path / "val2.bin")
    sd.b.astype(np.float64).tofile(tmp_path / "b.bin")
    sd.pou.astype(np.float64).tofile(tmp_path / "pou.bin")
    np.ascontiguousarray(grid.dof_coords(sd.glob), dtype=np.float64).tofile(tmp_path / "coords.bin")
    p = run(exe, tmp_path, mode, local, krylov)
    print(p.stdout)
    lines = {ln.split()[0]: ln.split() for ln in p.stdout.splitlines()}
    assert lines["same_objects"][1] == "1" and lines["same_objects"][3] == "1"
    assert lines["coarse_matrix_equal"][1] == "1" and lines["levels_dropped"][1] == "1"
    assert lines["refreshed"][1:] == lines["fresh"][1:] and lines["refreshed"][4] == "1"
    z1, z2, zf = (np.fromfile(tmp_path / f"z_{k}.bin", dtype=np.float64) for k in ("first", "refreshed", "fresh"))
    assert np.isfinite(zf).all() and np.array_equal(z2, zf) and not np.array_equal(z1, z2)
