"""CPU checks of the multi-right-hand-side interface: the ctypes prototypes of the ddm_*_multi entry points, and the argument checks that
fail before any device work (no GPU needed)."""
import ctypes

import numpy as np
import pytest

MULTI = {
    "ddm_op_apply_multi": 5, "ddm_op_applyscaleadd_multi": 6, "ddm_dot_multi": 6, "ddm_schwarz_apply_multi": 5,
    "ddm_galerkin_apply_multi": 5, "ddm_combined_apply_multi": 5, "ddm_cg_solve_multi": 10, "ddm_ilu0_set_status": 2,
}


def test_multi_prototypes(ddm):
    for name, nargs in MULTI.items():
        res, args = ddm.SYMBOLS[name]
        assert res is ctypes.c_int and len(args) == nargs, name
    # the column count is an int right after the object handle; the result array of the block CG is a SolveResult pointer
    for name in MULTI:
        if name != "ddm_ilu0_set_status":
            assert ddm.SYMBOLS[name][1][3 if name == "ddm_cg_solve_multi" else 2] is ctypes.c_int, name
    assert ddm.SYMBOLS["ddm_cg_solve_multi"][1][-1] is ctypes.POINTER(ddm.SolveResult)
    assert ddm.SYMBOLS["ddm_op_applyscaleadd_multi"][1][3] is ctypes.c_double


def test_multi_entry_points_reject_bad_arguments_without_a_device(ddm):
    lib = ddm.load_library()
    res = (ddm.SolveResult * 4)()
    out = np.zeros(4)
    assert lib.ddm_cg_solve_multi(None, None, None, 4, None, None, 1e-10, 10, None, res) == ddm.DDM_EINVAL
    assert "ddm_cg_solve_multi" in lib.ddm_last_error(None).decode()
    assert lib.ddm_op_apply_multi(None, None, 4, None, None) == ddm.DDM_EINVAL
    assert lib.ddm_op_applyscaleadd_multi(None, None, 4, 1.0, None, None) == ddm.DDM_EINVAL
    assert lib.ddm_dot_multi(None, None, 4, None, None, out.ctypes.data) == ddm.DDM_EINVAL
    assert "ddm_dot_multi" in lib.ddm_last_error(None).decode()
    for name in ("ddm_schwarz_apply_multi", "ddm_galerkin_apply_multi", "ddm_combined_apply_multi"):
        assert getattr(lib, name)(None, None, 4, None, None) == ddm.DDM_EINVAL
        assert name in lib.ddm_last_error(None).decode()
    assert lib.ddm_ilu0_set_status(None, 1) == ddm.DDM_EINVAL


def test_block_shape_checks_of_the_binding(ddm):
    assert ddm._ncols(np.zeros((7, 3)), np.zeros((7, 3))) == 3
    assert ddm._ncols(np.zeros(7)) == 1
    with pytest.raises(ValueError):
        ddm._ncols(np.zeros((7, 3)), np.zeros((7, 2)))
