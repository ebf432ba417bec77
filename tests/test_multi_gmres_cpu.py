"""CPU checks of ddm_gmres_solve_multi (restarted GMRES for several right-hand sides): the ctypes prototype, the argument checks that
fail before any device work, and the solver dispatch of TwoLevelSchwarz.solve_multi (no GPU needed)."""
import ctypes

import pytest


def test_gmres_multi_prototype(ddm):
    res, args = ddm.SYMBOLS["ddm_gmres_solve_multi"]
    assert res is ctypes.c_int and len(args) == 11
    assert args[3] is ctypes.c_int                       # nrhs, right after ctx / op / prec
    assert args[6] is ctypes.c_double                    # reduction
    assert args[7] is ctypes.c_int and args[8] is ctypes.c_int   # maxit, restart
    assert args[-1] is ctypes.POINTER(ddm.SolveResult)
    assert callable(ddm.gmres_solve_multi)


@pytest.mark.parametrize("nrhs, maxit, restart", [(4, 10, 5), (0, 10, 5), (33, 10, 5), (4, 10, 0), (4, -1, 5)])
def test_gmres_multi_rejects_bad_arguments_without_a_device(ddm, nrhs, maxit, restart):
    """null handles with otherwise valid numbers, nrhs 0 and 33, restart 0, maxit -1: DDM_EINVAL naming the function"""
    lib = ddm.load_library()
    res = (ddm.SolveResult * 33)()
    lib.ddm_cg_solve_multi(None, None, None, 4, None, None, 1e-10, 10, None, res)   # (leaves another function's name in the error text)
    assert lib.ddm_gmres_solve_multi(None, None, None, nrhs, None, None, 1e-10, maxit, restart, None, res) == ddm.DDM_EINVAL
    assert "ddm_gmres_solve_multi" in lib.ddm_last_error(None).decode()


def test_solve_multi_rejects_unknown_solver_before_touching_the_device(ddm):
    """the dispatch happens first: no attribute of the object (context, operator, ...) is read for an unknown solver type"""
    from dune_ddm_amd.solver import TwoLevelSchwarz
    tl = object.__new__(TwoLevelSchwarz)                 # no __init__: no device, no context
    with pytest.raises(NotImplementedError, match="minressolver"):
        tl.solve_multi(solver="minressolver")
    with pytest.raises(NotImplementedError, match="bicgstabsolver"):
        tl.solve_multi(solver="bicgstabsolver")
