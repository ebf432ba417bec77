"""CPU checks of the queued CG driver (ddm_cg_solve_queue: any number of right-hand sides through a block of fixed width; no GPU
needed): the exported symbol and its prototype, the argument checks that fail before any device work, and the argument checks of
TwoLevelSchwarz.solve_many."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_queue_prototype(ddm):
    """the symbol is exported by the library (load_library resolves every entry of SYMBOLS) with the documented signature: ncols is a
    64-bit count, width an int, then the arguments of ddm_cg_solve_multi after nrhs"""
    lib = ddm.load_library()
    P, I, L, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    R = ctypes.POINTER(ddm.SolveResult)
    assert ddm.SYMBOLS["ddm_cg_solve_queue"] == (I, [P, P, P, L, I, P, P, D, I, P, R])
    assert ddm.SYMBOLS["ddm_cg_solve_queue"][1][5:] == ddm.SYMBOLS["ddm_cg_solve_multi"][1][4:]
    assert lib.ddm_cg_solve_queue is not None
    assert callable(ddm.cg_solve_queue)
    header = open(os.path.join(ROOT, "include", "ddm_hip.h")).read()
    assert "int ddm_cg_solve_queue(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, int64_t ncols, int width, double *X, double *B, double reduction," in header


@pytest.mark.parametrize("ncols, width, maxit, word", [(4, 2, 10, "bad arguments"), (4, 0, 10, "width"), (4, 33, 10, "width"), (0, 2, 10, "ncols"),
                                                        (4, 2, -1, "bad arguments"), (2 ** 40, 8, 10, "bad arguments")])
def test_queue_rejects_bad_arguments_without_a_device(ddm, ncols, width, maxit, word):
    """null handles with otherwise valid numbers, width 0 and 33, ncols 0, maxit -1: DDM_EINVAL naming the function (ncols beyond
    2^31 is a valid count: it gets as far as the null handles)"""
    lib = ddm.load_library()
    res = (ddm.SolveResult * 4)()
    lib.ddm_cg_solve_multi(None, None, None, 4, None, None, 1e-10, 10, None, res)   # (leaves another function's name in the error text)
    assert lib.ddm_cg_solve_queue(None, None, None, ncols, width, None, None, 1e-10, maxit, None, res) == ddm.DDM_EINVAL
    msg = lib.ddm_last_error(None).decode()
    assert "ddm_cg_solve_queue" in msg and word in msg, msg
    # the block entry point keeps its cap
    assert lib.ddm_cg_solve_multi(None, None, None, 33, None, None, 1e-10, 10, None, res) == ddm.DDM_EINVAL


def test_solve_many_checks_its_arguments_first(ddm):
    """solve_many refuses a width outside [1, 32] and a negative maxit before it reads any attribute of the object; with valid numbers,
    on an object without a device, it gets past these checks and fails on the first attribute it needs (AttributeError).  solve_multi
    still refuses bicgstabsolver by name."""
    from dune_ddm_amd.solver import TwoLevelSchwarz
    tl = object.__new__(TwoLevelSchwarz)                 # no __init__: no device, no context
    for width in (0, 33, -1):
        with pytest.raises(ValueError, match="width"):
            tl.solve_many(None, width=width)
    with pytest.raises(ValueError, match="maxit"):
        tl.solve_many(None, width=8, maxit=-1)
    for width in (1, 8, 32):
        with pytest.raises(AttributeError):
            tl.solve_many(None, width=width)
    with pytest.raises(NotImplementedError, match="bicgstabsolver"):
        tl.solve_multi(solver="bicgstabsolver")
