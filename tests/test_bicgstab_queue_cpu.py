"""CPU checks of the queued BiCGSTAB driver (ddm_bicgstab_solve_queue: any number of right-hand sides through a BiCGSTAB block of
fixed width; no GPU needed): the exported symbol and its prototype, the argument checks that fail before any device work, the
argument checks of TwoLevelSchwarz.solve_many(solver=...), and the queue protocol itself restated in numpy
(tests/bicgstab_queue_reference.py) -- the only test of the breakdown path: no well-posed input at test size reaches 1e-80
deterministically on the device."""
import ctypes
import os

import numpy as np
import pytest

from tests import bicgstab_queue_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. signature, export, argument checks ---------------------------------------------------------------------------------------------
def test_bicgstab_queue_prototype(ddm):
    """the arguments of ddm_cg_solve_queue with nhist (int32 per column) between the history and the results, as ddm_bicgstab_solve has it"""
    lib = ddm.load_library()
    P, I, L, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    R, N = ctypes.POINTER(ddm.SolveResult), ctypes.POINTER(ctypes.c_int32)
    assert ddm.SYMBOLS["ddm_bicgstab_solve_queue"] == (I, [P, P, P, L, I, P, P, D, I, P, N, R])
    q = ddm.SYMBOLS["ddm_cg_solve_queue"][1]
    assert ddm.SYMBOLS["ddm_bicgstab_solve_queue"][1] == q[:-1] + [N] + q[-1:]
    assert lib.ddm_bicgstab_solve_queue is not None
    assert callable(ddm.bicgstab_solve_queue)
    header = open(os.path.join(ROOT, "include", "ddm_hip.h")).read()
    assert ("int ddm_bicgstab_solve_queue(ddm_ctx *ctx, ddm_op *op, ddm_combined *prec, int64_t ncols, int width, double *X, double *B, double reduction,\n"
            "                             int maxit, double *hist_host, int32_t *nhist, ddm_solve_result *res);") in header


@pytest.mark.parametrize("ncols, width, maxit, word", [(4, 2, 10, "bad arguments"), (4, 0, 10, "width"), (4, 33, 10, "width"), (0, 2, 10, "ncols"),
                                                        (4, 2, -1, "bad arguments")])
def test_bicgstab_queue_rejects_bad_arguments_without_a_device(ddm, ncols, width, maxit, word):
    """null handles with otherwise valid numbers, width 0 and 33, ncols 0, maxit -1: DDM_EINVAL naming the function"""
    lib = ddm.load_library()
    res = (ddm.SolveResult * 4)()
    lib.ddm_cg_solve_queue(None, None, None, 4, 2, None, None, 1e-10, 10, None, res)   # (leaves another function's name in the error text)
    assert lib.ddm_bicgstab_solve_queue(None, None, None, ncols, width, None, None, 1e-9, maxit, None, None, res) == ddm.DDM_EINVAL
    msg = lib.ddm_last_error(None).decode()
    assert "ddm_bicgstab_solve_queue" in msg and word in msg, msg


def test_solve_many_checks_solver_and_numbers_first(ddm):
    """an unknown solver is refused by name before any attribute of the object is read, the message naming the two that are accepted; the
    width and maxit checks hold for both; with valid numbers an object without a device fails on the first attribute it needs"""
    from dune_ddm_amd.solver import TwoLevelSchwarz
    tl = object.__new__(TwoLevelSchwarz)                 # no __init__: no device, no context
    for name in ("minressolver", "restartedgmressolver"):
        with pytest.raises(NotImplementedError) as e:
            tl.solve_many(None, solver=name)
        assert "cgsolver" in str(e.value) and "bicgstabsolver" in str(e.value) and name in str(e.value)
    for solver in ("cgsolver", "bicgstabsolver"):
        for width in (0, 33):
            with pytest.raises(ValueError, match="width"):
                tl.solve_many(None, width=width, solver=solver)
        with pytest.raises(ValueError, match="maxit"):
            tl.solve_many(None, width=8, maxit=-1, solver=solver)
        with pytest.raises(AttributeError):
            tl.solve_many(None, width=8, solver=solver)
    with pytest.raises(NotImplementedError, match="bicgstabsolver"):
        tl.solve_multi(solver="bicgstabsolver")          # (the block solve is solve_many with M <= width)


# ---- 2. the protocol in numpy ----------------------------------------------------------------------------------------------------------
N, RED, MAXIT = 24, 1e-9, 60


@pytest.fixture(scope="module")
def system():
    """a small dense non-symmetric system, a fixed non-symmetric preconditioner (an inexact inverse), 7 right-hand sides of different
    difficulty (the number of eigen-directions they excite differs), each solved on its own"""
    rng = np.random.default_rng(2024)
    A = np.diag(np.linspace(1.0, 9.0, N)) + 0.35 * rng.standard_normal((N, N))
    Winv = np.linalg.inv(np.diag(np.diag(A)) + np.triu(A, 1) * 0.5) + 0.01 * rng.standard_normal((N, N))
    B = rng.standard_normal((N, 7))
    B[N // 3:, 1] = 0.0
    B[:, 4] *= 1e-6
    B[3:, 5] = 0.0
    singles = [ref.single(A, Winv, np.zeros(N), B[:, j], RED, MAXIT) for j in range(7)]
    return A, Winv, B, singles


def test_fresh_slot_reproduces_the_first_step_bitwise(system):
    """p = v = 0 through the general direction update is r exactly, whatever beta and omega: the `it < 1` branch"""
    A, Winv, B, singles = system
    rng = np.random.default_rng(5)
    z = np.zeros(N)
    for beta in (1.0, -3.7e40, 2.0 ** -900, 5e307):
        for omega in (1.0, -0.3, 1e300):
            r = rng.standard_normal(N) * 10.0 ** rng.integers(-30, 30)
            assert np.array_equal(ref.direction(z, z, r, beta, omega), r)
    for j in range(7):                                   # ... and so a column alone in one slot is the single loop, bit for bit
        q = ref.queue(A, Winv, np.zeros((N, 1)), B[:, j:j + 1], 1, RED, MAXIT)
        s = singles[j]
        assert s["converged"] and q["converged"][0] and q["iterations"][0] == s["iterations"] and q["nhist"][0] == len(s["hist"])
        assert np.array_equal(q["hist"][:len(s["hist"]), 0], s["hist"]) and np.isnan(q["hist"][len(s["hist"]):, 0]).all()
        assert np.array_equal(q["X"][:, 0], s["x"])


def test_seven_columns_through_three_slots_equal_seven_single_solves(system):
    """M = 7, w = 3: refills in the middle of the other slots' recurrences change nothing, bit for bit; a column that stopped after a first
    half step while another slot ran on exists and was left untouched by the second (asserted inside the reference at every boundary)"""
    A, Winv, B, singles = system
    q = ref.queue(A, Winv, np.zeros((N, 7)), B, 3, RED, MAXIT)
    print("half steps", [len(s["hist"]) - 1 for s in singles], "frozen", q["frozen"])
    for j, s in enumerate(singles):
        k = len(s["hist"])
        assert q["nhist"][j] == k and q["iterations"][j] == s["iterations"] == k // 2 and q["converged"][j] == s["converged"] == True  # noqa: E712
        assert np.array_equal(q["hist"][:k, j], s["hist"]) and np.isnan(q["hist"][k:, j]).all(), j
        assert np.array_equal(q["X"][:, j], s["x"]), j
    assert len({len(s["hist"]) for s in singles}) > 2                     # the columns do leave at different times
    assert q["frozen"] and all((q["nhist"][j] - 1) % 2 == 1 for j, _ in q["frozen"])
    assert any(len([c for c in row if c >= 0]) == 3 and sorted(row) != [0, 1, 2] for row in q["trace"])   # refilled slots ran beside old ones


def test_queue_boundaries_zero_columns_maxit_and_warm_start(system):
    """zero columns (two in a row) are finished at the boundary they enter at and the slot is refilled again; maxit = 2 stores the whole
    block at once after 4 half steps; maxit = 0 leaves X; a non-zero initial guess is the single loop from that guess"""
    A, Winv, B, singles = system
    Bz = np.stack([np.zeros(N), B[:, 0], np.zeros(N), np.zeros(N), B[:, 1], B[:, 2], np.zeros(N)], axis=1)
    X0 = np.zeros((N, 7))
    q = ref.queue(A, Winv, X0, Bz, 2, RED, MAXIT)
    for c, j in enumerate([None, 0, None, None, 1, 2, None]):
        if j is None:
            assert q["iterations"][c] == 0 and q["converged"][c] and q["nhist"][c] == 1 and q["hist"][0, c] == 0.0 and not q["X"][:, c].any()
        else:
            assert np.array_equal(q["X"][:, c], singles[j]["x"]) and q["nhist"][c] == len(singles[j]["hist"])
    assert q["trace"][0] == [4, 1]                     # slot 0 took columns 0, 2, 3 (zero: refilled again at once) and then 4; slot 1 column 1
    q = ref.queue(A, Winv, np.zeros((N, 7)), B, 3, RED, 2)
    assert (q["iterations"] == 2).all() and (q["nhist"] == 5).all() and not q["converged"].any()
    assert q["trace"] == [[0, 1, 2]] * 2 + [[3, 4, 5]] * 2 + [[6, -1, -1]] * 2
    for j in range(7):
        s = ref.single(A, Winv, np.zeros(N), B[:, j], RED, 2)
        assert np.array_equal(q["X"][:, j], s["x"]) and np.array_equal(q["hist"][:5, j], s["hist"])
    Xs = np.random.default_rng(1).standard_normal((N, 7))
    q = ref.queue(A, Winv, Xs, B, 3, RED, 0)
    assert (q["iterations"] == 0).all() and (q["nhist"] == 1).all() and np.array_equal(q["X"], Xs) and not q["trace"]
    q = ref.queue(A, Winv, Xs, B, 3, RED, MAXIT)
    for j in range(7):
        s = ref.single(A, Winv, Xs[:, j], B[:, j], RED, MAXIT)
        assert np.array_equal(q["X"][:, j], s["x"]) and np.array_equal(q["hist"][:len(s["hist"]), j], s["hist"])


def test_breakdown_checks_fire_on_the_same_operands():
    """a hand-made 2 x 2 system whose <rt, v> is exactly 0 (A a quarter turn, W = I, b = e_1: v = A b is orthogonal to rt = b): the single
    loop and the queue stop on h = 0.0 before alpha = rho_new / h is formed; the queue names the caller's column.  With A = I the same
    right-hand side converges in its first half step, so the column before the bad one is stored and keeps its result."""
    A = np.array([[0.0, 1.0], [-1.0, 0.0]])
    W = np.eye(2)
    b = np.array([1.0, 0.0])
    with pytest.raises(ref.Breakdown) as e1:
        ref.single(A, W, np.zeros(2), b, RED, 10)
    assert e1.value.scalar == "h" and e1.value.value == 0.0 and e1.value.column is None
    B = np.stack([2.0 * b, np.array([0.0, 1.0]), b], axis=1)
    for width in (1, 2, 3):
        with pytest.raises(ref.Breakdown) as e2:
            ref.queue(A, W, np.zeros((2, 3)), B, width, RED, 10)
        assert (e2.value.scalar, e2.value.value, e2.value.column) == ("h", 0.0, 0), width    # slots are visited in ascending order
    # rho and omega: the operands are the ones the direction update is about to use -- a slot whose scalars are fresh (1, 1) passes,
    # and the checks come in the single loop's order (rho, omega, then h)
    Ai = np.array([[1.0, 2.0], [0.0, 1.0]])
    s = ref.single(Ai, W, np.zeros(2), b, RED, 10)
    q = ref.queue(Ai, W, np.zeros((2, 1)), b[:, None], 1, RED, 10)
    assert s["converged"] and np.array_equal(q["X"][:, 0], s["x"]) and q["nhist"][0] == len(s["hist"])
