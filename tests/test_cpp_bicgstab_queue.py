"""Dune::HipBiCGSTABSolver::apply_queue (std::vector<X> of right-hand sides through a block of fixed width ->
ddm_bicgstab_solve_queue; apply_queue itself sits in the base class of the device Krylov solvers) compiled against the mock DUNE
headers (tests/cpp/mock) through tests/cpp/Makefile, and run against TwoLevelSchwarz.solve_many(solver="bicgstabsolver") on
the same problem and columns."""
import numpy as np
import pytest

from tests.cpp_harness import build, ddm_symbols_used, dump_one_rank_problem, run

XTOL = 1e-8          # x of a block column against another solve of it (tests/test_gpu_multi_rhs.py)


def test_bicgstab_queue_adaptor_compiles_and_links(ddm, tmp_path):
    ddm.load_library()
    used = ddm_symbols_used(build("bicgstab_queue_adaptor"))
    assert "ddm_bicgstab_solve_queue" in used and all(u in ddm.SYMBOLS for u in used), used


@pytest.mark.gpu
def test_bicgstab_queue_adaptor_matches_solve_many(ddm, tmp_path):
    """M = 9 columns through w = 4 slots, multiplicative combination: iteration counts equal those of solve_many on the same columns, x
    within 1e-8 of the largest entry; the adaptor leaves b as it was, refuses an empty column list and a width of 33, and
    HipRestartedGMResSolver::apply_queue throws Dune::NotImplemented."""
    from dune_ddm_amd import synth
    from dune_ddm_amd.problem import build_structured
    from dune_ddm_amd.solver import TwoLevelSchwarz
    M, w = 9, 4
    exe = build("bicgstab_queue_adaptor")
    dec = build_structured(synth.StructuredPoisson((14, 13, 12), (1, 1, 1)), overlap=1, pou_type="distance")
    sd = dec.subs[0]
    dump_one_rank_problem(tmp_path, sd, b=False)
    # right-hand sides: seeded random ones that are zero on the Dirichlet rows (not the problem's own: the load vector of f = 1 is a
    # genuine BiCGSTAB breakdown under the multiplicative combination, tests/test_gpu_parity.py)
    B = np.ascontiguousarray(np.random.default_rng(12345).standard_normal((sd.n, M)) * (sd.dirichlet_ovlp == 0)[:, None])
    B.tofile(tmp_path / "rhs.bin")
    p = run(exe, tmp_path, M, w)
    assert "queue_ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    assert "b_unchanged 1" in p.stdout and "errors_caught 3" in p.stdout
    cols = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("col ")]
    assert len(cols) == M
    Xc = np.fromfile(tmp_path / "x_queue.bin", dtype=np.float64).reshape(sd.n, M)
    tl = TwoLevelSchwarz(dec, coarse="pou", schwarz_type="standard", mode="multiplicative")
    assert tl.rl.n_o == sd.n
    res, _, X = tl.solve_many(B, width=w, reduction=1e-9, maxit=200, solver="bicgstabsolver")
    Xh = X.cpu().numpy()
    for j in range(M):
        assert int(cols[j][2]) == res[j].iterations and cols[j][3] == "1" and res[j].converged == 1, (j, cols[j], res[j].iterations)
        assert np.max(np.abs(Xc[:, j] - Xh[:, j])) <= XTOL * np.max(np.abs(Xh[:, j])), j
    tl.ctx.close()
