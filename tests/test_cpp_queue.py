"""Dune::HipCGSolver::apply_queue (std::vector<X> of right-hand sides through a block of fixed width -> ddm_cg_solve_queue) compiled
against the mock DUNE headers (tests/cpp/mock) through tests/cpp/Makefile, and run against TwoLevelSchwarz.solve_many on the
same problem and columns."""
import numpy as np
import pytest

from tests.cpp_harness import build, ddm_symbols_used, dump_one_rank_problem, run

XTOL = 1e-8          # x of a block column against another solve of it (tests/test_gpu_multi_rhs.py)


def test_queue_adaptor_compiles_and_links(ddm, tmp_path):
    ddm.load_library()
    used = ddm_symbols_used(build("queue_adaptor"))
    assert "ddm_cg_solve_queue" in used and all(u in ddm.SYMBOLS for u in used), used


@pytest.mark.gpu
def test_queue_adaptor_matches_solve_many(ddm, tmp_path):
    """M = 9 columns through w = 4 slots: iteration counts equal those of solve_many on the same columns, x within 1e-8 of the
    largest entry; the adaptor leaves b as it was and refuses an empty column list and a width of 33."""
    from dune_ddm_amd import synth
    from dune_ddm_amd.problem import build_structured
    from dune_ddm_amd.solver import TwoLevelSchwarz
    M, w = 9, 4
    exe = build("queue_adaptor")
    dec = build_structured(synth.StructuredPoisson((14, 13, 12), (1, 1, 1)), overlap=1, pou_type="distance")
    sd = dec.subs[0]
    dump_one_rank_problem(tmp_path, sd, b=False)
    # right-hand sides: the problem's, then seeded random ones that are zero on the Dirichlet rows like the problem's
    R = np.random.default_rng(12345).standard_normal((sd.n, M - 1)) * (sd.dirichlet_ovlp == 0)[:, None]
    B = np.ascontiguousarray(np.concatenate([sd.b.astype(np.float64)[:, None], R], axis=1))
    B.tofile(tmp_path / "rhs.bin")
    p = run(exe, tmp_path, M, w)
    assert "queue_ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    assert "b_unchanged 1" in p.stdout and "errors_caught 2" in p.stdout
    cols = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("col ")]
    assert len(cols) == M
    Xc = np.fromfile(tmp_path / "x_queue.bin", dtype=np.float64).reshape(sd.n, M)
    tl = TwoLevelSchwarz(dec, coarse="pou", schwarz_type="standard", mode="additive")
    assert tl.rl.n_o == sd.n
    res, _, X = tl.solve_many(B, width=w, reduction=1e-10, maxit=500)
    Xh = X.cpu().numpy()
    for j in range(M):
        assert int(cols[j][2]) == res[j].iterations and cols[j][3] == "1" and res[j].converged == 1, (j, cols[j], res[j].iterations)
        assert np.max(np.abs(Xc[:, j] - Xh[:, j])) <= XTOL * np.max(np.abs(Xh[:, j])), j
    tl.ctx.close()
