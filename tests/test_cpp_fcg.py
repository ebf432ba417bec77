"""Dune::HipRestartedFCGSolver and Dune::HipCompleteFCGSolver (dune/ddm/hip/solvers.hh; [solver] type = restartedfcgsolver /
completefcgsolver) compiled against the mock DUNE headers (tests/cpp/mock) through the pattern rule of tests/cpp/Makefile: getHipSolver
returns them for the two keys, their single-vector and block applies are bitwise what ddm_fcg_solve / ddm_fcg_solve_multi compute on
the same device objects, with the iteration counts the Python drivers give on the same problem, and apply_queue throws
Dune::NotImplemented."""
import numpy as np
import pytest

from tests.cpp_harness import build, ddm_symbols_used, dump_one_rank_problem, run

# the program needs no entry in the Makefile: "./build/<name>" is a target of its pattern rule $(OUT)/%, and build() returns that path
TARGET = "./build/fcg_adaptor"
M = 3


def test_fcg_adaptor_compiles_and_links(ddm, tmp_path):
    ddm.load_library()
    used = ddm_symbols_used(build(TARGET))
    assert "ddm_fcg_solve" in used and "ddm_fcg_solve_multi" in used and all(u in ddm.SYMBOLS for u in used), used


def seeded_columns(b, dirichlet, m):
    """seeded_columns of tests/cpp/adaptor_fixture.hh: the problem's b, then pseudo-random columns that are zero on the Dirichlet rows"""
    n = len(b)
    B = np.zeros((n, m))
    s = 12345
    for c in range(m):
        for i in range(n):
            s = (s * 6364136223846793005 + 1442695040888963407) % 2**64
            r = (s >> 11) / 9007199254740992.0 - 0.5
            B[i, c] = b[i] if c == 0 else (0.0 if dirichlet[i] else r)
    return B


@pytest.mark.gpu
def test_fcg_adaptor_matches_the_c_abi_bitwise(ddm, tmp_path):
    from dune_ddm_amd import synth
    from dune_ddm_amd.problem import build_structured
    from dune_ddm_amd.solver import TwoLevelSchwarz
    exe = build(TARGET)
    dec = build_structured(synth.StructuredPoisson((14, 13, 12), (1, 1, 1)), overlap=1, pou_type="distance")
    sd = dec.subs[0]
    dump_one_rank_problem(tmp_path, sd)
    # the iteration counts of the Python drivers on the same one-rank problem and columns (restricted ILU(0) Schwarz + POU, multiplicative)
    tl = TwoLevelSchwarz(dec, coarse="pou", schwarz_type="restricted", mode="multiplicative")
    B = seeded_columns(np.asarray(sd.b, dtype=np.float64), np.asarray(sd.dirichlet_ovlp) > 0, M)
    expected = []
    for solver in ("restartedfcgsolver", "completefcgsolver"):
        res1, hist1, x1 = tl.solve(reduction=1e-10, maxit=500, solver=solver, mmax=3)
        res, hist, X = tl.solve_multi(B, reduction=1e-10, maxit=500, solver=solver, mmax=3)
        assert res1.converged and all(r.converged for r in res)
        expected += [res1.iterations] + [r.iterations for r in res]
    tl.prec.check_status()
    tl.ctx.close()
    p = run(exe, tmp_path, M, *expected)
    out = p.stdout
    assert "factory restartedfcgsolver 1" in out and "factory completefcgsolver 1" in out and "fcg_ok" in out, out[-2000:] + p.stderr[-2000:]
    assert "queue restartedfcgsolver 1" in out and "queue completefcgsolver 1" in out
    single = [ln.split() for ln in out.splitlines() if ln.startswith("single ")]
    cols = [ln.split() for ln in out.splitlines() if ln.startswith("col ")]
    assert len(single) == 2 and all(s[2] == s[3] == s[4] and s[5:] == ["0", "0"] for s in single), single
    assert len(cols) == 2 * M and all(c[3] == c[4] == c[5] and c[6:] == ["0", "0"] for c in cols), cols
