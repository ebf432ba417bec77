"""Dune::HipBlockGMResSolver (dune/ddm/hip/solvers.hh; [solver] type = blockgmressolver) compiled against the mock DUNE headers
(tests/cpp/mock) through the pattern rule of tests/cpp/Makefile: getHipSolver returns it for the key, its block apply and its
single-vector apply (the block of width 1) are bitwise what ddm_bgmres_solve_multi computes on the same device objects, with the
iteration counts the Python path (TwoLevelSchwarz.solve_block_gmres) gives on the same problem, apply_queue throws
Dune::NotImplemented and minressolver is still refused with a message that names the new type.  The adaptor fixture drives one rank
with one subdomain, so the problem is the golden problem's 12^3 grid as a single subdomain; restricted Schwarz and the multiplicative
combination make the preconditioner non-symmetric; restart 6 makes the solves restart."""
import numpy as np
import pytest

from tests.cpp_harness import build, ddm_symbols_used, dump_one_rank_problem, run
from tests.test_cpp_fcg import seeded_columns

# the program needs no entry in the Makefile: "./build/<name>" is a target of its pattern rule $(OUT)/%, and build() returns that path
TARGET = "./build/bgmres_adaptor"
M = 3


def test_bgmres_adaptor_compiles_and_links(ddm, tmp_path):
    ddm.load_library()
    used = ddm_symbols_used(build(TARGET))
    assert "ddm_bgmres_solve_multi" in used and all(u in ddm.SYMBOLS for u in used), used


@pytest.mark.gpu
def test_bgmres_adaptor_matches_the_c_abi_bitwise(ddm, tmp_path):
    from dune_ddm_amd import synth
    from dune_ddm_amd.problem import build_structured
    from dune_ddm_amd.solver import TwoLevelSchwarz
    exe = build(TARGET)
    dec = build_structured(synth.StructuredPoisson((12, 12, 12), (1, 1, 1)), overlap=1, pou_type="distance")
    sd = dec.subs[0]
    dump_one_rank_problem(tmp_path, sd)
    # the iteration counts of the Python path on the same one-rank problem and columns (restricted ILU(0) Schwarz + POU, multiplicative)
    tl = TwoLevelSchwarz(dec, coarse="pou", schwarz_type="restricted", mode="multiplicative")
    B = seeded_columns(np.asarray(sd.b, dtype=np.float64), np.asarray(sd.dirichlet_ovlp) > 0, M)
    res1, hist1, X1, widths1 = tl.solve_block_gmres(B[:, :1].copy(), reduction=1e-10, maxit=500, restart=6)
    res, hist, X, widths = tl.solve_block_gmres(B, reduction=1e-10, maxit=500, restart=6)
    assert res1[0].converged and all(r.converged for r in res) and widths[0] == M and len(widths) > 6
    expected = [res1[0].iterations] + [r.iterations for r in res]
    tl.prec.check_status()
    tl.ctx.close()
    p = run(exe, tmp_path, M, *expected)
    out = p.stdout
    assert "factory 1" in out and "queue 1" in out and "errors_caught 1" in out and "bgmres_ok" in out, out[-2000:] + p.stderr[-2000:]
    single = [ln.split() for ln in out.splitlines() if ln.startswith("single ")]
    cols = [ln.split() for ln in out.splitlines() if ln.startswith("col ")]
    assert len(single) == 1 and single[0][1] == single[0][2] == single[0][3] and single[0][4:] == ["0", "0"], single
    assert len(cols) == M and all(c[2] == c[3] == c[4] and c[5:] == ["0", "0"] for c in cols), cols
