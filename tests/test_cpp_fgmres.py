"""Dune::HipRestartedFlexibleGMResSolver (dune/ddm/hip/solvers.hh; [solver] type = restartedflexiblegmressolver) compiled against the
mock DUNE headers (tests/cpp/mock) through tests/cpp/Makefile: getHipSolver returns it for the new key, and its
single-vector and block applies are bitwise what ddm_fgmres_solve / ddm_fgmres_solve_multi compute on the same device objects."""
import pytest

from tests.cpp_harness import build, ddm_symbols_used, dump_one_rank_problem, run


def test_fgmres_adaptor_compiles_and_links(ddm, tmp_path):
    ddm.load_library()
    used = ddm_symbols_used(build("fgmres_adaptor"))
    assert "ddm_fgmres_solve" in used and "ddm_fgmres_solve_multi" in used and all(u in ddm.SYMBOLS for u in used), used


@pytest.mark.gpu
def test_fgmres_adaptor_matches_the_c_abi_bitwise(ddm, tmp_path):
    from dune_ddm_amd import synth
    from dune_ddm_amd.problem import build_structured
    exe = build("fgmres_adaptor")
    dec = build_structured(synth.StructuredPoisson((14, 13, 12), (1, 1, 1)), overlap=1, pou_type="distance")
    sd = dec.subs[0]
    dump_one_rank_problem(tmp_path, sd)
    p = run(exe, tmp_path, 3)
    assert "factory 1" in p.stdout and "fgmres_ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    single = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("single ")]
    cols = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("col ")]
    assert len(single) == 1 and single[0][1] == single[0][2] and single[0][3:] == ["0", "0"], single
    assert len(cols) == 3 and all(c[2] == c[3] and c[4:] == ["0", "0"] for c in cols), cols
