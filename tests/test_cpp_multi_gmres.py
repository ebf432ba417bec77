"""Dune::HipRestartedGMResSolver's block apply (std::vector<X> of right-hand sides -> ddm_gmres_solve_multi) compiled against the mock
DUNE headers (tests/cpp/mock) through tests/cpp/Makefile, and run against column-by-column device solves of the same
adaptor."""
import pytest

from tests.cpp_harness import build, ddm_symbols_used, dump_one_rank_problem, run


def test_block_gmres_adaptor_compiles_and_links(ddm, tmp_path):
    ddm.load_library()
    used = ddm_symbols_used(build("multi_gmres_adaptor"))
    assert "ddm_gmres_solve_multi" in used and all(u in ddm.SYMBOLS for u in used), used


@pytest.mark.gpu
def test_block_gmres_adaptor_matches_column_solves(ddm, tmp_path):
    from dune_ddm_amd import synth
    from dune_ddm_amd.problem import build_structured
    exe = build("multi_gmres_adaptor")
    dec = build_structured(synth.StructuredPoisson((14, 13, 12), (1, 1, 1)), overlap=1, pou_type="distance")
    sd = dec.subs[0]
    dump_one_rank_problem(tmp_path, sd)
    p = run(exe, tmp_path, 3)
    assert "block_ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    cols = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("col ")]
    assert len(cols) == 3 and all(c[2] == c[3] for c in cols), cols
