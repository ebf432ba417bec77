"""CPU checks of the single-launch block solve (engine `xcd` of the multi-RHS path; no GPU needed): the plan tables of
ddm_trsv_multi_plan_host -- what build_schedule (csrc/tri_levels.hpp) adds to the level engine -- against tests/trsv_cases.level_table
on every factor of tests/trsv_cases.py, the shape conditions tests/test_gpu_trsv_multi_xcd.py relies on, the team arithmetic of the
kernel (ddm_trsv_multi_team_host), and the prototypes and argument checks of the new entry points."""
import ctypes
import os

import numpy as np
import pytest

from tests import trsv_cases as tc
from tests import trsv_multi_cases as mc

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ddm_hip.h")


# ---- plan tables -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.NAMES + ("loop8",))
def test_plan_tables_match_the_level_table(ddm, name):
    """per triangle: the range of block b in level l has Triangle.m[l] rows (none beyond the block's last level), the ranges tile every
    level of the merged schedule (first range starts at 0, last ends at the level's row count), the level counts match"""
    c = mc.case(name)
    nb = len(c.block_ptr) - 1
    for upper in (False, True):
        off, bn = ddm.trsv_multi_plan_host(c.M, c.block_ptr, upper)
        whole = c.whole.blocks[0][1 if upper else 0]
        assert off.shape == (whole.nlev, nb + 1) and bn.shape == (nb,)
        assert np.all(off[:, 0] == 0) and np.array_equal(off[:, nb], whole.m)          # the ranges tile every level
        assert np.all(np.diff(off, axis=1) >= 0)
        for b in range(nb):
            t = c.table.blocks[b][1 if upper else 0]
            assert bn[b] == t.nlev, (name, upper, b)
            rows = off[:, b + 1] - off[:, b]
            assert np.array_equal(rows[:t.nlev], t.m) and not rows[t.nlev:].any(), (name, upper, b)


def test_plan_positions_are_the_rows_of_the_block(ddm):
    """on blocks9: position p of level l holds the p-th row (ascending) of that level; the rows of positions off[l, b] .. off[l, b + 1]
    are exactly the rows of block b with that level"""
    c = mc.case("blocks9")
    bp = np.asarray(c.block_ptr)
    for upper in (False, True):
        off, bn = ddm.trsv_multi_plan_host(c.M, c.block_ptr, upper)
        level = np.concatenate([c.table.blocks[b][1 if upper else 0].level for b in range(len(bp) - 1)])
        for l in range(off.shape[0]):
            rows = np.flatnonzero(level == l)                                          # ascending: the order of build_schedule
            for b in range(len(bp) - 1):
                mine = rows[off[l, b]:off[l, b + 1]]
                assert np.array_equal(mine, rows[(rows >= bp[b]) & (rows < bp[b + 1])])


def test_plan_refuses_malformed_patterns(ddm):
    import scipy.sparse as sp
    c = mc.case("blocks3")
    with pytest.raises(ValueError):
        ddm.trsv_multi_plan_host(c.M, [0, c.n - 1], False)                              # does not cover the matrix
    with pytest.raises(ValueError):
        ddm.trsv_multi_plan_host(c.M, [0, 10, 5, c.n], False)                           # decreasing
    M = sp.csr_matrix(np.array([[1.0, 1.0], [1.0, 0.0]]))
    M.eliminate_zeros()
    with pytest.raises(ValueError):
        ddm.trsv_multi_plan_host(M, [0, 2], False)                                      # no diagonal entry in row 1


# ---- the shapes the GPU tests rely on --------------------------------------------------------------------------------------------
def test_shape_conditions_of_the_gpu_tests():
    # more items in a level than one XCD team has threads at m = 32 (quad items: rows * 8): band17 as the issue counts it ...
    assert mc.max_block_level_rows(mc.case("band17")) * 32 // 4 > mc.XCD_TEAM_THREADS
    # ... but band17's one team spans the chip; a second item per thread needs more items than the threads of the case's OWN team
    assert mc.max_block_level_rows(mc.case("band17")) * 32 // 4 <= mc.team_threads(mc.case("band17"))
    loop = mc.case("loop8")
    assert len(loop.block_ptr) - 1 == 8 and mc.team_threads(loop) == mc.XCD_TEAM_THREADS
    assert all(int(t.m.max()) * 32 // 4 > mc.XCD_TEAM_THREADS for t in loop.table.triangles)     # quad form, m = 32
    assert all(int(t.m.max()) * 7 < mc.XCD_TEAM_THREADS for t in loop.table.triangles)           # (the scalar widths take one item)
    assert loop.n <= tc.MAX_N and not mc.has_wide_level(loop)
    # 600 consecutive one-row levels
    chain = mc.case("chain600")
    assert all(t.nlev == 600 and int(t.m.max()) == 1 for t in chain.table.triangles)
    # blocks with different level counts, in both triangles; an XCD with two blocks; uneven teams
    for name in ("blocks3", "blocks9", "blocks17"):
        c = mc.case(name)
        assert len({b[0].nlev for b in c.table.blocks}) > 1 and len({b[1].nlev for b in c.table.blocks}) > 1, name
    assert mc.teams(mc.case("blocks3")) == 3 and mc.teams(mc.case("blocks9")) == 8 and mc.teams(mc.case("band17")) == 1
    # the declined cases have a level of w >= 96, the others none
    for name in tc.NAMES + ("loop8",):
        assert mc.has_wide_level(mc.case(name)) == (name in ("wide", "layers")), name


# ---- team arithmetic -------------------------------------------------------------------------------------------------------------
def _all_workgroups(ddm, tickets, nblocks, force_one=False):
    out, gt = [], 0
    for x in range(8):
        for t in range(tickets[x]):
            out.append((x, ddm.trsv_multi_team_host(tickets, nblocks, x, t, gt, force_one)))
            gt += 1
    return out


@pytest.mark.parametrize("nblocks", range(1, 18))
def test_teams_with_full_tickets(ddm, nblocks):
    """32 workgroups on every XCD: T = min(nblocks, 8) teams, XCD x in team x % T, sizes 32 times the XCDs of the team, ranks a
    permutation of 0 .. size - 1 per team"""
    tickets = [32] * 8
    T = min(nblocks, 8)
    wgs = _all_workgroups(ddm, tickets, nblocks)
    ranks = {t: [] for t in range(T)}
    for x, tm in wgs:
        assert tm["teams"] == T and tm["team"] == x % T and not tm["one_team"]
        assert tm["size"] == 32 * sum(1 for y in range(8) if y % T == x % T)
        ranks[tm["team"]].append(tm["rank"])
    for t in range(T):
        assert sorted(ranks[t]) == list(range(32 * sum(1 for y in range(8) if y % T == t)))


@pytest.mark.parametrize("nblocks", [3, 5, 7])
def test_uneven_teams(ddm, nblocks):
    """uneven tickets and T = 3, 5, 7 (teams of different numbers of XCDs): sizes are the ticket sums, ranks a permutation"""
    tickets = [31, 33, 32, 30, 34, 32, 29, 35]
    wgs = _all_workgroups(ddm, tickets, nblocks)
    for t in range(nblocks):
        mine = [tm for x, tm in wgs if x % nblocks == t]
        size = sum(tickets[x] for x in range(8) if x % nblocks == t)
        assert all(tm["team"] == t and tm["size"] == size and tm["teams"] == nblocks for tm in mine)
        assert sorted(tm["rank"] for tm in mine) == list(range(size))
    assert len({tm["size"] for _, tm in wgs}) > 1


@pytest.mark.parametrize("tickets, nblocks, force", [([8, 0, 8, 8, 8, 8, 8, 8], 8, False), ([8, 0, 8, 8, 8, 8, 8, 8], 17, False), ([0, 0, 0, 0, 256, 0, 0, 0], 2, False),
                                                     ([32] * 8, 9, True), ([32] * 8, 1, True)])
def test_an_empty_team_or_the_debug_mode_gives_one_team(ddm, tickets, nblocks, force):
    wgs = _all_workgroups(ddm, tickets, nblocks, force)
    grid = sum(tickets)
    assert all(tm["one_team"] and tm["teams"] == 1 and tm["team"] == 0 and tm["size"] == grid for _, tm in wgs)
    assert sorted(tm["rank"] for _, tm in wgs) == list(range(grid))


def test_an_empty_xcd_in_a_team_of_several_keeps_the_teams(ddm):
    """XCD 1 hosts nothing, 3 blocks: team 1 = XCDs 1, 4, 7 still has workgroups"""
    tickets = [8, 0, 8, 8, 8, 8, 8, 8]
    wgs = _all_workgroups(ddm, tickets, 3)
    assert all(not tm["one_team"] and tm["teams"] == 3 for _, tm in wgs)
    assert sorted(tm["rank"] for x, tm in wgs if x % 3 == 1) == list(range(16))


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
def test_prototypes_header_and_null_arguments(ddm):
    lib = ddm.load_library()
    P, I, L, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint32
    assert ddm.SYMBOLS["ddm_ilu0_set_multi_engine"] == (I, [P, P, I])
    assert ddm.SYMBOLS["ddm_ilu0_multi_info"] == (I, [P, P, L, P])
    assert ddm.SYMBOLS["ddm_schwarz_set_multi_engine"] == (I, [P, I])
    assert ddm.SYMBOLS["ddm_schwarz_set_multi_engine"] == ddm.SYMBOLS["ddm_schwarz_set_multi_precision"]
    assert ddm.SYMBOLS["ddm_trsv_multi_plan_host"] == (I, [L, P, P, L, P, I, P, L, P, P])
    assert ddm.SYMBOLS["ddm_trsv_multi_team_host"] == (I, [P, I, I, I, U, U, U, P])
    header = open(HEADER).read()
    for name in ("ddm_ilu0_set_multi_engine", "ddm_ilu0_multi_info", "ddm_schwarz_set_multi_engine", "ddm_trsv_multi_plan_host", "ddm_trsv_multi_team_host"):
        assert getattr(lib, name) is not None
        assert "int " + name + "(" in header, name
    assert "DDM_TRSV_MULTI_MODE" in header
    assert callable(ddm.Ilu0.set_multi_engine) and callable(ddm.Ilu0.multi_info) and callable(ddm.SchwarzPreconditioner.set_multi_engine)
    assert ddm.MULTI_ENGINES[:2] == ("levels", "xcd")
    for mode in (0, 1, 2, 3, -1):
        assert lib.ddm_ilu0_set_multi_engine(None, None, mode) == ddm.DDM_EINVAL
        assert lib.ddm_schwarz_set_multi_engine(None, mode) == ddm.DDM_EINVAL
    assert "ddm_ilu0_set_multi_engine" in lib.ddm_last_error(None).decode()
    cnt = ctypes.c_int64()
    assert lib.ddm_ilu0_multi_info(None, None, 0, ctypes.byref(cnt)) == ddm.DDM_EINVAL
    nlev = ctypes.c_int64()
    assert lib.ddm_trsv_multi_plan_host(0, None, None, 1, None, 0, None, 0, None, ctypes.byref(nlev)) == ddm.DDM_EINVAL
    assert lib.ddm_trsv_multi_team_host(None, 1, 0, 0, 0, 0, 8, None) == ddm.DDM_EINVAL


def test_two_level_schwarz_takes_the_keyword():
    """TwoLevelSchwarz(..., multi_engine="levels") is the default; the C++ adaptor reads [schwarz] multi_engine"""
    import inspect
    from dune_ddm_amd.solver import TwoLevelSchwarz
    assert inspect.signature(TwoLevelSchwarz.__init__).parameters["multi_engine"].default == "levels"
    hh = open(os.path.join(os.path.dirname(HEADER), "..", "dune-ddm_amd", "dune", "ddm", "hip", "schwarz.hh")).read()
    assert 'subtree.get("multi_engine", std::string("levels"))' in hh and "ddm_schwarz_set_multi_engine" in hh


def test_multi_engine_adaptor_compiles_and_links(ddm):
    from tests.cpp_harness import build, ddm_symbols_used
    ddm.load_library()
    used = ddm_symbols_used(build("./build/multi_engine_adaptor"))
    assert "ddm_schwarz_set_multi_engine" in used and "ddm_ilu0_multi_info" in used and all(u in ddm.SYMBOLS for u in used), used
