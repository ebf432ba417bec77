"""-m gpu: the ILU(0) solve of the box engine (k_box_sweep and its companions, csrc/trsv_box.hpp; builder and enqueue:
csrc/trsv_box_host.hpp, csrc/engine_box.hpp) at the shapes its builder and its kernel branch on, with values that are independent per
entry, each with DDM_BOX_SPREAD = 0 (XCD-local hand-overs where 8 or more blocks allow them) and 1 (write-through).

The cases, what each reaches and the proof that it does -- on the host builder's own output -- are in tests/box_cases.py and
tests/test_box_cases_reference.py (CPU), which also shows that losing one stream value or one product breaks both checks below.
Which case reaches which branch:

  shell entries per box row   ext20: rows of every count 0 .. 20, so all ten product slots q = 0 .. 9 are read and the early exit
                              __any(mycnt > 2q) is taken at every q; the 20 | 21 edge: ext20 and shrink20 (20, accepted), shrink (21 in the
                              last plane: that plane is given back), ext21_mid (21 in plane 1: declined); ext_odd: every odd count, the
                              padded product
  geometry edges              nx = 2: thin1024, tall70; nx = 3: nx3, thin1023; nx = 120 | 121: nx120 | nx121 (declined); ny = 64 | 65:
                              ny64 | ny65; ny = 128 | 129: ny128 | ny129; ny = 512, eight lines per lane, and MAX_STEPS 1024 | 1026:
                              thin1024 | thin1026 (declined), 1023: thin1023; nz = 2: nz2 (and the thin and nx cases); more planes than
                              workgroups that serve the block: tall70 (test_planes_retaken); 64 | 63 rows: tiny64 | tiny63 (declined);
                              zero, one and two turns of the step loop past the last step: see test_the_table_as_a_whole (CPU)
  detect giving planes back   shrink, shrink20 (the rows of the plane become rows behind the box, the last kept plane gets nine more
                              shell entries per row), and inside hetero7 .. hetero17
  the declines                fewer than two conforming planes: ext21_mid (ends on xcd2: 34 upper entries), one_declines; less than half
                              of the block: half_ok | half; one block of several declines: one_declines (the whole matrix goes to pipe)
  blocks of different shapes  hetero4, hetero7, hetero8, hetero9, hetero17: sh_tab reloaded with another table per block, both sides of
                              the eight-block switch of local_ok / gcount
  the folded tail             test_tail: x * scale + add of the upper sweep and of k_box_shell_out, at row level
  the diagnostic path         test_stamped_solve (DDM_BOX_CHECK=1, P.dbg)
  the nested factor's engine  pipe: every case with rows behind the box; xcd2: shell_wide; levels: test_nested_levels

Per solve:

  (a) tc.Residual(M, F.factors()).ratio(d, x, 2^-53) <= C = 2 (w_L + w_U + 3) (derivation: trsv_cases.bound);
  (b) bit equality with the oracle's sequential solve: the box engine sums every row in ascending column order.

F.engine() must be exactly box_cases.EXPECT[name], and F.box_info() what the CPU reference proved things about.  No case is skipped
or filtered at run time."""
import numpy as np
import pytest

from tests import box_cases as bc
from tests import pipe_cases as pc
from tests import trsv_cases as tc

pytestmark = pytest.mark.gpu

U64 = 2.0 ** -53
BOX_ENV = ("DDM_BOX_SPREAD", "DDM_BOX_GRID", "DDM_BOX_CHECK", "DDM_BOX_DEBUG", "DDM_BOX_SHELL_LEVELS",
           "DDM_PIPE_DELTA", "DDM_PIPE_SPAN", "DDM_PIPE_REUSE", "DDM_PIPE_WG_PER_CU", "DDM_PIPE_SPREAD")   # the device must build what the CPU test proved things about


def _box_mode(monkeypatch, spread, **extra):
    for v in BOX_ENV:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("DDM_TRSV_MODE", "box")
    monkeypatch.setenv("DDM_BOX_SPREAD", spread)
    for k, v in extra.items():
        monkeypatch.setenv(k, v)


def _factor(ddm, ctx, c, lu_ref):
    F = ddm.Ilu0(ctx, ddm.CsrMatrix(ctx, c.M), c.block_ptr)
    lu = F.factors()
    dev = float(np.max(np.abs(lu - lu_ref)) / np.max(np.abs(lu_ref)))
    assert dev < 1e-13, dev                                     # same elimination order on the host
    return F, lu


def _default_grid():
    import torch
    return 2 * (torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8)   # build_box_engine


def _check_info(F, name, grid, nested):
    """the device built exactly what the CPU reference proved things about"""
    info = F.box_info()
    want = [B.figures for B in bc.built(name).blocks] if bc.EXPECT[name] == "box" else []
    assert info["blocks"] == want, (name, info["blocks"], want)
    if want:
        assert info["grid"] == grid and info["nested"] == nested, (name, info["grid"], grid, info["nested"], nested)
    return info


def _differs(x, want):
    bad = x != want
    return f"{int(bad.sum())} of {len(x)} entries differ from the oracle" + (f", first at row {int(np.flatnonzero(bad)[0])}" if bad.any() else "")


@pytest.mark.parametrize("spread", ["0", "1"])
@pytest.mark.parametrize("name", bc.NAMES)
def test_solve(ddm, name, spread, monkeypatch):
    """factors against the oracle's; three solves into a NaN-filled x -- the capture, a replay, a replay with another right-hand
    side -- with status 0 after each; the engine the case table names; the builder's figures; checks (a) and (b); the replay equals
    the first solve"""
    import torch
    _box_mode(monkeypatch, spread)
    ref = bc.ref(name)
    c = ref.c
    ctx = ddm.torch_context(0)
    F, lu = _factor(ddm, ctx, c, ref.lu)
    res = tc.Residual(c.M, lu)
    dd = [torch.tensor(d).cuda() for d in ref.d]
    xd = torch.empty(c.n, dtype=torch.float64, device="cuda")
    got = []
    for k in (0, 0, 1):
        xd.fill_(float("nan"))
        F.solve(dd[k], xd)
        ctx.sync()
        assert F.status() == 0, (name, spread, F.engine(), len(got), F.status())
        got.append((k, xd.cpu().numpy().copy()))
    engine = F.engine()
    assert engine == bc.EXPECT[name], (name, spread, engine)
    _check_info(F, name, _default_grid(), bc.NESTED.get(name))
    for rep, (k, x) in enumerate(got):
        ratio = res.ratio(ref.d[k], x, U64)
        print(f"\n{name} spread {spread} (engine {engine}) solve {rep}: residual ratio {ratio:.2f} (C = {c.C}), {_differs(x, ref.x[k])}")
        assert ratio <= c.C, (name, spread, engine, rep, ratio, c.C)
        assert np.array_equal(x, ref.x[k]), (name, spread, engine, rep, _differs(x, ref.x[k]))
    assert np.array_equal(got[0][1], got[1][1]), (name, spread, engine, "replay differs from the first solve")
    ctx.close()


@pytest.mark.parametrize("spread", ["0", "1"])
@pytest.mark.parametrize("name", bc.TAIL)
def test_tail(ddm, name, spread, monkeypatch):
    """the folded tail of a Schwarz level at row level: Ilu0.solve_tail with scale only, add only, both and neither, each call made
    twice (capture and replay), into a NaN-filled x; bit-equal to (x_oracle * scale) + add in numpy -- two roundings: the kernels are
    compiled with contraction off.  Box rows get it from the upper sweep, the rows behind the box from k_box_shell_out."""
    import torch
    _box_mode(monkeypatch, spread)
    ref = bc.ref(name)
    c = ref.c
    rng = np.random.default_rng(53)
    scale, add = rng.standard_normal(c.n), rng.standard_normal(c.n)
    assert (ref.d[0] != 0).all() and (scale != 0).all() and (add != 0).all()
    ctx = ddm.torch_context(0)
    F, _ = _factor(ddm, ctx, c, ref.lu)
    d, sd, ad = (torch.tensor(v).cuda() for v in (ref.d[0], scale, add))
    xd = torch.empty(c.n, dtype=torch.float64, device="cuda")
    for use_scale, use_add in ((True, False), (False, True), (True, True), (False, False)):
        want = ref.x[0]
        if use_scale:
            want = want * scale
        if use_add:
            want = want + add
        for rep in range(2):
            xd.fill_(float("nan"))
            F.solve_tail(d, xd, sd if use_scale else None, ad if use_add else None)
            ctx.sync()
            assert F.status() == 0 and F.engine() == "box", (name, spread, use_scale, use_add, rep, F.status(), F.engine())
            x = xd.cpu().numpy()
            print(f"\n{name} spread {spread} scale {use_scale} add {use_add} call {rep}: {_differs(x, want)}")
            assert np.array_equal(x, want), (name, spread, use_scale, use_add, rep, _differs(x, want))
    ctx.close()


@pytest.mark.parametrize("spread", ["0", "1"])
@pytest.mark.parametrize("name", bc.CHAINED)
def test_ten_solves_back_to_back(ddm, name, spread, monkeypatch):
    """hand-overs under load on 9 and 17 blocks of different shapes (XCD 0 owns two or three): 10 solves enqueued back to back, each
    on the previous result, against 10 oracle solves"""
    import torch
    _box_mode(monkeypatch, spread)
    ref = bc.ref(name)
    c = ref.c
    ctx = ddm.torch_context(0)
    F, _ = _factor(ddm, ctx, c, ref.lu)
    a = torch.tensor(ref.d[0]).cuda()
    b = torch.full_like(a, float("nan"))
    for _ in range(10):
        F.solve(a, b)
        a, b = b, a
    ctx.sync()
    assert F.status() == 0 and F.engine() == "box", (name, spread, F.status(), F.engine())
    x = ref.d[0]
    for _ in range(10):
        x = pc.oracle_solve(ref.f, x)
    got = a.cpu().numpy()
    print(f"\n{name} spread {spread}: {_differs(got, x)} after 10 solves")
    assert np.array_equal(got, x), (name, spread)
    ctx.close()


def _solve_twice(ddm, ctx, name, spread):
    import torch
    ref = bc.ref(name)
    F, _ = _factor(ddm, ctx, ref.c, ref.lu)
    d = torch.tensor(ref.d[0]).cuda()
    xd = torch.empty_like(d)
    for rep in range(2):
        xd.fill_(float("nan"))
        F.solve(d, xd)
        ctx.sync()
        assert F.status() == 0 and F.engine() == "box", (name, spread, rep, F.status(), F.engine())
        x = xd.cpu().numpy()
        assert np.array_equal(x, ref.x[0]), (name, spread, rep, _differs(x, ref.x[0]))
    return F


@pytest.mark.parametrize("spread", ["0", "1"])
@pytest.mark.parametrize("name,grid", [("tall70", "8"), ("hetero9", "8"), ("tall70", None)])
def test_planes_retaken(ddm, name, grid, spread, monkeypatch):
    """DDM_BOX_GRID=8: eight workgroups serve the 70 planes of tall70 (alone, and as a block of hetero9), so by counting a workgroup
    takes further plane tickets; tall70 also at the default grid, where with spread 0 only the workgroups of one XCD serve the block.

    This cannot wait forever: a workgroup takes a ticket of one (block, sweep) queue and walks that plane at once, to its end, before
    it takes another; tickets are handed out in plane order; every workgroup of the launch is resident once the start barrier
    (st->arrived == gridDim.x) has passed.  The holder of plane K - 1 is therefore running that plane or done with it, and it waits
    for nothing but plane K - 2: the chain ends at plane 0, which waits for nothing.  (Every wait is bounded by BOX_SPIN_LIMIT as well
    and ends in a status word, not a hang.)"""
    _box_mode(monkeypatch, spread, **({"DDM_BOX_GRID": grid} if grid else {}))
    ctx = ddm.torch_context(0)
    F = _solve_twice(ddm, ctx, name, spread)
    info = _check_info(F, name, int(grid) if grid else _default_grid(), bc.NESTED[name])
    assert max(b[2] for b in info["blocks"]) == 70 and (grid is None or info["grid"] == 8 < 70)
    ctx.close()


@pytest.mark.parametrize("spread", ["0", "1"])
@pytest.mark.parametrize("name", ["tall70", "hetero9"])
def test_stamped_solve(ddm, name, spread, monkeypatch):
    """the diagnostic path (DDM_BOX_CHECK=1, P.dbg): status 0 and the oracle's bits; Ilu0.box_check() for block 0: per sweep and plane
    start <= end and an XCC id below 8, zeros beyond nz; with spread 0 and eight or more blocks every plane of block 0 ran on one XCD"""
    _box_mode(monkeypatch, spread, DDM_BOX_CHECK="1")
    ctx = ddm.torch_context(0)
    F = _solve_twice(ddm, ctx, name, spread)
    nz = F.box_info()["blocks"][0][2]
    st = F.box_check().astype(np.int64)
    assert st.shape == (2, 128, 4)
    for sweep in (0, 1):
        assert (st[sweep, :nz, 0] > 0).all() and (st[sweep, :nz, 0] <= st[sweep, :nz, 1]).all(), (name, spread, sweep, st[sweep, :nz, :2])
        assert ((st[sweep, :nz, 3] >= 0) & (st[sweep, :nz, 3] < 8)).all(), (name, spread, sweep, st[sweep, :nz, 3])
        assert not st[sweep, nz:].any(), (name, spread, sweep)
        if spread == "0" and bc.case(name).nblocks >= 8:
            assert len(set(st[sweep, :nz, 3].tolist())) == 1, (name, sweep, st[sweep, :nz, 3])
    ctx.close()


@pytest.mark.parametrize("name", ["ext20", "shell_wide"])
def test_nested_levels(ddm, name, monkeypatch):
    """the rows behind the box on the level kernels (DDM_BOX_SHELL_LEVELS=1) give the same bits as on the single-launch engine the
    nested factor settles on otherwise (pipe for ext20, xcd2 for shell_wide); box_info names the nested engine in both settings"""
    for levels in (False, True):
        _box_mode(monkeypatch, "0", **({"DDM_BOX_SHELL_LEVELS": "1"} if levels else {}))
        ctx = ddm.torch_context(0)
        F = _solve_twice(ddm, ctx, name, "0")
        _check_info(F, name, _default_grid(), "levels" if levels else bc.NESTED[name])
        ctx.close()
