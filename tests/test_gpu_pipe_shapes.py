"""-m gpu: the ILU(0) solve of the pipe engine (k_trsv_pipe, csrc/trsv_pipe.hpp) at the shapes its schedule builder and its kernel
branch on: row widths at 14 | 15, 20 | 21 and 26 | 27 in either sweep, wide halves with ring and with gathered operands, tiles of
different sizes following each other, own results 15, 16 and 17 steps old, exactly 112 producer tasks, a regrouped and a dissolved
schedule, tasks of 1, 2 and 3 steps, packed rows, re-used lanes, and 1 .. 17 uneven blocks on both sides of the nb < 8 switch, each
with DDM_PIPE_SPREAD = 0 (XCD-local hand-overs where 8 or more blocks allow them) and 1 (write-through).

The cases, what each reaches and the proof that it does -- on the host builder's own output, with the options the device uses --
are in tests/pipe_cases.py and tests/test_pipe_cases_reference.py (CPU), which also shows that losing one operand of any of these
classes breaks both checks below.  Per solve:

  (a) tc.Residual(M, F.factors()).ratio(d, x, 2^-53) <= C = 2 (w_L + w_U + 3) (derivation: trsv_cases.bound);
  (b) bit equality with the oracle's sequential solve: pipe sums every row in ascending column order.

F.engine() must be exactly pipe_cases.EXPECT[name]: "pipe", or "xcd2" for the matrices the builder declines (a builder that starts
declining a case would otherwise be tested on another engine without anyone noticing).  No case is skipped or filtered at run time.
test_stamped_solve runs the kernel's stamped instantiation (the diagnostic build behind tools/pipe_trace.py) on three of the cases."""
import numpy as np
import pytest

from tests import pipe_cases as pc
from tests import trsv_cases as tc

pytestmark = pytest.mark.gpu

U64 = 2.0 ** -53
SCHEDULE_ENV = ("DDM_PIPE_DELTA", "DDM_PIPE_SPAN", "DDM_PIPE_REUSE", "DDM_PIPE_WG_PER_CU")   # the device must build what the CPU test proved things about


def _pipe_mode(monkeypatch, spread):
    for v in SCHEDULE_ENV:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("DDM_TRSV_MODE", "pipe")
    monkeypatch.setenv("DDM_PIPE_SPREAD", spread)


def _factor(ddm, ctx, c, lu_ref):
    F = ddm.Ilu0(ctx, ddm.CsrMatrix(ctx, c.M), c.block_ptr)
    lu = F.factors()
    dev = float(np.max(np.abs(lu - lu_ref)) / np.max(np.abs(lu_ref)))
    assert dev < 1e-13, dev                                     # same elimination order on the host
    return F, lu


@pytest.mark.parametrize("spread", ["0", "1"])
@pytest.mark.parametrize("name", pc.NAMES)
def test_solve(ddm, name, spread, monkeypatch):
    """factors against the oracle's; three solves into a NaN-filled x -- the capture, a replay, a replay with another right-hand
    side -- with status 0 after each; the engine the case table names; checks (a) and (b); the replay equals the first solve"""
    import torch
    _pipe_mode(monkeypatch, spread)
    ref = pc.ref(name)
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
    assert engine == pc.EXPECT[name], (name, spread, engine)
    for rep, (k, x) in enumerate(got):
        ratio = res.ratio(ref.d[k], x, U64)
        bad = int(np.sum(x != ref.x[k]))
        print(f"\n{name} spread {spread} (engine {engine}) solve {rep}: residual ratio {ratio:.2f} (C = {c.C}), {bad} of {c.n} entries differ from the oracle"
              + (f", first at row {int(np.flatnonzero(x != ref.x[k])[0])}" if bad else ""))
        assert ratio <= c.C, (name, spread, engine, rep, ratio, c.C)
        assert np.array_equal(x, ref.x[k]), (name, spread, engine, rep, bad)
    assert np.array_equal(got[0][1], got[1][1]), (name, spread, engine, "replay differs from the first solve")
    ctx.close()


@pytest.mark.parametrize("spread", ["0", "1"])
@pytest.mark.parametrize("name", pc.CHAINED)
def test_ten_solves_back_to_back(ddm, name, spread, monkeypatch):
    """hand-overs under load on 9 and 17 uneven blocks (XCD 0 owns two or three): 10 solves enqueued back to back, each on the
    previous result, against 10 oracle solves"""
    import torch
    _pipe_mode(monkeypatch, spread)
    ref = pc.ref(name)
    c = ref.c
    ctx = ddm.torch_context(0)
    F, lu = _factor(ddm, ctx, c, ref.lu)
    a = torch.tensor(ref.d[0]).cuda()
    b = torch.full_like(a, float("nan"))
    for _ in range(10):
        F.solve(a, b)
        a, b = b, a
    ctx.sync()
    assert F.status() == 0 and F.engine() == "pipe", (name, spread, F.status(), F.engine())
    x = ref.d[0]
    for _ in range(10):
        x = pc.oracle_solve(ref.f, x)
    got = a.cpu().numpy()
    print(f"\n{name} spread {spread}: {int(np.sum(got != x))} of {c.n} entries differ from 10 oracle solves")
    assert np.array_equal(got, x), (name, spread)
    ctx.close()


STAMPED = ("mix9", "w26", "chains65")   # 9 uneven blocks (XCD-local mode); both wide halves; a dissolved schedule of 1 .. 3-step tasks


@pytest.mark.parametrize("spread", ["0", "1"])
@pytest.mark.parametrize("name", STAMPED)
def test_stamped_solve(ddm, name, spread, monkeypatch):
    """the stamped instantiation of the kernel (F.pipe_trace, tools/pipe_trace.py): status 0, x bit-equal to the oracle, and per task
    the 16-word layout (csrc/trsv_pipe.hpp, STAMP): [6] = the task's steps in the host builder's schedule, [0] <= [1] <= [2],
    [7] an XCC id, the unused words [5] and [10] zero, store times [16 ..] non-decreasing over the first min(steps, 256) steps"""
    import torch
    _pipe_mode(monkeypatch, spread)
    ref = pc.ref(name)
    c = ref.c
    ctx = ddm.torch_context(0)
    F, _ = _factor(ddm, ctx, c, ref.lu)
    d = torch.tensor(ref.d[0]).cuda()
    xd = torch.full_like(d, float("nan"))
    st, meta = F.pipe_trace(d, xd)
    ctx.sync()
    assert F.status() == 0, (name, spread, F.status())
    x = xd.cpu().numpy()
    assert np.array_equal(x, ref.x[0]), (name, spread, int(np.sum(x != ref.x[0])))
    tasks = pc.schedule(name).tasks
    assert len(st) == len(tasks) and meta[:, 1].tolist() == [t[0] for t in tasks] and meta[:, 0].tolist() == [t[1] for t in tasks]
    st = st.astype(np.int64)
    for q, (_, _, _, widths) in enumerate(tasks):
        nsteps = len(widths)
        assert st[q, 6] == nsteps, (name, spread, q, int(st[q, 6]), nsteps)
        assert st[q, 0] <= st[q, 1] <= st[q, 2], (name, spread, q, st[q, :3].tolist())
        assert 0 <= st[q, 7] < 8, (name, spread, q, int(st[q, 7]))
        assert st[q, 5] == 0 and st[q, 10] == 0, (name, spread, q, int(st[q, 5]), int(st[q, 10]))
        assert (np.diff(st[q, 16:16 + min(nsteps, 256)]) >= 0).all(), (name, spread, q)
    ctx.close()
