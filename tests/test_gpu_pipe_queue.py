"""-m gpu: the pipe engine with tasks queued in front of producers (csrc/trsv_pipe_host.hpp, "Queue order"; the bound per queue:
csrc/engine_pipe.hpp).  The device's default order, the creation order (DDM_PIPE_MOVE=0) and the level engine must give the same
bits, with tasks really moved.  The orders run here are the ones tests/test_pipe_queue_order.py accepts on the CPU with the fewest
workgroups per queue that the builder's argument allows."""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

SCHEDULE_ENV = ("DDM_PIPE_DELTA", "DDM_PIPE_SPAN", "DDM_PIPE_REUSE", "DDM_PIPE_WG_PER_CU", "DDM_PIPE_MOVE", "DDM_PIPE_MOVE_GAP")   # the device must build what the CPU test proved things about


def _blocks(N, P):
    from dune_ddm_amd import synth
    from dune_ddm_amd.problem import build_structured
    dec = build_structured(synth.StructuredPoisson(N, P), overlap=2, pou_type="distance", shrink=0)
    mats = [sd.A_dir.tocsr() for sd in dec.subs]
    M = sp.block_diag(mats, format="csr")
    M.sort_indices()
    return M, np.concatenate([[0], np.cumsum([m.shape[0] for m in mats])]).astype(np.int64)


def _solve(ddm, M, bp, d, monkeypatch, mode, move=None):
    """(x on the device after two solves, status, engine, pipe_info or None)"""
    import torch
    monkeypatch.setenv("DDM_TRSV_MODE", mode)
    if move is None:
        monkeypatch.delenv("DDM_PIPE_MOVE", raising=False)
    else:
        monkeypatch.setenv("DDM_PIPE_MOVE", move)
    ctx = ddm.torch_context(0)
    F = ddm.Ilu0(ctx, ddm.CsrMatrix(ctx, M), bp)
    dd = torch.as_tensor(d).cuda()
    x = torch.full((M.shape[0],), float("nan"), dtype=torch.float64, device="cuda")
    for _ in range(2):                                           # (the second solve: a new epoch on used progress words)
        x.fill_(float("nan"))
        F.solve(dd, x)
    ctx.sync()
    out = (x.clone(), F.status(), F.engine(), F.pipe_info() if mode == "pipe" else None)
    ctx.close()
    return out


@pytest.mark.parametrize("N,P,spread,bound", [((64, 64, 64), (2, 2, 2), "0", 32),      # one queue per XCD
                                              ((48, 48, 48), (3, 2, 2), "0", 16),      # 12 subdomains: two queues on four of the XCDs
                                              ((64, 64, 64), (2, 2, 2), "1", 32)])     # write-through hand-overs, subdomains not bound to XCDs
def test_moved_queue_order_gives_the_same_bits(ddm, N, P, spread, bound, monkeypatch):
    import torch
    assert torch.cuda.is_available()
    for k in SCHEDULE_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("DDM_PIPE_SPREAD", spread)
    M, bp = _blocks(N, P)
    d = np.random.default_rng(5).standard_normal(M.shape[0])
    x_moved, st, eng, info = _solve(ddm, M, bp, d, monkeypatch, "pipe")
    assert st == 0 and eng == "pipe"
    print(f"\n{N} / {P} spread {spread}: grid {info['grid']}, bound {info['move_max']}, moved {info['moved_forward']}+{info['moved_backward']} "
          f"of {info['ntasks']} tasks, most in one queue {info['max_moved']}")
    nb = len(bp) - 1
    per_queue = min((info["grid"] // 8) // ((nb + 7) // 8), info["grid"] // nb)  # workgroups that start on one queue (engine_pipe.hpp)
    assert info["spread"] == int(spread) and info["move_max"] == min(per_queue // 2, 32) > 0
    if info["grid"] == 512:                                      # two workgroups on each of 256 CUs: 64 per XCD
        assert info["move_max"] == bound
    assert info["moved_forward"] + info["moved_backward"] > 0 and 0 < info["max_moved"] <= bound
    assert int(info["moved"].sum()) == info["moved_forward"] + info["moved_backward"]
    x_base, st, eng, info0 = _solve(ddm, M, bp, d, monkeypatch, "pipe", move="0")
    assert st == 0 and eng == "pipe"
    assert info0["move_max"] == 0 and info0["moved_forward"] + info0["moved_backward"] == 0 and not info0["moved"].any()
    x_lev, st, eng, _ = _solve(ddm, M, bp, d, monkeypatch, "levels")
    assert st == 0 and eng == "levels"
    assert bool(torch.isfinite(x_moved).all())
    assert torch.equal(x_moved, x_base)
    assert torch.equal(x_moved, x_lev)
