"""-m gpu: the rank-local passes of the single-vector Schwarz apply (k_defect_gather, k_halo_sum_restrict) and the CG loop without its
one-workgroup launches (k_dot_fin, k_cg_update_norm_fin, k_cg_direction_beta) against the general path, which DDM_FUSE_LOCAL=0 selects
when the objects are created.  The new kernels make the same copies, the same additions in the same order and the same divisions on the
same operands, so every comparison is of bit patterns (torch.equal on the int64 views: NaN payloads and the sign of zero count)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SCAL = dict(RHOLAST=0, PQ=1, STEP=2, RHO=3, BETA=4, DEF2=5)     # csrc/kernels.hpp
WG, RED_TRIPS, HALO_TRIPS, RED_MAX_BLOCKS = 256, 4, 8, 1024

CASES = ["9x8x7-overlap1", "9x8x7-overlap2", "islands-2x1x2", "one-subdomain"]


def bits(t):
    import torch
    return (t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))).view(torch.int64).cpu()


def same_bits(a, b):
    import torch
    return torch.equal(bits(a), bits(b))


def from_device(ctx, ptr, n):
    out = np.empty(n, dtype=np.float64)
    ctx.check(ctx.lib.ddm_memcpy_d2h(ctx.h, out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr), 8 * n))
    return out


def scalars(ctx):
    return from_device(ctx, ctx.lib.ddm_ctx_scalars(ctx.h), 6)


def schwarz_state(tl):
    """(applies through the tables?, pointer to d_ovlp, pointer to x_ovlp)"""
    loc, d, x = ctypes.c_int(), ctypes.c_void_p(), ctypes.c_void_p()
    tl.ctx.check(tl.ctx.lib.ddm_schwarz_debug_local(tl.ctx.h, tl.schwarz.h, ctypes.byref(loc), ctypes.byref(d), ctypes.byref(x)))
    return bool(loc.value), d.value, x.value


def build_pair(monkeypatch, name):
    """the problem once; on it the solver objects with the rank-local passes and with the general path"""
    from dune_ddm_amd import synth
    from dune_ddm_amd.problem import build_structured
    from dune_ddm_amd.solver import TwoLevelSchwarz
    if name == "islands-2x1x2":
        grid, overlap = synth.StructuredPoisson((9, 8, 7), (2, 1, 2), synth.islands_kappa((8, 7, 6), 1e4, 4, 2)), 2
    elif name == "one-subdomain":
        grid, overlap = synth.StructuredPoisson((9, 8, 7), (1, 1, 1)), 2
    else:
        grid, overlap = synth.StructuredPoisson((9, 8, 7), (2, 2, 2)), int(name[-1])
    dec = build_structured(grid, overlap=overlap, pou_type="distance", shrink=0)
    coarse = "none" if name == "one-subdomain" else "pou"      # (one subdomain: the Schwarz level alone, its restriction is the apply's last pass too)
    out = {}
    for fuse in ("1", "0"):
        monkeypatch.setenv("DDM_FUSE_LOCAL", fuse)
        tl = TwoLevelSchwarz(dec, coarse=coarse, schwarz_type="standard", mode="additive")
        tl.schwarz.wait_setup()
        assert schwarz_state(tl)[0] == (fuse == "1")
        out[fuse] = tl
    return out["1"], out["0"]


@pytest.mark.parametrize("name", CASES)
def test_apply_and_cg_are_bit_identical(ddm, monkeypatch, name):
    import torch
    new, old = build_pair(monkeypatch, name)
    n, nov = new.rl.n_o, new.rl.n
    rng = np.random.default_rng(len(name))
    for rep in range(2):
        d = rng.standard_normal(n)
        res = {}
        for tag, tl in (("new", new), ("old", old)):
            x = torch.full((n,), float("nan"), dtype=torch.float64, device=tl.dev)
            dd = tl.to_device(d)
            tl.prec.apply(x, dd)
            tl.ctx.sync()
            tl.prec.check_status()
            res[tag] = (from_device(tl.ctx, schwarz_state(tl)[1], nov), x)
        assert np.isfinite(res["old"][0]).all() and torch.isfinite(res["old"][1]).all()
        assert same_bits(res["new"][0], res["old"][0])          # d_ov
        assert same_bits(res["new"][1], res["old"][1])          # z
    for k in (1, 3):
        runs = {}
        for tag, tl in (("new", new), ("old", old)):
            x, b = tl.zeros(n), tl.to_device(tl.rl.b)
            cg = ddm.CgIteration(tl.ctx, tl.op, tl.prec, x, b)
            cg.steps(k)
            deff = cg.defect()
            tl.prec.check_status()
            runs[tag] = (x, b, np.array([deff]), scalars(tl.ctx))
            cg.end()
        assert np.isfinite(runs["old"][2]).all() and torch.isfinite(runs["old"][0]).all() and runs["old"][2][0] > 0.0
        for i, what in enumerate(("x", "b", "defect", "scalars (rho, <p, q>, lambda, beta, rholast, <b, b>)")):
            assert same_bits(runs["new"][i], runs["old"][i]), (what, k)
    if name != "one-subdomain":   # two calls: the deferred defect norm rides on the coarse all-reduce inside a call and not across calls
        counts = {}
        for tag, tl in (("new", new), ("old", old)):
            x, b = tl.zeros(n), tl.to_device(tl.rl.b)
            c0 = tl.ctx.comm_counts()
            cg = ddm.CgIteration(tl.ctx, tl.op, tl.prec, x, b)
            cg.steps(2)
            cg.steps(3)
            cg.defect()
            cg.end()
            counts[tag] = [int(a - b0) for a, b0 in zip(tl.ctx.comm_counts(), c0)]
        assert counts["new"] == counts["old"]                   # all-reduces, their doubles and halo exchanges are counted as before


def tail_trips(n, trips=RED_TRIPS):
    """(workgroups, trips of the loop that keeps `trips` rows of a thread in flight, trips of the tail loop) of thread 0 of workgroup 0
    in the reduction kernels (RED_TRIPS: k_dot_partial, k_dot_fin; HALO_TRIPS: k_halo_sum_restrict)"""
    nb = min(RED_MAX_BLOCKS, max(1, -(-n // (4 * WG))))
    step, i, loop, tail = nb * WG, 0, 0, 0
    while i + (trips - 1) * step < n:
        i, loop = i + trips * step, loop + 1
    while i < n:
        i, tail = i + step, tail + 1
    return nb, loop, tail


SIZES = [1, WG - 1, WG, 4 * WG, 4 * WG + 1, 4 * WG * RED_MAX_BLOCKS + 77, 11 * WG * RED_MAX_BLOCKS - 7]


def test_sizes_cover_the_branches():
    assert tail_trips(4 * WG) == (1, 1, 0) and tail_trips(4 * WG + 1) == (2, 0, 3)          # 0 and 3 tail trips; 1 and 2 workgroups
    assert tail_trips(1)[0] == 1 and tail_trips(SIZES[-2]) == (RED_MAX_BLOCKS, 1, 1)       # the capped grid: more partials than threads of a workgroup
    # k_halo_sum_restrict takes HALO_TRIPS rows of a thread at a time, the last group clamped: below the cap a thread has at most four
    # rows; the largest size gives thread 0 eleven (a full group and one of three), the last threads ten
    assert tail_trips(SIZES[-1], HALO_TRIPS) == (RED_MAX_BLOCKS, 1, 3) and tail_trips(SIZES[-1]) == (RED_MAX_BLOCKS, 2, 3)


@pytest.fixture(scope="module")
def ctx(ddm):
    return ddm.torch_context(0)


@pytest.mark.parametrize("masked", [True, False], ids=["masked", "unmasked"])
@pytest.mark.parametrize("n", SIZES)
def test_self_finishing_reductions(ddm, ctx, n, masked):
    """each reduction kernel alone against the kernels it stands in for, twice in a row with nothing between the launches (the second
    launch finds the ticket its predecessor put back)"""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(n)
    P = ddm._ptr

    def vec(m=n):
        return torch.from_numpy(rng.standard_normal(m)).to(dev)
    mask = torch.from_numpy((rng.random(n) < 0.7).astype(np.uint8)).to(dev) if masked else None
    mp = P(mask) if masked else None
    # tables of the sum + restriction: row m of z owns row perm[m] of an overlapping vector of n + 5 rows and adds 0 .. 3 more
    nov = n + 5
    own = rng.permutation(nov)[:n].astype(np.int32)
    ncp = rng.integers(0, 4, n) * (rng.random(n) < 0.3)
    cp_ptr = np.concatenate([[0], np.cumsum(ncp)]).astype(np.int32)
    cp_idx = rng.integers(0, nov, max(int(cp_ptr[-1]), 1)).astype(np.int32)
    t_own, t_ptr, t_idx = (torch.from_numpy(a).to(dev) for a in (own, cp_ptr, cp_idx))
    lib = ctx.lib

    def run(kind, fin, a, b, c, d, first, out):
        ctx.check(lib.ddm_debug_reduction(ctx.h, kind, fin, n, mp, P(a), P(b), P(c) if c is not None else None, P(d) if d is not None else None, first,
                                          P(t_own), P(t_ptr), P(t_idx), P(out)))

    scal_ptr = lib.ddm_ctx_scalars(ctx.h)
    x, y, x2, y2, p, q, xov, xov2 = vec(), vec(), vec(), vec(), vec(), vec(), vec(nov), vec(nov)
    for first in (1, 0):
        got = {}
        for fin in (1, 0):
            init = np.zeros(6)
            init[SCAL["PQ"]], init[SCAL["RHO"]], init[SCAL["RHOLAST"]] = 3.7, (7.0 if first else 1.3), 1.9
            ctx.check(lib.ddm_memcpy_h2d(ctx.h, ctypes.c_void_p(scal_ptr), init.ctypes.data_as(ctypes.c_void_p), 48))
            o = torch.full((4, 3), float("nan"), dtype=torch.float64, device=dev)
            a, b, z1, z2 = x.clone(), y.clone(), torch.full((n,), float("nan"), dtype=torch.float64, device=dev), torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
            run(0, fin, x, y, None, None, first, o[0])          # the dot product, twice
            run(0, fin, x2, y2, None, None, first, o[1])
            run(2, fin, z1, y, xov, None, first, o[2])          # the sum + restriction with its dot product, twice
            run(2, fin, z2, y2, xov2, None, first, o[3])
            o2 = torch.full((2, 3), float("nan"), dtype=torch.float64, device=dev)
            run(1, fin, a, b, p, q, first, o2[0])               # the update with its norm, twice (the second on the first's result)
            run(1, fin, a, b, p, q, 0, o2[1])
            ctx.sync()
            got[fin] = (o[:, 0].clone(), o2, a, b, z1, z2)
        assert torch.isfinite(got[0][0]).all() and torch.isfinite(got[0][1]).all()
        for i, what in enumerate(("dots", "norm, lambda, rholast", "x", "b", "z", "z (second)")):
            assert same_bits(got[1][i], got[0][i]), (what, first)
    # the sum itself against numpy: the same additions in list order
    xh = xov.cpu().numpy()
    want = xh[own].copy()
    for j in range(3):
        rows = np.nonzero(ncp > j)[0]
        want[rows] = want[rows] + xh[cp_idx[cp_ptr[rows] + j]]
    assert same_bits(got[1][4], want)


@pytest.mark.parametrize("name", ["9x8x7-overlap2", "islands-2x1x2"])
def test_sum_of_copies_makes_the_same_additions(ddm, monkeypatch, name):
    """-0.0, an infinity and a NaN among the copies of overlap rows: the one pass adds what pack + unpack + restrict add, in their order"""
    import torch
    monkeypatch.setenv("DDM_FUSE_LOCAL", "1")
    new, _ = build_pair(monkeypatch, name)
    tl = new
    n, nov = tl.rl.n_o, tl.rl.n
    maps = ddm.local_maps_host(nov, n, tl.rl.ext_map, tl.rl.plan_ovlp_copy, tl.rl.plan_ovlp_add)
    rng = np.random.default_rng(7)
    xov = rng.standard_normal(nov)
    shared = np.nonzero(np.diff(maps["cp_ptr"]) > 0)[0]               # non-overlapping rows with copies elsewhere
    assert len(shared) > 8
    rows = rng.choice(shared, 8, replace=False)
    xov[maps["own_of"][rows[0]]] = -0.0                               # -0.0 + -0.0 = -0.0, but 0.0 + -0.0 = 0.0: the first term is the owner's
    xov[maps["cp_idx"][maps["cp_ptr"][rows[0]]:maps["cp_ptr"][rows[0] + 1]]] = -0.0
    xov[maps["own_of"][rows[1]]] = -0.0
    xov[maps["cp_idx"][maps["cp_ptr"][rows[2]]]] = np.inf
    xov[maps["own_of"][rows[3]]] = -np.inf
    xov[maps["cp_idx"][maps["cp_ptr"][rows[4] + 1] - 1]] = np.nan
    xov[maps["own_of"][rows[5]]] = np.inf                             # inf + -inf: a NaN made by the addition itself
    xov[maps["cp_idx"][maps["cp_ptr"][rows[5]]]] = -np.inf
    r = tl.to_device(rng.standard_normal(n))
    xd = tl.to_device(xov)
    mask = torch.from_numpy(np.ascontiguousarray(tl.rl.owner_novlp, dtype=np.uint8)).to(tl.dev)
    res = {}
    for general in (0, 1):
        z = torch.full((n,), 123.0, dtype=torch.float64, device=tl.dev)
        out = torch.zeros(1, dtype=torch.float64, device=tl.dev)
        tl.ctx.check(tl.ctx.lib.ddm_schwarz_debug_sum_restrict(tl.ctx.h, tl.schwarz.h, ddm._ptr(xd), general, ddm._ptr(mask), ddm._ptr(r), ddm._ptr(z), ddm._ptr(out)))
        tl.ctx.sync()
        res[general] = (z, out)
    assert torch.isnan(res[1][0]).any() and torch.isinf(res[1][0]).any()
    assert (bits(res[1][0]) == bits(torch.tensor([-0.0], dtype=torch.float64))[0]).any()
    assert same_bits(res[0][0], res[1][0]) and same_bits(res[0][1], res[1][1])
