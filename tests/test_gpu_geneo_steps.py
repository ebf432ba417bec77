"""-m gpu: the device steps of the GenEO block eigensolver (GeneoRun, csrc/geneo.hpp) one by one, called as the eigensolver calls
them: on slots of n x 3m arrays S = [X | W | P] with ld = 3m and on the n x m residual block, through the exports that forward to
the eigensolver's own host functions (csr_mm_ld, csr_adopt + csr_mm2_ld, ilu0_solve_multi_ld, GeneoWork::gram / rotate, the
launch_geneo_* functions).  The end-to-end tests (tests/test_gpu_geneo.py) compare converged eigenpairs; a block iteration with a
Rayleigh-Ritz step repairs a slightly wrong step at the price of iterations, and GeneoRun::refresh() recomputes the products the
rotation carries, so those tests cannot see such an error.  These can.

The cases, the reason for every width and the host references are in tests/geneo_step_cases.py; tests/test_geneo_step_cases_reference.py
(CPU) pins them.  Every output block is wider than its target and pre-filled with NaN (or with recorded values where the step reads
it); every test asserts that nothing outside the target columns and no input changed.

  products    csr_mm_ld and csr_mm2_ld on the X, W and P slots, for a pair with the cache-blocked row order and one created under
              DDM_SPMM_NATURAL_ORDER=1: EQUAL BITS with the float64 restatement of the row sums in entry order (both outputs).
  solves      ilu0_solve_multi_ld(D = n x m, ldd = m; X = W slot, ldx = 3m) for the ILU(0) factor (double and single-precision
              sweeps) and the host-engine direct factor: equal bits with the contiguous call on the same factor (which
              tests/test_gpu_trsv_shapes.py and tests/test_gpu_direct_host_shapes.py pin to their references); for the device
              supernodal factor (atomic adds) the residual criterion of tests/sn_cases.py for both and for their difference.  Graph
              cache: a contiguous call, then the same two pointers with ldx = 3m, must give the strided result; a replay equal bits.
  Gram        R^T R, (A~X)^T (A~X) with ld = 3m (U == V: SAME = true of k_gram_small, or k_gram_mfma) and R^T W with mixed
              strides, within 1e-13 sum |a| |b| + 1e-300 of the float64 host product.
  rotation    three different arrays through one launch set with gap_from = gap = m (the Rayleigh-Ritz step) and W <- W - X G in
              place on one array (the orthogonalisation), within 1e-13 |U| |Y| (+ |W|).
  helpers     k_geneo_random / residual / copy_cols / rowscale / finalize: equal bits with the numpy expression;
              k_geneo_invsqrt_diag: within 1 ulp of 1.0 / np.sqrt(g) -- measured on an MI355X: every entry EQUAL at every width (the
              test prints it), so the device's double sqrt and division round as numpy's do on these values.

Measured on one MI355X: every bit comparison holds at every width (nowhere did equal bits have to give way to a bound); Gram
products at most 0.048, rotations 0.004 of their bounds; supernodal factor at 52 columns: ratio 5.8e-3 (chain1d) and 2.4e-3 (lu13)
for both calls, difference 0.  What the tests notice (an experiment, not committed): a library with args.U[1] / args.U[2] swapped
and the `+ gap` dropped in k_rotate_mfma, `va` read for `va2` in k_spmm_rowmajor4_tiled<true> and `ldd` in place of `ldx` in the
gathers of k_trsv_level_multi4 fails test_block_products[8 .. 32, tiled], test_strided_solves_ilu0[8 .. 48, double] and
test_rotation_as_the_rayleigh_ritz_step_runs_it at every width, and nothing else.

No case is skipped or filtered at run time."""
import numpy as np
import pytest

from tests import geneo_step_cases as gc
from tests import sn_cases as sc

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _dev(a):
    import torch
    t = torch.as_tensor(np.array(a, order="C")).cuda()                   # (a copy: the cases' arrays are read-only)
    assert t.data_ptr() % 32 == 0                                        # what Shapes takes for granted
    return t


def _nan(*shape):
    import torch
    t = torch.full(shape, NAN, dtype=torch.float64, device="cuda")
    assert t.data_ptr() % 32 == 0
    return t


def _only(out, cols, what):
    """the host copy of a device block whose columns outside `cols` must still be NaN"""
    o = out.cpu().numpy()
    mask = np.ones(o.shape[1], dtype=bool)
    mask[cols] = False
    assert np.isnan(o[:, mask]).all(), (what, "written outside the target columns")
    return o[:, cols]


def _unchanged(t, a, what):
    assert np.array_equal(t.cpu().numpy(), a), (what, "an input changed")


# ---- block products ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["tiled", "natural"])
@pytest.mark.parametrize("m", gc.WIDTHS)
def test_block_products(ddm, m, order, monkeypatch):
    """YA = A X, YC = C X (csr_mm2_ld) and each alone (csr_mm_ld) with X, YA, YC in slot k of three ld = 3m arrays, k = X, W, P.
    All kernels add the rounded products in entry order from 0.0 (the library is built -ffp-contract=off): equal bits with
    gc.spmm_restated are required and were obtained on an MI355X at every width, slot and order -- no bound is used."""
    case = gc.sparse()
    X, ref = gc.products(m)
    sh = gc.Shapes(m)
    monkeypatch.delenv("DDM_SPMM_NATURAL_ORDER", raising=False)
    if order == "natural":
        monkeypatch.setenv("DDM_SPMM_NATURAL_ORDER", "1")
    ctx = ddm.torch_context(0)
    pair = ddm.CsrPair(ctx, case.M, case.vc, case.block_ptr)
    assert pair.has_row_order() == (order == "tiled")
    Xd = _dev(X)
    launched = set()
    for k in range(3):
        cols = gc.slot(m, k)
        kernels = sh.product_kernels(k, True, pair.has_row_order())
        assert (kernels == ["k_spmm_rowmajor4_tiled<true>"]) == (order == "tiled" and m in (8, 24, 28, 32)), (m, k, kernels)
        launched.update(kernels + sh.product_kernels(k, False, pair.has_row_order()))
        YA, YC = _nan(case.n, 3 * m), _nan(case.n, 3 * m)
        pair.mm2_ld(Xd[:, cols], YA[:, cols], YC[:, cols])
        ctx.sync()
        assert np.array_equal(_only(YA, cols, "YA"), ref[k, "A"]), (m, k, order, "A X differs from the sums in entry order")
        assert np.array_equal(_only(YC, cols, "YC"), ref[k, "C"]), (m, k, order, "C X differs from the sums in entry order")
        for second, name in ((False, "A"), (True, "C")):
            Y = _nan(case.n, 3 * m)
            pair.mm_ld(Xd[:, cols], Y[:, cols], second=second)
            ctx.sync()
            assert np.array_equal(_only(Y, cols, name), ref[k, name]), (m, k, order, name, "single product")
    _unchanged(Xd, X, "X")
    print(f"\n[geneo steps] products m = {m}, {order}: {sorted(launched)}")
    pair.close()
    ctx.close()


# ---- strided solves ----------------------------------------------------------------------------------------------------------------
def _strided_against_contiguous(ctx, F, D, m, f32, exact):
    """(contiguous result, strided result).  The contiguous solve into a block of its own; then the graph-cache sequence on ONE pair of
    pointers: contiguous (ldx = m), strided into the W slot (ldx = 3m), strided again (a replay)."""
    n = D.shape[0]
    Dd = _dev(D)
    Xc = _nan(n, m)
    F.solve_multi(Dd, Xc, single_precision=f32)
    ctx.sync()
    assert F.status() == 0
    want = Xc.cpu().numpy()
    assert np.isfinite(want).all()
    S = _nan(n, 3 * m)
    W = S[:, gc.slot(m, 1)]
    flat = S.view(-1)[m:m + n * m].view(n, m)                             # the same first element, rows of m
    assert flat.data_ptr() == W.data_ptr() and flat.is_contiguous() and W.stride(0) == 3 * m
    F.solve_multi(Dd, flat, single_precision=f32)
    ctx.sync()
    if exact:
        assert np.array_equal(flat.cpu().numpy(), want)
    S.fill_(NAN)
    F.solve_multi_ld(Dd, W, single_precision=f32)                        # same D, same X pointer, other ldx: nothing may be replayed
    ctx.sync()
    got = _only(S, gc.slot(m, 1), "W slot").copy()
    assert np.isfinite(got).all(), "the strided solve left NaN in its target (a replay of the contiguous capture?)"
    if exact:
        assert np.array_equal(got, want), "strided solve differs from the contiguous one"
        S.fill_(NAN)
        F.solve_multi_ld(Dd, W, single_precision=f32)                    # the replay
        ctx.sync()
        assert np.array_equal(_only(S, gc.slot(m, 1), "W slot"), want), "replay of the strided solve differs"
    assert F.status() == 0
    _unchanged(Dd, D, "D")
    return want, got


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("m", gc.WIDTHS)
def test_strided_solves_ilu0(ddm, m, f32):
    """W = T R as GeneoRun::search_directions runs it with the ILU(0) preconditioner: no atomics, equal bits"""
    case = gc.sparse()
    _, D = case.blocks(m)
    sh = gc.Shapes(m)
    ctx = ddm.torch_context(0)
    F = ddm.Ilu0(ctx, ddm.CsrMatrix(ctx, case.factor_matrix), case.block_ptr)
    assert ctx.lib.ddm_ilu0_is_direct(F.h) == 0
    _strided_against_contiguous(ctx, F, D, m, f32, exact=True)
    widest = int(np.diff(case.factor_matrix.indptr).max())
    print(f"\n[geneo steps] ILU(0) solve m = {m}, f32 = {f32}: strided {sh.level_kernel(f32, widest)}, contiguous {sh.level_kernel(f32, widest, contiguous=True)}")
    ctx.close()


@pytest.mark.parametrize("m", gc.WIDTHS)
def test_strided_solves_host_direct(ddm, m, monkeypatch):
    """the same with the host-engine direct factor (L U on the symmetrised pattern: block 1 is not symmetric): k_perm_gather with
    ldd = m, the level kernels on the packed panel, k_perm_scatter with ldx = 3m; no atomics, equal bits"""
    case = gc.sparse()
    _, D = case.blocks(m)
    monkeypatch.setenv("DDM_DIRECT_ENGINE", "host")
    ctx = ddm.torch_context(0)
    F = ddm.Ilu0(ctx, ddm.CsrMatrix(ctx, case.factor_matrix), case.block_ptr, direct=True, general=True)
    assert ctx.lib.ddm_ilu0_is_direct(F.h) == 1 and F.engine() == "levels" and F.refinement()[0] == 0
    want, _ = _strided_against_contiguous(ctx, F, D, m, False, exact=True)
    r = case.factor_matrix @ want - D                                    # a direct factor: the contiguous result solves the system
    assert np.abs(r).max() <= 1e-10 * np.abs(D).max()
    ctx.close()


@pytest.mark.parametrize("name", ["chain1d", "lu13"])
def test_strided_solves_supernodal(ddm, name, monkeypatch):
    """the device supernodal factor at m = 52 > 48 columns: two panels, D + c0 with ldd = m and X + c0 with ldx = 3m.  Its kernels
    add atomically, so strided and contiguous are compared through the residual criterion of tests/sn_cases.py: Evaluated.ratio <= 1
    for each, Evaluated.difference <= 1 between them, column by column."""
    m = 52
    assert m > gc.SN_PANEL == sc.PANEL and len(sc.panels(m)) == 2
    c = sc.case(name)
    c.env(monkeypatch, "default")
    ctx = ddm.torch_context(0)
    F = ddm.Ilu0(ctx, ddm.CsrMatrix(ctx, c.M), c.block_ptr, direct=True, general=c.general)
    assert ctx.lib.ddm_ilu0_is_direct(F.h) == 1 and F.engine() == "supernodal" and F.refinement()[0] == 0
    D = np.ascontiguousarray(c.D[:, :m])
    want, got = _strided_against_contiguous(ctx, F, D, m, False, exact=False)
    Ec, Es = c.evaluate(D, want), c.evaluate(D, got)
    diff = Es.difference(Ec)
    print(f"\n[geneo steps] supernodal {name}, m = {m}: ratio contiguous {Ec.ratio().max():.3e}, strided {Es.ratio().max():.3e}, difference {diff.max():.3e}")
    assert Ec.ratio().max() <= 1.0 and Es.ratio().max() <= 1.0, (Ec.ratio(), Es.ratio())
    assert diff.max() <= 1.0, diff
    ctx.close()


# ---- Gram products -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", gc.WIDTHS)
def test_gram_products_of_the_iteration(ddm, m):
    """the three call forms of GeneoRun: W.gram(R, m, m, R, m, m), W.gram(AS, ld, m, AS, ld, m) (U == V) and W.gram(R, m, m, Wb, ld, m)"""
    d = gc.dense(m)
    ctx = ddm.torch_context(0)
    Rd, Sd, ASd = _dev(d.R), _dev(d.S), _dev(d.AS)
    AXd, Wd = ASd[:, gc.slot(m, 0)], Sd[:, gc.slot(m, 1)]
    forms = (("R^T R", Rd, Rd, d.R, d.R), ("AX^T AX", AXd, AXd, d.AS[:, gc.slot(m, 0)], d.AS[:, gc.slot(m, 0)]), ("R^T W", Rd, Wd, d.R, d.S[:, gc.slot(m, 1)]))
    for what, U, V, Uh, Vh in forms:
        G = ddm.blockvec_gram(ctx, gc.SUB_PTR, U, V)
        ref, bound = gc.gram_ref(Uh, Vh)
        err = np.abs(G - ref)
        ok = err <= 1e-13 * bound + 1e-300
        print(f"\n[geneo steps] Gram m = {m} {what} ({gc.Shapes.gram_kernel(m, m, U is V)}): largest error / bound {np.max(err / (1e-13 * bound + 1e-300)):.3f}")
        assert ok.all(), (m, what, np.argwhere(~ok)[:4])
    for t, a in ((Rd, d.R), (Sd, d.S), (ASd, d.AS)):
        _unchanged(t, a, "Gram operand")
    ctx.close()


# ---- rotation ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", gc.WIDTHS)
def test_rotation_as_the_rayleigh_ritz_step_runs_it(ddm, m):
    """W.rotate(3, {S, AS, CS}, .., ld, p = 3m, Y, q = 2m, ld, ld, gap_from = m, gap = m): Out_k[:, 0:m) = U_k Y[:, 0:m),
    Out_k[:, 2m:3m) = U_k Y[:, m:2m), Out_k[:, m:2m) untouched, for three different sources and outputs"""
    d = gc.dense(m)
    ctx = ddm.torch_context(0)
    src = (d.S, d.AS, d.CS)
    U = [_dev(a) for a in src]
    out = [_nan(d.n, 3 * m) for _ in src]
    ddm.blockvec_rotate_multi(ctx, gc.SUB_PTR, U, d.Y, out, gap_from=m, gap=m)
    worst = 0.0
    for k, a in enumerate(src):
        o = out[k].cpu().numpy()
        ref, bnd = gc.rotate_ref(a, d.Y)
        assert np.isnan(o[:, gc.slot(m, 1)]).all(), (m, k, "the W slot was written")
        for name, tgt, cols in (("X", gc.slot(m, 0), slice(0, m)), ("P", gc.slot(m, 2), slice(m, 2 * m))):
            err, b = np.abs(o[:, tgt] - ref[:, cols]), 1e-13 * bnd[:, cols] + 1e-300
            assert np.all(err <= b), (m, k, name, np.argwhere(~(err <= b))[:4])
            worst = max(worst, float(np.max(err / b)))
        _unchanged(U[k], a, "rotation source")
    print(f"\n[geneo steps] rotation m = {m}: {[l[1:] for l in gc.Shapes(m).rayleigh_ritz_rotation()]}, largest error / bound {worst:.3f}")
    ctx.close()


@pytest.mark.parametrize("m", gc.WIDTHS)
def test_rotation_as_the_orthogonalisation_runs_it(ddm, m):
    """W.rotate(1, {X slot}, {W slot}, {W slot}, ld, m, G, m, ld, ld): W <- W - X G in place, Base and Out the W slot of the array
    whose X slot is U"""
    d = gc.dense(m)
    ctx = ddm.torch_context(0)
    Sd = _dev(d.S)
    Xs, Ws = Sd[:, gc.slot(m, 0)], Sd[:, gc.slot(m, 1)]
    ddm.blockvec_rotate_multi(ctx, gc.SUB_PTR, [Xs], d.G, [Ws], base=[Ws])
    s = Sd.cpu().numpy()
    ref, bnd = gc.rotate_ref(d.S[:, gc.slot(m, 0)], d.G)
    W0 = d.S[:, gc.slot(m, 1)]
    err, b = np.abs(s[:, gc.slot(m, 1)] - (W0 - ref)), 1e-13 * (np.abs(W0) + bnd)
    assert np.all(err <= b), (m, np.argwhere(~(err <= b))[:4])
    assert np.array_equal(s[:, gc.slot(m, 0)], d.S[:, gc.slot(m, 0)]) and np.array_equal(s[:, gc.slot(m, 2)], d.S[:, gc.slot(m, 2)])
    ctx.close()


# ---- helper kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", gc.WIDTHS)
def test_random_start_block(ddm, m):
    """k_geneo_random into the W slot of an ld = 3m array and into an ld = m + 1 array: the same numbers (the entry index is
    i m + j whatever the leading dimension), equal to the numpy splitmix64, seeds 0 and 1"""
    d = gc.dense(m)
    ctx = ddm.torch_context(0)
    wd = _dev(d.w)
    for seed in (0, 1):
        ref = gc.random_block(d.n, m, seed, d.w)
        for width, cols in ((3 * m, gc.slot(m, 1)), (m + 1, slice(0, m))):
            out = _nan(d.n, width)
            ddm.geneo_random(ctx, gc.SUB_PTR, seed, wd, out[:, cols])
            assert np.array_equal(_only(out, cols, "random"), ref), (m, seed, width)
    _unchanged(wd, d.w, "mask")
    ctx.close()


@pytest.mark.parametrize("m", gc.WIDTHS)
def test_residual_copy_and_rowscale(ddm, m):
    """k_geneo_residual (mu differs per subdomain; A~X and C~X the X slots of ld = 3m arrays), k_geneo_copy_cols, k_geneo_rowscale"""
    d = gc.dense(m)
    ctx = ddm.torch_context(0)
    ASd, CSd, mud, wd = _dev(d.AS), _dev(d.CS), _dev(d.mu), _dev(d.w)
    x = gc.slot(m, 0)
    out = _nan(d.n, m + 1)
    ddm.geneo_residual(ctx, gc.SUB_PTR, mud, ASd[:, x], CSd[:, x], out[:, :m])
    assert np.array_equal(_only(out, slice(0, m), "residual"), gc.residual_ref(d.mu, d.sub_of_row, d.AS[:, x], d.CS[:, x]))
    out = _nan(d.n, m + 1)
    ddm.geneo_copy_cols(ctx, gc.SUB_PTR, CSd[:, gc.slot(m, 2)], out[:, :m])
    assert np.array_equal(_only(out, slice(0, m), "copy"), d.CS[:, gc.slot(m, 2)])
    wide = np.concatenate([d.R, np.arange(d.n, dtype=np.float64)[:, None]], axis=1)
    Rw = _dev(wide)
    ddm.geneo_rowscale(ctx, gc.SUB_PTR, wd, Rw[:, :m])
    r = Rw.cpu().numpy()
    assert np.array_equal(r[:, :m], d.R * d.w[:, None]) and np.array_equal(r[:, m], wide[:, m])
    for t, a in ((ASd, d.AS), (CSd, d.CS), (mud, d.mu), (wd, d.w)):
        _unchanged(t, a, "helper operand")
    ctx.close()


@pytest.mark.parametrize("m", gc.WIDTHS)
def test_invsqrt_diag_and_finalize(ddm, m):
    """k_geneo_invsqrt_diag on diagonals of mixed size with 0.0, a negative one and 1e-301 (exactly 0.0 out); k_geneo_finalize with
    nev < m, scale rows m wide, output nev x n, one subdomain with scale 0 (exact zeros).
    invsqrt: 1 ulp against 1.0 / np.sqrt(g) is allowed; on an MI355X every entry was equal at every width."""
    d = gc.dense(m)
    ctx = ddm.torch_context(0)
    G = gc.gram_diagonals(d.nsub, m)
    Gd, sd = _dev(G), _nan(d.nsub + 1, m)
    ddm.geneo_invsqrt_diag(ctx, gc.SUB_PTR, Gd, sd[:d.nsub])
    s = sd.cpu().numpy()
    ref = gc.invsqrt_diag_ref(G)
    assert np.isnan(s[d.nsub]).all()
    s = s[:d.nsub]
    assert s[0, 0] == 0.0 and s[1, m - 1] == 0.0 and s[2, m // 2] == 0.0 and np.array_equal(s == 0.0, ref == 0.0)
    print(f"\n[geneo steps] invsqrt m = {m}: all {s.size} entries equal to 1.0 / np.sqrt(g): {np.array_equal(s, ref)}")
    assert np.all(np.abs(s - ref) <= np.spacing(ref)), np.max(np.abs(s - ref) / np.spacing(ref))
    _unchanged(Gd, G, "Gram matrices")
    nev = m - 4
    scale = d.mu.copy()
    scale[1] = 0.0
    Rd, scd = _dev(d.R), _dev(scale)
    basis = _nan(nev + 1, d.n)
    ddm.geneo_finalize(ctx, gc.SUB_PTR, scd, Rd, basis[:nev])
    b = basis.cpu().numpy()
    assert np.isnan(b[nev]).all()
    assert np.array_equal(b[:nev], gc.finalize_ref(scale, d.sub_of_row, d.R, nev))
    assert np.all(b[:nev, d.rows(1)] == 0.0) and np.all(b[:nev, d.rows(0)] != 0.0)
    _unchanged(Rd, d.R, "V")
    ctx.close()
