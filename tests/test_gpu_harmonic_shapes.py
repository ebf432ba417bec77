"""-m gpu: the harmonic extension ddm_harmonic (csrc/geneo.hpp) and the operators the coarse-space builders make of it -- the split
of A into A^ = [A_ii 0; 0 I], G_ib and G_bi (harmonic_create_impl), the extension and the projection P (harmonic_apply with keep /
keep_b), P^T (harmonic_apply_transposed), the T T^T operator of ddm_svd_basis (harmonic_apply_ttt) and the 48-column chunk loop of
ddm_harmonic_extend -- on BOTH direct engines (DDM_DIRECT_ENGINE=host / device), against the refined host reference of
tests/harmonic_cases.py, which also holds the cases, the widths and the reason for each; tests/test_harmonic_cases_reference.py
(CPU) pins them.  tests/test_gpu_coarse_spaces.py sees these operators only through a converged eigensolver, which repairs a
slightly wrong projection at the price of iterations.

Criterion: 1e-10 of the column's largest reference entry, per column, over the rows the operation computes (hc.column_ratio <= 1);
rows and columns an operation leaves alone are compared bit by bit; rows it defines as zero with == 0.0.  Rows an operation
overwrites are pre-filled with NaN (k_geneo_project used to multiply them by keep = 0), padding columns with a sentinel.

Measured on one MI355X, largest error / tolerance over all widths and layouts (host engine, device engine):
  extend 1.99e-4, 2.02e-4    P 1.54e-4, 1.55e-4    P^T 4.95e-5, 5.02e-5    T T^T 1.65e-4, 1.65e-4    adjoint 8.3e-8, 1.1e-7 of its bound
each reached on nearly_sym_lo, whose Cholesky factor reads one triangle of a matrix whose triangles differ by 1e-13 in one entry while
the reference takes A as given; on every other case at most 1.4e-5, 1.2e-5, 4.2e-6 and 2.1e-5.  The repetitions gave equal bits on
both engines.  What the tests notice (an experiment, not committed): with `keep[i] * X` back in k_geneo_project, test_extend and
test_projection fail on every case and engine and nothing else does; with X for X + c0 in ddm_harmonic_extend, keep for keep_b in
harmonic_apply_transposed and interior-ones for D in the last step of harmonic_apply_ttt, test_extend (every case), and
test_projection_transposed, test_t_tt_operator and test_adjoint (every case with a boundary row) fail and nothing else does.

No case is skipped or filtered at run time."""
import ctypes

import numpy as np
import pytest

from tests import harmonic_cases as hc

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = -7.25e77
ENGINES = ("host", "device")


def _dev(a):
    import torch
    t = torch.as_tensor(np.array(a, order="C")).cuda()
    assert t.data_ptr() % 32 == 0                                         # what hc.Shapes takes for granted
    return t


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _open(ddm, name, engine, monkeypatch, transpose=True):
    c = hc.case(name)
    monkeypatch.setenv("DDM_DIRECT_ENGINE", engine)
    ctx = ddm.torch_context(0)
    A = ddm.CsrMatrix(ctx, c.A)
    if c.spec.lists:
        ii, bb = hc.index_lists(c.cls)
        H = ddm.HarmonicExtension(ctx, A, ii, bb, c.block_ptr)
    else:
        H = ddm.HarmonicExtension.from_classes(ctx, A, c.cls, c.block_ptr, transpose=transpose)
    return c, ctx, H


def _slot_block(c, src, m, ld, slot, nan_rows=()):
    """an n x ld host array of sentinels with the leading m columns of src in columns slot m .. slot m + m, NaN in nan_rows there"""
    S = np.full((c.n, ld), SENTINEL)
    cols = slice(slot * m, slot * m + m)
    S[:, cols] = src[:, :m]
    for rows in nan_rows:
        S[rows, cols] = NAN
    return S, cols


def _rest_untouched(got, S, rows, cols, what):
    """everything outside got[rows, cols] has the bits of S"""
    mask = np.ones(S.shape, dtype=bool)
    mask[np.ix_(rows, np.arange(S.shape[1])[cols])] = False
    assert np.array_equal(_bits(got)[mask], _bits(S)[mask]), (what, "changed outside its output")


# ---- structure -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", hc.NAMES)
def test_structure(ddm, name, engine, monkeypatch):
    """G_ib and G_bi as the library holds them equal the slices of A entry for entry (==), the symmetric switch falls where 1e-12
    puts it, the factor is the engine's; the index-list entry point with duplicates gives what the classes give"""
    c, ctx, H = _open(ddm, name, engine, monkeypatch)
    info = H.info()
    assert info["n"] == c.n and info["symmetric"] == int(c.spec.symmetric) and info["supernodal"] == int(engine == "device")
    assert info["factor_nnz"] > 0 and info["work_cols"] == 0
    for which in ((0,) if c.spec.lists else (0, 1)):
        for got, ref in zip(H.host_matrix(which), c.embedded(bool(which))):
            assert got.dtype == ref.dtype and np.array_equal(got, ref), (name, "G_bi" if which else "G_ib")
    if c.spec.lists:
        assert info["nnz_gbi"] == -1
        with pytest.raises(ValueError):
            H.host_matrix(1)
        twin = ddm.HarmonicExtension.from_classes(ctx, ddm.CsrMatrix(ctx, c.A), c.cls, c.block_ptr)
        for got, ref in zip(H.host_matrix(0), twin.host_matrix(0)):
            assert np.array_equal(got, ref)
        assert {k: v for k, v in twin.info().items() if k != "nnz_gbi"} == {k: v for k, v in info.items() if k != "nnz_gbi"}
        twin.close()
    print(f"\n[harmonic] {name}, {engine}: {info}")
    H.close()
    ctx.close()


# ---- the extension through the public entry point ------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", hc.NAMES)
def test_extend(ddm, name, engine, monkeypatch):
    """ddm_harmonic_extend at every width and leading dimension of the table: interior rows (NaN before) within tolerance, every other
    row and the padding columns bit-equal to their input"""
    c, ctx, H = _open(ddm, name, engine, monkeypatch)
    worst, kernels = 0.0, set()
    for nrhs in hc.EXTEND_WIDTHS:
        ref = c.extend_ref(nrhs)
        for ldx in hc.extend_lds(nrhs):
            S, cols = _slot_block(c, c.X, nrhs, ldx, 0, nan_rows=(c.ii,))
            Sd = _dev(S)
            H.extend(Sd[:, cols])
            ctx.sync()
            got = Sd.cpu().numpy()
            _rest_untouched(got, S, c.ii, cols, (name, nrhs, ldx))
            assert np.isfinite(got[c.ii, cols]).all(), (name, nrhs, ldx, "NaN left in or carried into the interior rows")
            ratio = hc.column_ratio(got[c.ii, cols], ref)
            assert ratio.max() <= 1.0, (name, engine, nrhs, ldx, ratio.max(), int(ratio.argmax()))
            if len(c.bb) == 0:
                assert np.all(got[c.ii, cols] == 0.0)
            worst = max(worst, float(ratio.max()))
            kernels.update(k for _, _, k in hc.Shapes.extend_calls(nrhs, ldx))
    assert kernels == {"k_spmm_rowmajor", "k_spmm_rowmajor4"}
    print(f"\n[harmonic] extend {name}, {engine}: largest error / tolerance {worst:.3e}")
    H.close()
    ctx.close()


# ---- P, P^T, T T^T at the eigensolver's strides --------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", hc.NAMES)
def test_projection(ddm, name, engine, monkeypatch):
    """P X = keep_b .* X - A^^-1 G_ib X: interior rows (NaN before) within tolerance, boundary rows bit-equal, neither rows (NaN
    before) 0.0; m = 52 is not chunked (two panels on the device engine)"""
    c, ctx, H = _open(ddm, name, engine, monkeypatch)
    worst = 0.0
    out_rows = np.concatenate([c.ii, c.nn])
    for m in hc.PROJ_WIDTHS:
        ref = c.extend_ref(m)
        for ld, slot in hc.proj_layouts(m):
            S, cols = _slot_block(c, c.X, m, ld, slot, nan_rows=(c.ii, c.nn))
            Sd = _dev(S)
            H.debug_apply(1, Sd[:, cols])
            ctx.sync()
            got = Sd.cpu().numpy()
            _rest_untouched(got, S, out_rows, cols, (name, m, ld, slot))
            assert np.all(got[c.nn, cols] == 0.0), (name, m, ld, slot, "rows that are neither interior nor boundary must be zeroed")
            ratio = hc.column_ratio(got[c.ii, cols], ref)
            assert ratio.max() <= 1.0, (name, engine, m, ld, slot, ratio.max())
            worst = max(worst, float(ratio.max()))
    print(f"\n[harmonic] P {name}, {engine}: largest error / tolerance {worst:.3e}")
    H.close()
    ctx.close()


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", hc.SYMMETRIC)
def test_projection_transposed(ddm, name, engine, monkeypatch):
    """P^T R = keep_b .* R - G_bi A^^-1 (interior .* R): interior and neither rows 0.0, boundary rows within tolerance of the definition
    with A_ii^-T"""
    c, ctx, H = _open(ddm, name, engine, monkeypatch)
    worst = 0.0
    allrows = np.arange(c.n)
    for m in hc.PROJ_WIDTHS:
        ref = c.Pt_ref(m)
        for ld, slot in hc.proj_layouts(m):
            S, cols = _slot_block(c, c.R, m, ld, slot)
            Sd = _dev(S)
            H.debug_apply(2, Sd[:, cols])
            ctx.sync()
            got = Sd.cpu().numpy()
            _rest_untouched(got, S, allrows, cols, (name, m, ld, slot))
            assert np.all(got[c.ii, cols] == 0.0) and np.all(got[c.nn, cols] == 0.0), (name, m, ld, slot)
            ratio = hc.column_ratio(got[c.bb, cols], ref[c.bb])
            assert ratio.max() <= 1.0, (name, engine, m, ld, slot, ratio.max())
            worst = max(worst, float(ratio.max()))
    print(f"\n[harmonic] P^T {name}, {engine}: largest error / tolerance {worst:.3e}")
    H.close()
    ctx.close()


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", hc.SYMMETRIC)
def test_t_tt_operator(ddm, name, engine, monkeypatch):
    """Y = T T^T X as ddm_svd_basis applies it (X and Y slots of two arrays): within tolerance of the dense product on the interior
    rows, 0.0 outside, X unchanged"""
    c, ctx, H = _open(ddm, name, engine, monkeypatch)
    worst = 0.0
    interior = c.cls == hc.INTERIOR
    for m in hc.PROJ_WIDTHS:
        ref = c.TTt_ref(m)
        for ld, slot in hc.proj_layouts(m):
            S, cols = _slot_block(c, c.R, m, ld, slot)
            Y0 = np.full((c.n, ld), SENTINEL)
            Y0[:, cols] = NAN
            Sd, Yd = _dev(S), _dev(Y0)
            H.debug_apply(3, Sd[:, cols], pou_int=c.d, Y=Yd[:, cols])
            got = Yd.cpu().numpy()
            _rest_untouched(got, Y0, np.arange(c.n), cols, (name, m, ld, slot))
            assert np.array_equal(_bits(Sd.cpu().numpy()), _bits(S)), "X changed"
            assert np.all(got[~interior, cols] == 0.0), (name, m, ld, slot)
            ratio = hc.column_ratio(got[c.ii, cols], ref[c.ii])
            assert ratio.max() <= 1.0, (name, engine, m, ld, slot, ratio.max())
            worst = max(worst, float(ratio.max()))
    print(f"\n[harmonic] T T^T {name}, {engine}: largest error / tolerance {worst:.3e}")
    H.close()
    ctx.close()


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", hc.SYMMETRIC)
def test_adjoint(ddm, name, engine, monkeypatch):
    """<P X, R> = <X, P^T R> column by column, both sides formed on the host in longdouble from device outputs, within 1e-10 of
    sum |P X| |R| + sum |X| |P^T R|.  X has finite values in every row here: P reads its boundary rows only."""
    c, ctx, H = _open(ddm, name, engine, monkeypatch)
    m = 12
    X, R = c.X[:, :m], c.R[:, :m]
    PXd, PtRd = _dev(X), _dev(R)
    H.debug_apply(1, PXd)
    H.debug_apply(2, PtRd)
    ctx.sync()
    PX, PtR = PXd.cpu().numpy().astype(hc.LD), PtRd.cpu().numpy().astype(hc.LD)
    Xl, Rl = X.astype(hc.LD), R.astype(hc.LD)
    lhs, rhs = (PX * Rl).sum(axis=0), (Xl * PtR).sum(axis=0)
    bound = 1e-10 * ((np.abs(PX) * np.abs(Rl)).sum(axis=0) + (np.abs(Xl) * np.abs(PtR)).sum(axis=0))
    gap = np.abs(lhs - rhs)
    print(f"\n[harmonic] adjoint {name}, {engine}: largest |<PX,R> - <X,P^T R>| / bound {float(np.max(np.where(gap == 0, 0, gap / np.where(bound > 0, bound, 1)))):.3e}")
    assert np.all(gap <= bound), (name, engine, gap, bound)
    H.close()
    ctx.close()


# ---- repetition: the captured multi-solve graph and the regrowth of the work blocks --------------------------------------------------
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", ("poisson-shell", "dominant_gen-random", "uneven9-blocks"))
def test_repetition(ddm, name, engine, monkeypatch):
    """every operation twice on the same buffers (the second solve replays the captured graph) and once more after a call with a wider
    block (reserve_cols allocates t1 and t2 afresh: nothing captured before may be replayed): equal bits with the first run"""
    c, ctx, H = _open(ddm, name, engine, monkeypatch)
    m, wide = 12, 52
    ops = (0, 1, 2) if c.spec.symmetric else (0, 1)
    src = {0: c.X, 1: c.X, 2: c.R}
    buf, first = {}, {}
    for op in ops:
        buf[op] = _dev(src[op][:, :m])
        H.debug_apply(op, buf[op])
        ctx.sync()
        first[op] = buf[op].cpu().numpy()
        assert np.isfinite(first[op]).all()
    assert H.info()["work_cols"] == m
    for round_ in ("replay", "after regrowth"):
        for op in ops:
            buf[op].copy_(_dev(src[op][:, :m]))
            H.debug_apply(op, buf[op])
            ctx.sync()
            assert np.array_equal(_bits(buf[op].cpu().numpy()), _bits(first[op])), (name, engine, op, round_)
        if round_ == "replay":
            W = _dev(c.X[:, :wide])
            H.debug_apply(1, W)
            ctx.sync()
            assert H.info()["work_cols"] == wide
            assert hc.column_ratio(W.cpu().numpy()[c.ii], c.extend_ref(wide)).max() <= 1.0
    H.close()
    ctx.close()


# ---- refusals and errors -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ENGINES)
def test_refusals_and_errors(ddm, engine, monkeypatch):
    from dune_ddm_amd import coarse_spaces as cs
    for name in hc.GENERAL:
        c, ctx, H = _open(ddm, name, engine, monkeypatch)
        Rd, Yd = _dev(c.R[:, :4]), _dev(c.R[:, :4])
        for op in (2, 3):
            with pytest.raises(ddm.DdmError) as e:
                H.debug_apply(op, Rd, pou_int=c.d, Y=Yd)
            assert e.value.code == ddm.DDM_ENOTIMPL, (name, op)
        assert np.array_equal(Rd.cpu().numpy(), c.R[:, :4])
        H.close()
        ctx.close()
    c, ctx, H = _open(ddm, "poisson-shell", engine, monkeypatch, transpose=False)
    assert H.info()["nnz_gbi"] == -1
    Rd, Yd = _dev(c.R[:, :4]), _dev(c.R[:, :4])
    for op in (2, 3):
        with pytest.raises(ddm.DdmError) as e:
            H.debug_apply(op, Rd, pou_int=c.d, Y=Yd)
        assert e.value.code == ddm.DDM_EINVAL
    H.close()
    A, bp, cls, row = hc.error_case()
    with pytest.raises(ddm.DdmError) as e:
        ddm.HarmonicExtension.from_classes(ctx, ddm.CsrMatrix(ctx, A), cls, bp)
    assert e.value.code == ddm.DDM_ENUMERIC and f"interior row {row} " in str(e.value)
    # the builders still refuse an interior block that is not symmetric
    c = hc.case("nearly_sym_hi-shell")
    pou, dm, bm = np.ones(c.n), (c.cls == hc.NEITHER).astype(np.uint8), (c.cls == hc.BOUNDARY).astype(np.uint8)
    par = cs._params(ctx, 2, 1e-5, 1e-3, 5, 4, 0, -0.5, None, "auto", None, False, False)
    with pytest.raises(ddm.DdmError) as e:
        cs._run_eig(ctx, "msgfem", (c.A, c.A), c.block_ptr, pou, dm, bm, par, list(range(len(c.block_ptr) - 1)), False)
    assert e.value.code == ddm.DDM_ENOTIMPL
    dA = ddm.CsrMatrix(ctx, c.A)
    basis, sv, info = np.empty((2, c.n)), np.zeros((len(c.block_ptr) - 1, 2)), ddm.GeneoInfo()
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = ctx.lib.ddm_svd_basis(ctx.h, dA.h, len(c.block_ptr) - 1, hp(c.block_ptr), hp(pou), hp(dm), hp(bm), 2, 0, 1e-8, 5, hp(basis), hp(sv), ctypes.byref(info))
    assert rc == ddm.DDM_ENOTIMPL
    ctx.close()
