"""-m gpu: the block (ddm_*_multi) and the coarse applies at the shapes their kernels branch on, against the CPU oracle column by column.

The other block tests run one tiny shape (subdomains below 2000 rows, m in {1, 3, 8} for the applies, the same number of coarse vectors
on every subdomain, at most 4 of them).  Here:

  * a large grid, (44, 42, 40) on 2 x 2 x 2 with overlap 2: every subdomain has more than one 8192-row chunk with a ragged last one
    (the chunk sums of k_coarse_restrict_final_multi / k_coarse_reduce), and n * m exceeds one pass of the element-wise grids for
    m >= 8 (the grid-stride loops of k_extend_multi, k_restrict_multi, k_scale_add_multi, k_pack_multi, k_unpack_multi, ...);
  * a hand-made coarse basis with (1, 2, 4, 5, 7, 9, 12, 3) vectors per subdomain: kmax = 12 (three passes of the j += 4 loop of the
    restriction), coarse_index < 0 slots in seven subdomains, K = 43 (k_dense_mm over several workgroups).  (In the prolongation an
    unused slot multiplies a basis row that include/ddm_hip.h requires to be zero, so whatever coefficient the kernel takes for it
    cannot change a finite result: that branch is exercised here but no test can tell its two sides apart.)
  * every block width 1..32 on the small grid (13, 12, 11): R = 64 / m with idle lanes, R = 2, the four-rows-in-flight loop with its
    ragged tail, the quad SpMM / level kernels for m = 4, 8, ..., 32 and the scalar ones otherwise, every 8/4/2/1 split of the
    column groups of the reductions, MULTI_MAX itself.

The reference is the float64 CPU oracle applied to each column (an independent implementation), under the project's rules as they
stand in tests/test_gpu_parity.py: RTOL_VEC = 1e-12 of the column's largest entry for an operator application, 1e-10 for a
preconditioner apply.  tests/test_apply_shapes_reference.py shows on the CPU that the oracle is more than four times closer than that
to the extended-precision value on exactly these inputs.  In addition every block column is compared with the single-vector device
entry point under RTOL_APPLY = 1e-13 (tests/test_gpu_multi_rhs.py); `dot_multi` is compared with `==`.  No case is skipped or
filtered at run time."""
import numpy as np
import pytest

from tests.test_apply_shapes_reference import LARGE, RTOL_PREC, SMALL, build_case, check_sizes, consistent_columns, split_novlp
from tests.test_gpu_multi_gmres import ATOL_HIST as GMRES_ATOL_HIST
from tests.test_gpu_multi_gmres import RTOL_HIST as GMRES_RTOL_HIST
from tests.test_gpu_multi_rhs import RTOL_APPLY
from tests.test_gpu_parity import ATOL_HIST, RTOL_HIST, RTOL_VEC

pytestmark = pytest.mark.gpu

MULTI_MAX = 32
WIDTHS = {"small": tuple(range(1, MULTI_MAX + 1)),
          # R = 64 / m = 12, 3, 2 with idle lanes (5, 21, 22, 31); R m = 64 exactly (1, 8, 32); the quad kernels (8, 12, 32); the maximum
          "large": (1, 5, 8, 12, 21, 22, 31, 32)}
CONFIGS = [("standard", "additive"), ("restricted", "additive"), ("standard", "multiplicative"), ("restricted", "multiplicative")]
OPS = ("apply", "applyscaleadd", "schwarz", "galerkin", "prec")
RULE = {"apply": RTOL_VEC, "applyscaleadd": RTOL_VEC, "schwarz": RTOL_PREC, "galerkin": RTOL_PREC, "prec": RTOL_PREC}


class Case:
    """One grid: the decomposition, the uneven basis, 32 fixed input columns and (computed once per configuration) the oracle's
    applies on them.  A block of width m is made of the first m columns."""

    def __init__(self, ddm, name):
        self.name = name
        self.dec, self.basis = build_case(ddm, LARGE if name == "large" else SMALL)
        self.n_o, self.n, self.rows = check_sizes(self.dec, self.basis, large=name == "large")
        print(f"\n{name} grid: n_o = {self.n_o}, n = {self.n}, rows per subdomain {min(self.rows)}..{max(self.rows)}")
        self.X = consistent_columns(self.dec, MULTI_MAX, seed=11)
        self.Y0 = consistent_columns(self.dec, MULTI_MAX, seed=97)
        self._oracle = {}

    def tl(self, stype, mode, **kw):
        from dune_ddm_amd.solver import TwoLevelSchwarz
        return TwoLevelSchwarz(self.dec, coarse=self.basis, schwarz_type=stype, mode=mode, **kw)

    def _columns(self, fn):
        dec, out = self.dec, []
        for j in range(MULTI_MAX):
            out.append(np.concatenate(fn(split_novlp(dec, self.X[:, j]), split_novlp(dec, self.Y0[:, j]))))
        return np.stack(out, axis=1)

    def oracle(self, stype, mode):
        """{operation: (n_o, 32) array}, "a0": the oracle's coarse matrix"""
        from tests.oracle_bridge import oracle_objects
        key = (stype, mode)
        if key in self._oracle:
            return self._oracle[key]
        dec = self.dec
        op, sp_, prec, sch, gal = oracle_objects(dec, schwarz_type=stype, mode=mode, coarse=self.basis)
        zeros = lambda: [np.zeros(sd.n_o) for sd in dec.subs]   # noqa: E731

        def apply(xs, ys):
            y = zeros()
            op.apply(xs, y)
            return y

        def usmv(xs, ys):
            op.applyscaleadd(-0.5, xs, ys)
            return ys

        def precond(p):
            def fn(xs, ys):
                z = zeros()
                p.apply(z, ys)
                return z
            return fn

        if "shared" not in self._oracle:                        # the operator and the coarse level do not depend on the configuration
            self._oracle["shared"] = {"apply": self._columns(apply), "applyscaleadd": self._columns(usmv), "galerkin": self._columns(precond(gal)),
                                      "a0": gal.a0.toarray()}
        res = dict(self._oracle["shared"])
        skey = ("schwarz", stype)
        if skey not in self._oracle:
            self._oracle[skey] = self._columns(precond(sch))
        res["schwarz"] = self._oracle[skey]
        res["prec"] = self._columns(precond(prec))
        self._oracle[key] = res
        return res


@pytest.fixture(scope="module")
def cases(ddm):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(ddm, name)
        return made[name]
    return get


def _coldev(a, ref):
    """per column: max |a - ref| / max |ref|"""
    return np.max(np.abs(a - ref), axis=0) / np.maximum(np.max(np.abs(ref), axis=0), 1e-300)


def _single_applies(tl, Xd, Yd):
    """the single-vector device entry points on every column: {operation: (n_o, 32) host array}"""
    import torch
    n_o, out = tl.rl.n_o, {k: [] for k in OPS}
    for j in range(Xd.shape[1]):
        x, y0 = Xd[:, j].contiguous(), Yd[:, j].contiguous()
        y = torch.full_like(x, float("nan"))
        tl.op.apply(x, y)
        out["apply"].append(y)
        y = y0.clone()
        tl.op.applyscaleadd(-0.5, x, y)
        out["applyscaleadd"].append(y)
        for key, dev in (("schwarz", tl.schwarz), ("galerkin", tl.galerkin), ("prec", tl.prec)):
            z = torch.full((n_o,), float("nan"), dtype=torch.float64, device=tl.dev)
            dev.apply(z, y0)
            out[key].append(z)
    tl.ctx.sync()
    return {k: torch.stack(v, dim=1).cpu().numpy() for k, v in out.items()}


def _block_applies(tl, X, Y0):
    """the block entry points on an (n_o, m) block; outputs that are overwritten are pre-filled with NaN"""
    import torch
    out = {}
    Y = torch.full_like(X, float("nan"))
    tl.op.apply_multi(X, Y)
    out["apply"] = Y
    Y = Y0.clone()
    tl.op.applyscaleadd_multi(-0.5, X, Y)
    out["applyscaleadd"] = Y
    for key, dev in (("schwarz", tl.schwarz), ("galerkin", tl.galerkin), ("prec", tl.prec)):
        Z = torch.full_like(X, float("nan"))
        dev.apply_multi(Z, Y0)
        out[key] = Z
    tl.ctx.sync()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("stype, mode", CONFIGS)
@pytest.mark.parametrize("grid", ["small", "large"])
def test_block_and_single_applies_match_oracle(ddm, cases, grid, stype, mode):
    """op.apply, op.applyscaleadd, schwarz.apply, galerkin.apply, prec.apply -- the single-vector entry points on 32 columns and the
    block entry points for every width of WIDTHS[grid] on the first m of them: column j against the oracle's apply on column j (project
    rule), the block column against the single-vector result (RTOL_APPLY), dot_multi == dot for every m in 1..32, and the coarse matrix
    assembled on the device against the oracle's."""
    case = cases(grid)
    ora = case.oracle(stype, mode)
    tl = case.tl(stype, mode)
    assert tl.K == 43 and tl.galerkin is not None
    Xd, Yd = tl.to_device(case.X), tl.to_device(case.Y0)

    a0dev = float(np.max(np.abs(tl.a0 - ora["a0"])) / np.max(np.abs(ora["a0"])))
    print(f"\n{grid} {stype} {mode}: a0 deviation {a0dev:.2e}")
    single = _single_applies(tl, Xd, Yd)
    worst = {k: float(_coldev(single[k], ora[k]).max()) for k in OPS}
    print("  single-vector vs oracle:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert a0dev < 1e-12
    for k in OPS:
        assert np.isfinite(single[k]).all(), k
        assert worst[k] < RULE[k], (k, worst[k])

    dots = [tl.op.dot(Xd[:, j].contiguous(), Yd[:, j].contiguous()) for j in range(MULTI_MAX)]
    for m in range(1, MULTI_MAX + 1):                           # every 8/4/2/1 split of the column groups, bit for bit
        d = tl.op.dot_multi(Xd[:, :m].contiguous(), Yd[:, :m].contiguous())
        assert len(d) == m and all(d[j] == dots[j] for j in range(m)), (m, list(d), dots[:m])

    worst_o, worst_s = {k: 0.0 for k in OPS}, {k: 0.0 for k in OPS}
    failures = []
    for m in WIDTHS[grid]:
        blk = _block_applies(tl, Xd[:, :m].contiguous(), Yd[:, :m].contiguous())
        for k in OPS:
            assert blk[k].shape == (case.n_o, m)
            if not np.isfinite(blk[k]).all():                   # an entry that was never written
                failures.append((m, k, "not finite"))
                continue
            eo, es = float(_coldev(blk[k], ora[k][:, :m]).max()), float(_coldev(blk[k], single[k][:, :m]).max())
            worst_o[k], worst_s[k] = max(worst_o[k], eo), max(worst_s[k], es)
            if not eo < RULE[k]:
                failures.append((m, k, "oracle", eo))
            if not es <= RTOL_APPLY:
                failures.append((m, k, "single-vector", es))
    print("  block vs oracle:", {k: f"{v:.2e}" for k, v in worst_o.items()})
    print("  block vs single-vector:", {k: f"{v:.2e}" for k, v in worst_s.items()})
    assert not failures, failures
    tl.prec.check_status()
    tl.ctx.close()


@pytest.mark.parametrize("grid", ["small", "large"])
def test_columns_do_not_depend_on_the_block_width(ddm, cases, grid):
    """Column j of op.apply_multi and of schwarz.apply_multi (standard and restricted) is bit-identical for m = 7 (scalar SpMM and
    level kernels), 8 and 32 (four columns per thread): same sums in the same order, and the halo, extend and restrict kernels only
    move or add entries in list order.  The coarse restriction is exempt -- its partition of the rows over the lanes (R = 64 / m) and
    with it the summation order depends on m -- so galerkin.apply_multi and prec.apply_multi are not part of this test."""
    import torch
    case = cases(grid)
    for stype in ("standard", "restricted"):
        tl = case.tl(stype, "additive")
        Xd, Yd = tl.to_device(case.X), tl.to_device(case.Y0)
        got = {}
        for m in (7, 8, 32):
            X, D = Xd[:, :m].contiguous(), Yd[:, :m].contiguous()
            Y, Z = torch.full_like(X, float("nan")), torch.full_like(X, float("nan"))
            tl.op.apply_multi(X, Y)
            tl.schwarz.apply_multi(Z, D)
            tl.ctx.sync()
            got[m] = (Y.cpu().numpy(), Z.cpu().numpy())
        for m in (8, 32):
            assert np.array_equal(got[m][0][:, :7], got[7][0]), ("op.apply_multi", stype, m)
            assert np.array_equal(got[m][1][:, :7], got[7][1]), ("schwarz.apply_multi", stype, m)
        assert np.array_equal(got[32][0][:, :8], got[8][0]) and np.array_equal(got[32][1][:, :8], got[8][1])
        tl.prec.check_status()
        tl.ctx.close()


def _rhs_columns(case, tl, m):
    """the first m of [b, r1, 2 b, 0, r2, r3, ...]: the block of tests/test_gpu_multi_rhs.py continued with random consistent columns"""
    b0 = np.asarray(tl.rl.b, dtype=np.float64)
    R = consistent_columns(case.dec, MULTI_MAX, seed=5)
    cols = [b0, R[:, 0], 2.0 * b0, np.zeros_like(b0)] + [R[:, j] for j in range(1, MULTI_MAX - 3)]
    return np.stack(cols[:m], axis=1)


SOLVES = {
    # CG needs the symmetric preconditioner; restart 6 gives several restart cycles (configuration b of tests/test_gpu_multi_gmres.py)
    "cg": dict(stype="standard", mode="additive", solver="cgsolver", restart=100, rtol=RTOL_HIST, atol=ATOL_HIST, maxit=300),
    "gmres": dict(stype="restricted", mode="additive", solver="restartedgmressolver", restart=6, rtol=GMRES_RTOL_HIST, atol=GMRES_ATOL_HIST, maxit=200),
}


@pytest.mark.parametrize("key", sorted(SOLVES))
def test_block_solves_at_the_edges_of_m(ddm, cases, key):
    """solve_multi on the small grid with the uneven basis for m = 32 (MULTI_MAX) and m = 15 (column groups 8 + 4 + 2 + 1): every
    column against tl.solve on that column -- same iteration count and converged flag, history and x under the rules of the two block
    test files; column 2 = 2 x column 0 bit for bit; the zero column converges at once and is never touched."""
    cfg = SOLVES[key]
    case = cases("small")
    tl = case.tl(cfg["stype"], cfg["mode"])
    B32 = _rhs_columns(case, tl, MULTI_MAX)
    kw = dict(reduction=1e-10, maxit=cfg["maxit"], solver=cfg["solver"], restart=cfg["restart"])
    singles = {}
    for j in range(MULTI_MAX):
        if j != 3:
            r1, h1, x1 = tl.solve(b=B32[:, j], **kw)
            singles[j] = (r1, np.asarray(h1), x1.cpu().numpy())
    for m in (MULTI_MAX, 15):
        res, hist, X = tl.solve_multi(B32[:, :m], **kw)
        Xh = X.cpu().numpy()
        its = [r.iterations for r in res]
        print(f"\n{key} m = {m}: block iterations {its}")
        assert len(res) == m and hist.shape == (max(its) + 1, m)
        worst_h = worst_x = 0.0
        for j in range(m):
            if j == 3:
                continue
            r1, h1, x1 = singles[j]
            assert res[j].iterations == r1.iterations and res[j].converged == r1.converged == 1, (m, j, res[j].iterations, r1.iterations)
            hj = hist[:res[j].iterations + 1, j]
            worst_h = max(worst_h, float(np.max(np.abs(hj - h1) / h1)))
            worst_x = max(worst_x, float(np.max(np.abs(Xh[:, j] - x1)) / np.max(np.abs(x1))))
            assert (np.abs(hj - h1) <= cfg["rtol"] * h1 + cfg["atol"] * h1[0]).all(), (m, j)
            assert np.isnan(hist[res[j].iterations + 1:, j]).all()
            assert np.max(np.abs(Xh[:, j] - x1)) <= 1e-8 * np.max(np.abs(x1)), (m, j)
            assert res[j].reduction <= 1e-10
        print(f"  worst history deviation / |r_k| {worst_h:.2e}, worst x deviation {worst_x:.2e}")
        assert res[2].iterations == res[0].iterations
        assert np.array_equal(Xh[:, 2], 2.0 * Xh[:, 0]) and np.array_equal(hist[:, 2], 2.0 * hist[:, 0], equal_nan=True)
        assert res[3].iterations == 0 and res[3].converged == 1 and res[3].def0 == 0.0
        assert not np.any(Xh[:, 3]) and hist[0, 3] == 0.0 and np.isnan(hist[1:, 3]).all()
    tl.prec.check_status()
    tl.ctx.close()


def test_block_gmres_on_the_large_grid_matches_oracle(ddm, cases):
    """One block GMRES solve with m = 8 and restart 6 on the large grid (n_o * m beyond one pass of the element-wise grids: the
    grid-stride loops of k_gmres_update_multi, k_scale_into_multi and k_axpy_negdev_multi), column 0 against the oracle's GMRES."""
    from tests.oracle_bridge import oracle_solve
    cfg = SOLVES["gmres"]
    case = cases("large")
    tl = case.tl(cfg["stype"], cfg["mode"])
    res, hist, X = tl.solve_multi(_rhs_columns(case, tl, 8), reduction=1e-10, maxit=cfg["maxit"], solver=cfg["solver"], restart=cfg["restart"])
    it, conv, hist_o, xo = oracle_solve(case.dec, reduction=1e-10, maxit=cfg["maxit"], solver=cfg["solver"], restart=cfg["restart"], coarse=case.basis,
                                        schwarz_type=cfg["stype"], mode=cfg["mode"])
    ho = np.array(hist_o)
    print(f"\nlarge grid block GMRES: iterations {[r.iterations for r in res]}, oracle {it}")
    assert all(r.converged for r in res)
    assert res[0].iterations == it and conv, (res[0].iterations, it)
    h0 = hist[:it + 1, 0]
    print(f"  history deviation / |r_k| {float(np.max(np.abs(h0 - ho) / ho)):.2e}")
    assert (np.abs(h0 - ho) <= cfg["rtol"] * ho + cfg["atol"] * ho[0]).all()
    want = np.concatenate(xo)
    Xh = X.cpu().numpy()
    assert np.max(np.abs(Xh[:, 0] - want)) <= 1e-8 * np.max(np.abs(want))
    assert res[2].iterations == res[0].iterations and np.array_equal(Xh[:, 2], 2.0 * Xh[:, 0])
    assert res[3].iterations == 0 and not np.any(Xh[:, 3])
    tl.prec.check_status()
    tl.ctx.close()
