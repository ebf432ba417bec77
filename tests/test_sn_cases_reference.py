"""CPU (-m "not gpu"): the cases of tests/sn_cases.py reach the kernel routes of the device supernodal solves they exist for, and the
residual criterion tests/test_gpu_sn_routes.py asserts of the device is met by a float64 reference and missed by broken ones.

(i) Coverage.  `Shapes` (a restatement of decide_top_levels, build_chains and the branches of solve_t / factorize / reserve on the
arrays of ddm.sn_symbolic_host) reproduces the launch table of the matrices tests/test_gpu_sn_chol.py uses -- none of which runs
k_sn_fwd1<128>, k_sn_bwd1_diag<128> or k_sn_bwd1_partial as code under test in the default configuration -- and, over the cases and
routes of the GPU test, the union of what runs holds every kernel of sn_solve1.hpp and of the solve part of sn_chol.hpp at both
width templates, the classes of REQUIRED_CLASSES, and the per-case figures of FIGURES.  The test prints, per case and route, the
kernels of every level.

(ii) Sharpness.  Evaluated.ratio (derivation: the module docstring of sn_cases) of the float64 reference solve is below 1; the
same solve with one entry of L dropped, one row of one update skipped in the factorisation, or one pivot not applied exceeds 1 by
a factor of 10^3 at least.  Measured (x86-64, 80-bit long double; seed 5 for the mutants' places, which are drawn among ALL places
where the mutant changes the arithmetic: the dropped entries are as small as 7e-5):

  case     n      blocks  supernodes  levels  w_L   w_U  C      reference  dropped entry  skipped row  pivot not applied  |x - refined| / |x|
  one21    7980   1       244         19      2056  962  10166  4.15e-4    2.4e9          3.1e9        6.5e11             3.0e-17
  many     30176  60      1034        6       422   260  2226   1.58e-3    3.4e9          2.4e10       1.7e12             3.0e-17
  eight17  9240   8       308         8       670   344  3386   1.50e-3    1.7e7          3.5e9        1.1e12             2.1e-17
  twelve   12180  12      430         8       670   344  3386   1.60e-3    7.5e8          2.1e8        1.3e12             3.4e-17
  flat2d   5325   4       258         9       287   87   1340   1.10e-3    1.7e6          5.3e10       1.2e12             4.9e-16
  chain1d  306    4       20          6       79    49   432    1.70e-3    6.2e8          2.3e10       4.8e10             8.2e-15
  lu13     1716   1       62          10      787   440  4046   1.24e-3    4.4e7          5.4e9        9.2e11             3.6e-16
  lu17     9240   8       308         8       670   344  3386   1.33e-3    1.0e11         3.6e10       1.7e12             3.2e-16
  lx13     1716   1       62          10      787   440  4046   1.85e-3    1.4e7          6.7e9        1.0e12             4.6e-16
  lx17     9240   8       308         8       670   344  3386   1.82e-3    3.0e10         2.3e10       1.8e12             4.8e-16
  lx21     7980   1       244         19      2056  962  10166  6.90e-4    2.0e7          1.7e9        4.2e11             2.9e-16

The refined solution (corrections from long double residuals) leaves max_i |d - A x|_i / (|A| |x| + |d|)_i = 0.45 .. 0.71 u: it is the
exact solution rounded to double.  The reference stays a factor 500 .. 2400 below the bound, as worst-case bounds with C of the
order of the row width do; the mutants stand 10^6 and more above it.

(iii) Row exchanges.  lx13, lx17 and lx21 (sn_cases._row_exchanging) are built so that the threshold pivoting inside the diagonal
blocks exchanges designed rows -- pairs and 3-cycles -- and the factor has no growth: with Q the exchanges, Q A is strictly column
dominant, so the argument of sn_cases' module docstring holds for Q A and the bound applies to (Q A) x = Q d unchanged in form
(C keeps its value: an exchange stays inside one supernode, whose columns share one row list and one U panel; g and h are formed
from the pivoted factors and mapped back through the orders).  `Reference` replays k_sn_lu_diag's rule in float64 and the tests
assert, with nothing filtered at run time: Q A is column dominant; the replay exchanges exactly the designed rows; in EVERY
decision |a_kk| / amax is 1 (kept) or at most 1.2e-2 (exchanged; the second candidate at most 0.15 amax), so no rounding of the
device decides otherwise; multipliers at most 0.23, max |U| / max |A| <= 1.0008; two thirds of the supernodes exchange.  Supernodes
with an exchange / without, over the three cases and their routes, per class of the solve: bottom level of the small kernels
200 / 107, of <64> 342 / 171, of <128> 66 / 35; top level run link by link (k_sn_top1) 307 / 153; not the first link of a dense
chain 14 / 6; root 6 / 4; big (T > BWD_SMALL; lx21 only) 6 / 4.  Shapes: 103 supernodes with a 3-cycle, 88 with two groups or
more, 3 with the pair of the first and the last column, 10 of 128 columns with a pair across a multiple of 32, 9 of more than 64
columns with a pair across column 64.  Three mutants of the reference for the consumers of the order (threshold asserted: 1):

  case   exchange of one supernode not applied  inverse order applied (3-cycle)  U panel in unpivoted order
  lx13   2.0e12                                 6.3e11                           2.4e11
  lx17   3.2e11                                 3.3e12                           1.3e11
  lx21   1.3e12                                 3.1e12                           1.1e11

The cases without exchanges keep their bits: the reference with the replay equals the one without it (pivoting=False) array by
array, and lu13 / lu17 keep every diagonal entry at a ratio of exactly 1.
"""
import numpy as np
import pytest

from tests import sn_cases as sc


def _describe(c, route):
    sh = c.shapes[route]
    lines = [f"  {route}: ltop = {sh.ltop}, ntop = {sh.ntop}, bottom levels {sh.levels()}, big at the bottom {sh.big_at_bottom()}, "
             f"chains {len(sh.chains)} (links {sorted(set(k for _, k in sh.chains))}), spread = {int(sh.spread)}"]
    for lev, cnt, mnc, mnr, ks in sc.single_vector_plan(sh, c.general):
        lines.append(f"    level {lev}: {cnt} supernodes, nc <= {mnc}, nr <= {mnr}: {', '.join(ks)}")
    return lines


def _reached(c):
    """(kernels, classes) the GPU test runs on case c: every single-vector route and the block solves"""
    kernels, classes = set(), set()
    for route in c.routes:
        sh = c.shapes[route]
        for _, _, _, _, ks in sc.single_vector_plan(sh, c.general):
            kernels.update(ks)
        S = c.S
        bottom = S.level < sh.lbot
        if sh.lbot:
            classes.add("small kernels on" if sh.small_kernels else "small kernels off")
            if not sh.small_kernels and any(sh.lev_maxnc[l] <= sc.SMALL_NC and sh.lev_maxnr[l] <= sc.SMALL_NR for l in range(sh.lbot)):
                classes.add("a small level through k_sn_fwd1<64>")
            if (sh.big & bottom).any():
                classes.add("big at the bottom")
            if (~sh.big & bottom & (S.nr > 0)).any():
                classes.add("not big at the bottom")
            if ((S.nr == 0) & bottom).any():
                classes.add("nr = 0 at the bottom")
            if ((S.nc == 1) & bottom).any():
                classes.add("nc = 1 at the bottom")
            if ((S.nc == sc.SN_MAX_COLS) & bottom).any():
                classes.add("nc = 128 at the bottom")
        if sh.ntop:
            top = ~bottom
            classes.add("top levels, one group (write-through)" if sh.spread else "top levels, XCD-local")
            if (sh.big & top).any():
                classes.add("big in the top levels")
            if ((S.nr == 0) & top).any():
                classes.add("nr = 0 in the top levels")
            if ((S.nc == 1) & top).any():
                classes.add("nc = 1 in the top levels")
            if ((S.nc == sc.SN_MAX_COLS) & top).any():
                classes.add("nc = 128 in the top levels")
            if sh.chains:
                classes.add("chains of one link" if min(k for _, k in sh.chains) == 1 else "no chain of one link")
                if sh.max_links > 1:
                    classes.add("chains of several links")
            blocks_per_xcd = np.bincount(np.arange(c.nblocks) % 8)
            if blocks_per_xcd.max() >= 2:
                classes.add("XCDs that own two blocks")
            if c.nblocks == 8:
                classes.add("one XCD per block")
    sh = c.shapes["default"]
    kernels.update(sc.block_plan(sh, c.general))
    classes.add("block solves: big" if sh.big.any() else "block solves: no big")
    for w in c.widths:
        classes.add(f"{len(sc.panels(w))} column panel(s)")
        classes.update(f"mpad {sc.mpad(pw)}" for _, pw in sc.panels(w))
        if w == 1:
            classes.add("nrhs = 1 through the block kernels")
    # the factorisation every route starts from
    if len(sh.partial_inverse_block()):
        classes.add("nc > 32 and no multiple of 32")
    if sh.update_tile_rows() > 1:
        classes.add("more than one tile row in the update triangle")
    if sh.tiles_with_several_targets():
        classes.add("a tile with several target supernodes")
    if (c.S.nc == 1).any():
        classes.add("nc = 1")
    if (c.S.nc == sc.SN_MAX_COLS).any():
        classes.add("nc = 128")
    if (c.S.nr == 0).any():
        classes.add("nr = 0")
    return kernels, classes


REQUIRED_CLASSES = (
    "small kernels on", "small kernels off", "a small level through k_sn_fwd1<64>", "big at the bottom", "not big at the bottom", "big in the top levels",
    "block solves: big", "block solves: no big", "nr = 0", "nr = 0 at the bottom", "nr = 0 in the top levels", "nc = 1", "nc = 1 at the bottom", "nc = 1 in the top levels",
    "nc = 128", "nc = 128 at the bottom", "nc = 128 in the top levels", "nc > 32 and no multiple of 32", "more than one tile row in the update triangle",
    "a tile with several target supernodes", "chains of one link", "chains of several links", "top levels, XCD-local", "top levels, one group (write-through)",
    "one XCD per block", "XCDs that own two blocks", "1 column panel(s)", "2 column panel(s)", "3 column panel(s)", "mpad 16", "mpad 32", "mpad 48",
    "nrhs = 1 through the block kernels")

# what each case exists for (the figures of the issue that asked for these tests, measured on the CPU)
FIGURES = {
    "one21": lambda c: (c.n, c.S.nsn, c.S.nlev, int((c.S.nc == 128).sum()), int(((c.S.nc > 64) & (c.S.nc < 128)).sum()), int(c.S.nr.max()), int(c.shapes["default"].big.sum()),
                        int(((c.S.nr == 0) & (c.S.parent < 0)).sum()), c.shapes["default"].ntop, c.shapes["default"].max_links > 1, c.shapes["levels"].levels(),
                        c.shapes["levels"].big_at_bottom()) == (7980, 244, 19, 9, 9, 862, 10, 1, 19, True, {"small": 1, "<64>": 4, "<128>": 14}, 10),
    "many": lambda c: c.shapes["default"].ntop == 0 and c.shapes["default"].levels()["<128>"] >= 1 and c.shapes["default"].levels()["<64>"] >= 1 and
    c.shapes["default"].levels()["small"] >= 1 and int((c.S.parent < 0).sum()) == c.nblocks == 60 and c.n == 30176,
    "eight17": lambda c: (c.nblocks, c.S.nlev, c.shapes["default"].ntop) == (8, 8, 7),
    "twelve": lambda c: c.nblocks == 12 and c.shapes["default"].ntop >= 4,
    "flat2d": lambda c: c.S.nc.max() <= 48 and c.S.nr.max() < 64 and c.shapes["default"].T.max() == 1,
    "chain1d": lambda c: (c.S.nsn, int((c.S.nc == 1).sum()), int(c.S.nr.max()), int((c.S.parent < 0).sum())) == (20, 9, 2, 4) and
    all(any(n % q for n in c.S.nc) for q in (4, 16, 32)),
    "lu13": lambda c: c.general and (c.nblocks, c.S.nsn, c.S.nlev) == (1, 62, 10) and abs(c.M - c.M.T).max() > 1e-3 * abs(c.M).max(),
    "lu17": lambda c: c.general and (c.nblocks, c.S.nsn, c.S.nlev) == (8, 308, 8) and abs(c.M - c.M.T).max() > 1e-3 * abs(c.M).max(),
    "lx13": lambda c: c.general and c.design is not None and _same_structure(c, "lu13"),
    "lx17": lambda c: c.general and c.design is not None and _same_structure(c, "lu17"),
    "lx21": lambda c: c.general and c.design is not None and _same_structure(c, "one21") and int(c.shapes["default"].big.sum()) == 10,
}


def _same_structure(c, other):
    """the supernodes, the tree and (where the other case is an L U case) the stored pattern of `other`"""
    o = sc.case(other)
    same = all(np.array_equal(getattr(c.S, a), getattr(o.S, a)) for a in ("perm", "first", "rows", "rptr", "level", "parent", "block"))
    if o.general:
        A, B = c.M.sorted_indices(), o.M.sorted_indices()
        same = same and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
    return same


def test_shapes_reproduce_the_launch_table_of_the_existing_matrices():
    """the matrices of tests/test_gpu_sn_chol.py in the default configuration: no <128> level, no big supernode at the bottom"""
    for (N, P), (nlev, ntop, bottom, big) in sc.EXISTING.items():
        M, bp = sc._poisson(N, P)
        sh = sc.Shapes(sc.Symbolic(M, bp))
        got = (sh.nlev, sh.ntop, tuple(sh.levels()[k] for k in ("small", "<64>", "<128>")), sh.big_at_bottom())
        print(f"{N} in {P}: levels {got[0]}, top levels {got[1]}, bottom small / <64> / <128> {got[2]}, big at the bottom {got[3]}")
        assert got == (nlev, ntop, bottom, big), (N, P, got)


def test_every_route_class_is_reached():
    kernels, classes = set(), set()
    for name in sc.NAMES:
        c = sc.case(name)
        print(f"\n{name}: n = {c.n}, {c.nblocks} block(s), general = {c.general}, {c.S.nsn} supernodes on {c.S.nlev} levels {list(c.shapes['default'].per_level)}, "
              f"nc {int(c.S.nc.min())}..{int(c.S.nc.max())}, nr <= {int(c.S.nr.max())}, {int((c.S.nc == 1).sum())} of one column, {int((c.S.nc == 128).sum())} of 128, "
              f"{int(c.shapes['default'].big.sum())} big, {int((c.S.nr == 0).sum())} with nr = 0; block widths {c.widths}: {', '.join(sc.block_plan(c.shapes['default'], c.general))}")
        assert FIGURES[name](c), name
        for route in c.routes:
            print("\n".join(_describe(c, route)))
        k, cl = _reached(c)
        kernels |= k
        classes |= cl
    plain = {k.replace("<LU>", "") for k in kernels}
    print("\nkernels reached:", sorted(kernels))
    print("classes reached:", sorted(classes))
    assert not set(sc.SOLVE_KERNELS) - plain, sorted(set(sc.SOLVE_KERNELS) - plain)
    assert not set(REQUIRED_CLASSES) - classes, sorted(set(REQUIRED_CLASSES) - classes)
    # the L U instantiations the L U cases reach
    for k in ("k_sn_fwd1_small<LU>", "k_sn_bwd1_small<LU>", "k_sn_fwd1<64><LU>", "k_sn_fwd1<128><LU>", "k_sn_bwd1_diag<64><LU>", "k_sn_bwd1_diag<128><LU>", "k_sn_top1<LU>",
              "k_sn_top_chain<LU>", "k_chain_scatter<LU>", "k_sn_fwd_diag<LU>", "k_sn_bwd_diag<LU>"):
        assert k in kernels, k


def test_spread_routes_only_where_they_are_a_choice():
    for name in sc.NAMES:
        c = sc.case(name)
        assert ("spread0" in c.routes) == (c.nblocks < 8) == ("spread1" in c.routes)
        assert {"default", "links", "levels", "levels_nosmall"} <= set(c.routes)


@pytest.mark.parametrize("name", [n for n in sc.NAMES if sc._CASES[n][1] and n not in sc.EXCHANGING])
def test_lu_cases_are_column_dominant(name):
    c = sc.case(name)
    dom = sc.column_dominance(c.M)
    print(f"{name}: min_j (|a_jj| - sum_i |a_ij|) / |a_jj| = {dom:.3g}")
    assert dom > 0
    # no row exchange in the reference: every pivot is the largest entry of its column of its diagonal block
    for s in range(c.S.nsn):
        Ld = c.ref.Ld[s]
        assert np.abs(np.tril(Ld, -1)).max(initial=0.0) < 1.0
    # ... and the replay of the device's threshold test says so: every diagonal entry is kept, as the largest candidate
    assert not c.ref.exchanging.any() and np.array_equal(c.ref.src, np.arange(c.n))
    assert all(ratio == 1.0 and not exchanged for dec in c.ref.decisions for ratio, _, exchanged in dec)


@pytest.mark.parametrize("name", ("lu13", "lu17", "chain1d"))
def test_cases_without_exchanges_keep_the_bits_of_the_reference_without_pivoting(name):
    """the reference with the replay of the pivot rule against the one that never looks (pivoting=False, the reference as it was):
    the same factor, the same solve and the same bound, bit for bit (the Cholesky cases never enter the replay: one stands for them)"""
    c = sc.case(name)
    old = sc.Reference(c.M, c.S, c.general, pivoting=False)
    for a in ("Ld", "Ud", "R", "V"):
        assert all(np.array_equal(p, q) for p, q in zip(getattr(c.ref, a), getattr(old, a))), (name, a)
    assert np.array_equal(c.ref.solve(c.D[:, :3]), old.solve(c.D[:, :3])) and np.array_equal(c.ref.solve(c.d), old.solve(c.d))
    for new, was in zip(c.ref.abs_factors(), old.abs_factors()):
        assert (new != was).nnz == 0
    for units in (c.units(None), c.units("default")):
        for new, was in zip(c.ref.unit_blocks(units), old.unit_blocks(units)):
            assert (new != was).nnz == 0


def _exchange_classes(c):
    """class of (iii) -> (supernodes with an exchange, supernodes without) over the routes of case c"""
    S, ex = c.S, c.ref.exchanging
    masks = {k: np.zeros(S.nsn, dtype=bool) for k in EXCHANGE_CLASSES}
    for route in c.routes:
        sh = c.shapes[route]
        for l in range(sh.lbot):
            masks["a bottom level of the small kernels" if sh.kind[l] == "small" else f"a bottom level of {sh.kind[l]}"] |= S.level == l
        plan = [ks for lev, _, _, _, ks in sc.single_vector_plan(sh, c.general) if lev == "top"]
        if plan and "k_sn_top1<LU>" in plan[0]:
            masks["a top level run link by link (k_sn_top1)"] |= S.level >= sh.ltop
        for s0, k in sh.chains:
            assert not sh.chains or "k_sn_top_chain<LU>" in plan[0]
            masks["not the first link of a dense chain (k_sn_top_chain)"][s0 + 1:s0 + k] = True
        masks["big (T > BWD_SMALL)"] |= sh.big
    masks["a root (no rows below)"] |= S.nr == 0
    return {k: (int((m & ex).sum()), int((m & ~ex).sum())) for k, m in masks.items()}


EXCHANGE_CLASSES = ("a bottom level of the small kernels", "a bottom level of <64>", "a bottom level of <128>", "a top level run link by link (k_sn_top1)",
                    "not the first link of a dense chain (k_sn_top_chain)", "a root (no rows below)", "big (T > BWD_SMALL)")


def _exchange_shapes(c):
    """shape of (iv) -> exchanging supernodes of case c that have it"""
    S, out = c.S, {k: set() for k in EXCHANGE_SHAPES}
    for s, g in c.design.groups:
        nc = int(S.nc[s])
        if len(g) == 3:
            out["a 3-cycle"].add(s)
        if len(c.design.of(s)) >= 2:
            out["two groups or more"].add(s)
        if g == (0, nc - 1):
            out["a pair of the first and the last column"].add(s)
        if len(g) == 2 and nc == 128 and g[0] // 32 != g[1] // 32:
            out["128 columns, a pair across a multiple of 32"].add(s)
        if len(g) == 2 and nc > 64 and g[0] < 64 <= g[1]:
            out["more than 64 columns, a pair across column 64"].add(s)
    return {k: len(v) for k, v in out.items()}


EXCHANGE_SHAPES = ("a 3-cycle", "two groups or more", "a pair of the first and the last column", "128 columns, a pair across a multiple of 32",
                   "more than 64 columns, a pair across column 64")


@pytest.mark.parametrize("name", sc.EXCHANGING)
def test_exchanging_cases_exchange_the_designed_rows_and_no_others(name):
    """(i), (ii) and (v) of the module docstring, case by case"""
    import scipy.sparse as sp
    c = sc.case(name)
    S, ref, des = c.S, c.ref, c.design
    Ap = sp.csr_matrix(c.M)[S.perm][:, S.perm]
    dom, dom_a = sc.column_dominance(Ap[des.src]), sc.column_dominance(Ap)
    assert dom > 0 and dom_a < 0                                         # (i): Q A is column dominant (and A is not)
    # (ii) the replay of the device's rule exchanges the designed rows, position by position, with decisions no rounding can turn
    assert np.array_equal(ref.src, des.src)
    assert all(np.array_equal(np.flatnonzero(ref.piv[s] != np.arange(S.nc[s])), sorted(r for g in des.of(s) for r in g)) for s in range(S.nsn))
    dec = [d for per in ref.decisions for d in per]
    assert len(dec) == c.n and int(sum(d[2] for d in dec)) == sum(len(g) - 1 for _, g in des.groups)
    kept, exchanged = [d for d in dec if not d[2]], [d for d in dec if d[2]]
    assert all(not 0.05 <= d[0] <= 0.2 for d in dec)
    assert all(d[0] == 1.0 for d in kept) and max(d[0] for d in exchanged) < 0.05 and max(d[1] for d in exchanged) <= 0.5
    growth = max(np.abs(U).max() for U in ref.Ud) / abs(c.M).max()
    mult = max(max(np.abs(np.tril(L, -1)).max(initial=0.0) for L in ref.Ld), max(np.abs(R).max(initial=0.0) for R in ref.R))
    assert mult < 1.0 and growth <= 1.01                                 # multipliers below 1, no growth: the unpivoted L U of Q A
    several = S.nc >= 2
    share = ref.exchanging[several].sum() / several.sum()
    print(f"\n{name}: {int(ref.exchanging.sum())} of {S.nsn} supernodes exchange rows ({len(des.groups)} groups, {sum(len(g) == 3 for _, g in des.groups)} 3-cycles, "
          f"{len(exchanged)} exchanges); dominance of Q A {dom:.3f}, of A {dom_a:.3g}; |a_kk| / amax <= {max(d[0] for d in exchanged):.2e} where a row is exchanged "
          f"(second candidate <= {max(d[1] for d in exchanged):.3f} amax), 1 elsewhere; largest multiplier {mult:.3f}, max |U| / max |A| = {growth:.4f}")
    assert share >= 1.0 / 3.0                                            # (v)
    for k, (w, wo) in _exchange_classes(c).items():
        print(f"  (iii) {k}: {w} with an exchange, {wo} without")
    for k, cnt in _exchange_shapes(c).items():
        print(f"  (iv) {k}: {cnt}")


def test_exchanges_reach_every_consumer_class():
    """(iii) and (iv): over the exchanging cases and their routes, every class of supernodes holds one that exchanges a row and one
    that does not, and every shape of exchange occurs"""
    classes = {k: np.zeros(2, dtype=np.int64) for k in EXCHANGE_CLASSES}
    shapes = {k: 0 for k in EXCHANGE_SHAPES}
    for name in sc.EXCHANGING:
        c = sc.case(name)
        for k, v in _exchange_classes(c).items():
            classes[k] += v
        for k, v in _exchange_shapes(c).items():
            shapes[k] += v
    print("\n(iii)", {k: tuple(int(x) for x in v) for k, v in classes.items()}, "\n(iv)", shapes)
    assert all(v.min() >= 1 for v in classes.values()), classes
    assert all(v >= 1 for v in shapes.values()), shapes
    for name, other in sc.SAME_PATTERN.items():                          # the refresh test of the GPU suite goes from one to the other
        assert _same_structure(sc.case(name), other)


@pytest.mark.parametrize("name", sc.NAMES)
def test_reference_meets_the_bound_and_mutants_miss_it(name):
    c = sc.case(name)
    x = c.ref.solve(c.d)
    own = max(c.evaluate(c.d, x, route).ratio() for route in (None, "default"))
    xr = c.refined(c.d)
    fwd = np.abs(x - xr).max() / np.abs(xr).max()
    res = float(np.max(np.abs(sc.residual_ld(c.M, c.d, xr)) / (abs(c.M) @ np.abs(xr) + np.abs(c.d)))) / sc.U64
    print(f"\n{name}: n = {c.n}, w_L = {c.wL}, w_U = {c.wU}, C = {c.C}; reference solve: ratio {own:.2e}, |x - refined| / |x| = {fwd:.1e}; "
          f"refined: max_i |d - A x|_i / (|A| |x| + |d|)_i = {res:.2f} u")
    assert own < 1.0
    assert res <= 2.0 and fwd <= 1e-9                                    # the refined solution is the exact one rounded to double
    EX = c.evaluate(c.D[:, :3], c.ref.solve(c.D[:, :3]))                # blocks go through the same code (BLAS sums in another order)
    assert EX.ratio().max() < 1.0 and EX.column(0).difference(c.evaluate(c.d, x)) <= 1.0
    found = sc.mutants(c)
    assert [kind for kind, _, _ in found][3:] == (list(sc.PIVOT_MUTANTS) if name in sc.EXCHANGING else [])
    for kind, where, xm in found:
        rm = min(c.evaluate(c.d, xm, route).ratio() for route in (None, "default"))
        print(f"  {kind}, {where}: ratio {rm:.2e}")
        assert rm > 1.0 if kind in sc.PIVOT_MUTANTS else rm >= 1e3, (kind, rm)
    # two intact solutions differ within their bounds; a mutant does not
    e, er = c.evaluate(c.d, x), c.evaluate(c.d, xr)
    assert e.difference(er) <= 1.0
    assert c.evaluate(c.d, found[2][2]).difference(e) >= 1e3


def test_vanishing_pivot_column_is_repaired_by_the_refinement():
    """lu13 with one column of zeros inside the diagonal block of a leaf supernode (sn_cases.vanishing_column_matrix): the matrix is
    regular, the replay of k_sn_lu_diag's rule meets exactly one vanishing column and gives it the pivot sqrt(eps) max |a_ij|, and
    the refinement rule of include/ddm_hip.h, replayed with the float64 reference on the probe's own right-hand side, ends below
    1e-12 -- the outcome tests/test_gpu_sn_routes.py asserts of the device.  Predicted (x86-64): 2 steps, probe backward errors
    6.28e-09, 1.48e-14, 2.35e-17; cond_2 = 186; the multipliers below the perturbed pivot reach 4.7e6."""
    M, bp, tiny = sc.vanishing_column_matrix()
    c = sc.case("lu13")
    assert M.shape[0] == 1716 and M.nnz == c.M.nnz and np.array_equal(M.indices, c.M.indices), "the zeros are stored: the pattern is lu13's"
    cond = np.linalg.cond(M.toarray())
    ref = sc.Reference(M, c.S, True, tiny=tiny)
    s, j = sc.VANISHING
    vanishing = [(t, k) for t, dec in enumerate(ref.decisions) for k, d in enumerate(dec) if d[0] != d[0]]
    assert vanishing == [(s, j)] and ref.Ud[s][j, j] == tiny
    # the multipliers of 1e6 below the replaced pivot leave the ancestors' blocks without column dominance: the threshold test has real
    # decisions to make there.  With this column it keeps every diagonal entry, and at no ratio that rounding could move across 0.1
    others = [d[0] for dec in ref.decisions for d in dec if d[0] == d[0]]
    assert not ref.exchanging.any() and min(others) > 0.2
    steps, om = sc.predict_refinement(M, ref.solve)
    print(f"\nvanishing column {j} of supernode {s}: cond_2 = {cond:.3g}, tiny = {tiny:.3e}, largest multiplier {max(np.abs(R).max(initial=0.0) for R in ref.R):.3g}; "
          f"predicted refinement: {steps} step(s), probe backward errors {[f'{o:.2e}' for o in om]}")
    assert cond <= 1e6
    assert steps >= 1 and om[0] > 1e-13 and om[steps] <= 1e-12
