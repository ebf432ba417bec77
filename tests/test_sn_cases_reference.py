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

The refined solution (corrections from long double residuals) leaves max_i |d - A x|_i / (|A| |x| + |d|)_i = 0.45 .. 0.71 u: it is the
exact solution rounded to double.  The reference stays a factor 600 .. 2400 below the bound, as worst-case bounds with C of the
order of the row width do; the mutants stand 10^6 and more above it.
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
}


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


@pytest.mark.parametrize("name", [n for n in sc.NAMES if sc._CASES[n][1]])
def test_lu_cases_are_column_dominant(name):
    c = sc.case(name)
    dom = sc.column_dominance(c.M)
    print(f"{name}: min_j (|a_jj| - sum_i |a_ij|) / |a_jj| = {dom:.3g}")
    assert dom > 0
    # no row exchange in the reference: every pivot is the largest entry of its column of its diagonal block
    for s in range(c.S.nsn):
        Ld = c.ref.Ld[s]
        assert np.abs(np.tril(Ld, -1)).max(initial=0.0) < 1.0


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
    for kind, where, xm in sc.mutants(c):
        rm = min(c.evaluate(c.d, xm, route).ratio() for route in (None, "default"))
        print(f"  {kind}, {where}: ratio {rm:.2e}")
        assert rm >= 1e3, (kind, rm)
    # two intact solutions differ within their bounds; a mutant does not
    e, er = c.evaluate(c.d, x), c.evaluate(c.d, xr)
    assert e.difference(er) <= 1.0
    assert c.evaluate(c.d, xm).difference(e) >= 1e3
