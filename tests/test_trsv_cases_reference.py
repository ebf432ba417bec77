"""CPU (-m "not gpu"): the cases of tests/trsv_cases.py reach the kernel branches they exist for, and the oracle's ILU(0) solve
meets the residual bound that tests/test_gpu_trsv_shapes.py asserts of the device.

Per case: every PRECONDITIONS predicate holds on `level_table` (without this a case can silently stop reaching its branch), the
caps n <= 20 000 and sum m w <= 4 10^6 hold, the oracle (oracle/kernels.c: sequential, column order, -ffp-contract=off) factors
the matrix without a zero pivot, and its solve of a standard-normal d satisfies

    residual_ratio(M, lu, d, x, 2^-53) <= C = 2 (w_L + w_U + 3),

w_L / w_U the widest lower / upper row (derivation: trsv_cases.bound).  A dropped or stale operand gives a ratio of 10^9 or more.

Measured (x86-64, 80-bit longdouble; d standard normal, seed 17), the oracle's ratio against C:

  case        n      blocks  nnz     w_L  w_U   sum m w  ratio  C
  band17      12700  1       301700  17   17    289272   5.58   74
  layers      10704  1       28320   2    4200  19376    1.85   8410
  wide        682    1       8442    40   300   9322     6.70   686
  chain600    600    1       1798    1    1     1198     1.66   10
  elasticity  3150   4       108486  37   41    179002   0.92   162
  dg          3504   4       66240   11   19    70544    3.50   66
  blocks3     2029   3       12185   3    21    10259    2.83   54
  blocks9     3939   9       52269   40   80    53011    5.04   246
  blocks17    7877   17      104537  40   80    106022   5.40   246

elasticity: blocks of 735, 840, 840, 735 rows with 57, 57, 57, 44 levels per triangle, 32..50 of them with w > 16 and 10..22 in the
few-wide-rows branch of the level kernel; dg: 104, 108, 108, 96 levels per triangle, one upper row of 19 entries.
"""
import numpy as np
import pytest

from tests import trsv_cases as tc

U64 = 2.0 ** -53


def test_level_table_on_a_hand_made_matrix():
    """5 rows: L pattern 1<-0, 2<-0, 3<-{1,2}, 4 alone; U the transpose.  Levels and widths by hand."""
    import scipy.sparse as sp
    Lp = sp.csr_matrix((np.ones(4), ([1, 2, 3, 3], [0, 0, 1, 2])), shape=(5, 5))
    M = tc.randomise(Lp + Lp.T, 0)
    t = tc.level_table(M, [0, 5])
    L, U = t.blocks[0]
    assert list(L.level) == [0, 1, 1, 2, 0] and list(L.m) == [2, 2, 1] and list(L.w) == [0, 1, 2]
    assert list(U.level) == [2, 1, 1, 0, 0] and list(U.m) == [2, 2, 1] and list(U.w) == [0, 1, 2]
    assert t.entries == 2 * (2 * 0 + 2 * 1 + 1 * 2) and t.wL == 2 and t.wU == 2
    # as two blocks [0, 4) and [4, 5): the single row is a block of its own
    t2 = tc.level_table(M, [0, 4, 5])
    assert [b[0].nlev for b in t2.blocks] == [3, 1] and list(t2.blocks[1][1].m) == [1]
    # strictly dominant diagonal, independent values on the two sides
    A = M.toarray()
    off = np.abs(A).sum(axis=1) - np.abs(np.diag(A))
    assert np.allclose(np.diag(A), 1.0 + off) and A[1, 0] != A[0, 1]


def test_residual_ratio_sees_one_dropped_operand():
    """the exact solve of a small dense-ish factor has a ratio of a few units; one entry of x off by 1e-6 relative has 10^9"""
    c = tc.case("wide")
    d = np.random.default_rng(3).standard_normal(c.n)
    lu, x = tc.oracle_factor_and_solve(c, d)
    good = tc.residual_ratio(c.M, lu, d, x, U64)
    xb = x.copy()
    xb[c.n // 2] *= 1.0 + 1e-6
    bad = tc.residual_ratio(c.M, lu, d, xb, U64)
    print(f"\nratio {good:.2f}; with one entry off by 1e-6: {bad:.2e}")
    assert good <= c.C and bad > 1e6 * c.C


@pytest.mark.parametrize("name", tc.NAMES)
def test_case_reaches_its_branches_and_the_oracle_meets_the_bound(ddm, name):
    c = tc.case(name)
    print(f"\n{name}: n = {c.n}, {len(c.block_ptr) - 1} block(s), nnz = {c.M.nnz}, w_L = {c.table.wL}, w_U = {c.table.wU}, sum m w = {c.table.entries}, C = {c.C}")
    shown = c.table.summary()
    for line in shown[:6] + (["  ..."] if len(shown) > 6 else []):
        print("  " + line)
    assert c.M.has_sorted_indices and c.M.shape == (c.n, c.n) and c.block_ptr[0] == 0 and c.block_ptr[-1] == c.n
    assert c.n <= tc.MAX_N and c.table.entries <= tc.MAX_ELL and c.whole.entries <= tc.MAX_ELL
    failed = [what for what, holds in tc.PRECONDITIONS[name] if not holds(c)]
    assert not failed, failed
    d = np.random.default_rng(17).standard_normal(c.n)
    lu, x = tc.oracle_factor_and_solve(c, d)                    # raises on a zero pivot
    assert np.isfinite(lu).all() and np.isfinite(x).all()
    ratio = tc.residual_ratio(c.M, lu, d, x, U64)
    print(f"  oracle residual ratio {ratio:.2f} (C = {c.C})")
    assert ratio <= c.C
