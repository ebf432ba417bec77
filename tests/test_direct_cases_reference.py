"""CPU (-m "not gpu"): the cases of tests/direct_cases.py reach the branches of the host direct factor's device solves they exist
for, and a float64 restatement of those solves meets the residual bound tests/test_gpu_direct_host_shapes.py asserts of the device.

Per case: every PRECONDITIONS predicate holds on `schedule_table` (without this a case can silently stop reaching its branch), at
most 10 000 rows, and direct_cases.sweeps -- gather with perm, sequential row sums over the transformed rows with the inverted blocks,
scatter -- of a standard-normal d satisfies Residual.ratio <= C = 2 (w_L + w_U + 9) (derivation: the module docstring of
direct_cases).  The same restatement broken in three ways -- the last operand of the widest row dropped, one unknown read stale (a
virtual one where the case has any), one dinv factor skipped -- exceeds C by a factor of 10^3 at least, so the device check can fail.

Measured (x86-64, 80-bit long double; d standard normal, seed 17): the restatement's ratio against C, and the smallest of the three
broken ratios over C (the dropped operand everywhere but dg_rows, where it is the stale unknown):

  case        n     blocks  entries  min_sn  supernodes  levels L+U  block path  w_L   w_U  ratio  C     broken / C
  sn8         9240  8       1975210  8       365         34+34       no          605   343  5.61   1914  2.6e9
  rows8       9240  8       1975210  10^6    0           463+463     yes         605   343  4.73   1914  2.7e10
  uneven5     2826  5       409744   10^6    0           340+340     yes         510   259  3.12   1556  2.6e10
  uneven5_sn  2826  5       409744   8       129         33+33       no          510   259  3.11   1556  7.0e4
  three       8160  3       2324602  10^6    0           738+738     no          1153  509  5.48   3342  2.4e9
  one         1716  1       474720   10^6    0           611+611     no          748   439  4.64   2392  9.8e10
  pairs       9240  8       1975210  2       631         22+22       no          605   343  5.60   1914  2.6e9
  dg          3504  4       256360   8       193         22+22       no          287   107  2.71   806   3.3e8
  dg_rows     9508  4       866432   10^6    0           308+308     yes         451   167  3.78   1254  1.2e7

Per-block schedules of the block path: rows8 926 -> 6424 levels in all (every block its own run), uneven5 680 -> 1636,
dg_rows 616 -> 2384.  On the
supernode rows the term 2 h / C is 0.13 g in the median and 2.5 g at most (uneven5_sn): the bound stays the plain one in size.
"""
import numpy as np
import pytest

from tests import direct_cases as dc


def test_schedule_table_on_a_hand_made_factor():
    """6 rows in two blocks [0, 4) and [4, 6).  Block 0: a dense run of 4 rows; block 1: a
    2-row run.  Supernode runs, transformed rows, levels and the per-block numbering by hand."""
    A = np.array([[4., 1, 1, 1, 0, 0],
                  [1, 4, 1, 1, 0, 0],
                  [1, 1, 4, 1, 0, 0],
                  [1, 1, 1, 4, 0, 0],
                  [0, 0, 0, 0, 4, 1],
                  [0, 0, 0, 0, 1, 4]])
    n = 6
    L, U = np.eye(n), A.copy()
    for k in range(n):                                           # dense L U without pivoting
        for i in range(k + 1, n):
            L[i, k] = U[i, k] / U[k, k]
            U[i, :] -= L[i, k] * U[k, :]
    import scipy.sparse as sp
    P = sp.csr_matrix((A != 0).astype(float))
    P.sort_indices()
    lu = np.array([L[i, j] if j < i else (1.0 / U[i, i] if i == j else U[i, j]) for i in range(n) for j in P.indices[P.indptr[i]:P.indptr[i + 1]]])
    f = {"perm": np.arange(n), "rowptr": P.indptr, "col": P.indices, "lu": lu}
    bp = [0, 4, 6]
    F = dc.Factor(f, bp)
    assert (F.wL, F.wU) == (3, 3)
    assert dc.supernode_runs(F, 2) == [(0, 4), (4, 6)] and dc.supernode_runs(F, 3) == [(0, 4)] and dc.supernode_runs(F, 5) == []
    # no supernodes: 4 + 2 chained rows, 4 global levels; per block 4 + 2
    T = dc.schedule_table(f, bp, 5)
    assert T.nlev == (4, 4) and list(T.L.m) == [2, 2, 1, 1] and list(T.L.entries) == [0, 2, 2, 3] and T.nvirt == 0
    Tb = dc.schedule_table(f, bp, 5, per_block=True)
    assert list(Tb.L.blk_lev_ptr) == [0, 4, 6] and list(Tb.L.m) == [1, 1, 1, 1, 1, 1] and list(Tb.U.entries) == [0, 1, 2, 3, 0, 1]
    assert not dc.block_path(T)
    # min 3: run (0, 4) transformed.  L: 4 phase-1 rows without entries (level 0), 4 phase-2 rows of 1..4 entries (level 1); rows 4, 5 plain
    T = dc.schedule_table(f, bp, 3)
    assert T.nvirt == 4 and T.nlev == (2, 2)
    assert list(T.L.dst) == [6, 7, 8, 9, 0, 1, 2, 3, 4, 5] and list(T.L.rhs) == [0, 1, 2, 3, -1, -1, -1, -1, 4, 5]
    assert list(T.L.len) == [0, 0, 0, 0, 1, 2, 3, 4, 0, 1] and list(T.L.m) == [5, 5] and list(T.L.entries) == [0, 11]
    assert list(T.U.dst) == [5, 4, 9, 8, 7, 6, 3, 2, 1, 0] and list(T.U.len) == [0, 1, 0, 0, 0, 0, 1, 2, 3, 4]
    assert list(T.L.S) == [1, 1] and T.L.plan == [(0, 2, True)]
    # the sweeps solve the system, with and without the transformation
    d = np.arange(1.0, 7.0)
    for ms in (2, 3, 5):
        x = dc.sweeps(dc.schedule_table(f, bp, ms), d)
        assert np.allclose(A @ x, d, rtol=0, atol=1e-14)


@pytest.mark.parametrize("nrhs", [1, 255, 256, 257, 260, 512, 513])
def test_panels_cover_every_column_once(nrhs):
    """the column panels of enqueue_csr_direct: at most 256 wide (k_trsv_csr_level_multi needs Sm nrhs <= 256 threads per row: rows
    per workgroup >= 1), every column in exactly one"""
    ps = dc.panels(nrhs)
    hit = np.zeros(nrhs, dtype=int)
    for c0, w in ps:
        assert 1 <= w <= dc.PANEL
        hit[c0:c0 + w] += 1
        for S in (1, 2, 4, 8, 16, 32, 64):
            Sm, rpb = dc.multi_threads_per_row(S, w)
            assert rpb >= 1 and Sm * w * rpb <= dc.WG
    assert (hit == 1).all() and len(ps) == -(-nrhs // dc.PANEL)


def test_block_sweep_widths_reach_the_thread_layouts():
    """Sm nrhs of k_trsv_csr_level_multi for a level of S = 64 at the widths the GPU test runs"""
    got = [dc.multi_threads_per_row(64, m) for m in (1, 2, 3, 5, 24, 48, 128, 129, 256)]
    assert [s * m for (s, _), m in zip(got, (1, 2, 3, 5, 24, 48, 128, 129, 256))] == [64, 128, 192, 160, 192, 192, 256, 129, 256]
    assert [r for _, r in got] == [4, 2, 1, 1, 1, 1, 1, 1, 1]


@pytest.mark.parametrize("name", dc.NAMES)
def test_case_reaches_its_branches_and_the_restatement_meets_the_bound(name):
    c = dc.case(name)
    print(f"\n{name}: n = {c.n}, {len(c.block_ptr) - 1} block(s), factor entries = {len(c.F.ci)}, min_sn = {c.min_sn}, general = {c.general}, "
          f"w_L = {c.F.wL}, w_U = {c.F.wU}, levels {c.table.nlev}, block path: {c.blocks}, C = {c.C}")
    for line in c.table.summary() + (c.btable.summary() if c.blocks else []):
        print("  " + line)
    assert c.n <= dc.MAX_N and np.isfinite(c.F.lu).all()
    failed = [what for what, holds in dc.PRECONDITIONS[name] if not holds(c)]
    assert not failed, failed
    d = np.random.default_rng(17).standard_normal(c.n)
    x = dc.sweeps(c.table, d)
    ratio = c.res.ratio(d, x, c.C)
    xs = c.M @ x
    print(f"  restatement: residual ratio {ratio:.2f} (C = {c.C}); |A x - d| / |d| = {np.max(np.abs(xs - d)) / np.max(np.abs(d)):.1e}")
    assert ratio <= c.C
    assert np.max(np.abs(xs - d)) <= 1e-9 * np.max(np.abs(d))    # the factor is the matrix's: x solves the system itself
    if c.blocks:                                                 # the per-block order of rows is another valid substitution order
        assert c.res.ratio(d, dc.sweeps(c.btable, d), c.C) <= c.C
    how, where = dc.breakages(c.table, d)
    for what, switch in how.items():
        rb = c.res.ratio(d, dc.sweeps(c.table, d, **switch), c.C)
        print(f"  {what}, {where[what]}: ratio {rb:.2e} = {rb / c.C:.1e} C")
        assert rb >= 1e3 * c.C, (what, rb, c.C)
