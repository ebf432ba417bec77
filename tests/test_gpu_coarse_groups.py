"""-m gpu: the coarse restriction with the defect loaded once per group of COARSE_JG = 10 vectors (k_coarse_restrict_spread; groups of
five per wave in k_coarse_restrict_partial) and the prolongation with two rows per 16-byte load (k_coarse_prolong_spread), through
ddm_galerkin_debug_chain: chunk partials, coarse defect and prolonged correction are torch.equal between the full-grid and the spread
passes, and both equal the arrays under tests/golden/coarse_groups/, which the one-vector-at-a-time kernels before the grouping
produced for the same seeded inputs (both paths changing together would show there)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coarse_groups")
JG = 10
# rows per subdomain: shorter than one trip of 8 x 64 rows; exactly one trip; a full 8192-row chunk and a chunk of one row; a full chunk
# and one of a trip and 37 rows (no multiple of 64).  Subdomains 1 and 2 start at the odd rows 301 and 813, so that their chunks (the
# one-row chunk at 9005 among them) take the prolongation's leading single row; the chunk [813, 9005) also ends in a single row.
SIZES = [301, 512, 8192 + 1, 8192 + 512 + 37]
KMAX = [1, JG - 1, JG, JG + 1, 20, 21]
# one wave for everything; a grid that divides nothing; more waves than work items (6 chunks x 3 groups at the most)
GRIDS = [1, 3, 1024]


def inputs(kmax):
    """seeded: (sub_ptr, basis kmax x n, coarse_index, A0^-1 stand-in K x K, overlapping defect)"""
    rng = np.random.default_rng(1000 + kmax)
    sub_ptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    n = int(sub_ptr[-1])
    # vectors per subdomain: two subdomains have fewer than kmax (zero rows in the basis, coarse_index < 0)
    counts = [kmax, max(1, kmax - 1), kmax, max(1, kmax // 2)]
    basis = np.zeros((kmax, n))
    coarse_index = np.full((len(SIZES), kmax), -1, dtype=np.int64)
    K = 0
    for s, k in enumerate(counts):
        basis[:k, sub_ptr[s]:sub_ptr[s + 1]] = rng.standard_normal((k, SIZES[s]))
        coarse_index[s, :k] = np.arange(K, K + k)
        K += k
    a0inv = rng.standard_normal((K, K)) / K
    # mixed magnitudes and some -0.0: another order of additions changes the sums
    d = rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 8, n)
    d[rng.choice(n, n // 50, replace=False)] = -0.0
    return sub_ptr, basis, coarse_index, a0inv, d


def chain_results(ddm, ctx, kmax, grids):
    """{spread_grid: (partials, d0, x_ovlp)} as numpy arrays.  The chain leaves its results in buffers of the preconditioner that it never
    clears, so before every run they are poisoned: the chain runs on an all-NaN defect through the OTHER pair of kernels (full-grid
    before a spread run and the reverse), which turns every partial and every row of x_ovlp into NaN.  A pass that skips a store -- a
    single first or last row, a pair of the last trip, a short last group -- then shows as NaN in the result."""
    import torch
    sub_ptr, basis, coarse_index, a0inv, d = inputs(kmax)
    n = basis.shape[1]
    K = a0inv.shape[0]
    gal = ddm.GalerkinPreconditioner(ctx, n, n, np.arange(n, dtype=np.int32), sub_ptr, basis, coarse_index, a0inv, None, None)
    dd = torch.as_tensor(d).to("cuda:0")
    poison = torch.full_like(dd, float("nan"))
    out = {}
    for g in grids:
        part, d0, xov = gal.debug_chain(poison, K, 0 if g > 0 else 5)
        assert torch.isnan(part).all() and torch.isnan(d0).all() and torch.isnan(xov).all(), "the poisoning run must reach every entry"
        out[g] = tuple(t.cpu().numpy().copy() for t in gal.debug_chain(dd, K, g))
    return out


@pytest.fixture(scope="module")
def ctx(ddm):
    return ddm.torch_context(0)


@pytest.mark.parametrize("kmax", KMAX)
def test_grouped_chain_equals_golden_and_full_grid(ddm, ctx, kmax):
    gold = np.load(os.path.join(GOLDEN, f"kmax{kmax}.npz"))
    res = chain_results(ddm, ctx, kmax, [0] + GRIDS)
    assert np.isfinite(gold["x_ovlp"]).all() and np.abs(gold["d0"]).max() > 0 and np.abs(gold["x_ovlp"]).max() > 0
    for g, (part, d0, xov) in res.items():
        # (bytes, not values: -0.0 and 0.0 differ)
        assert part.tobytes() == gold["partial"].tobytes(), f"partials, spread_grid {g}"
        assert d0.tobytes() == gold["d0"].tobytes(), f"coarse defect, spread_grid {g}"
        assert xov.tobytes() == gold["x_ovlp"].tobytes(), f"prolonged correction, spread_grid {g}"
