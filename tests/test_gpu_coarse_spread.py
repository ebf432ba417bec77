"""-m gpu: the spread passes over the coarse basis (k_coarse_restrict_spread / k_coarse_prolong_spread: one-wave workgroups,
persistent) against the full-grid kernels they stand in for beside the local solve, through the diagnostic entry
ddm_galerkin_debug_chain.  Same sums in the same order: chunk partials, coarse defect and prolonged correction are torch.equal."""
import numpy as np
import pytest

from tests.coarse_cases import ragged_basis

pytestmark = pytest.mark.gpu

# 2x2x2 subdomains, overlap 2.  24^3 and 33^3: one short chunk per subdomain (2744 and up to 6859 rows: no multiple of 64, the last
# trip incomplete); 44^3: 13824 rows per subdomain, a full 8192-row chunk and a shorter one.  "ragged": 5 vectors, 3 on subdomain 5
# (zero rows, coarse_index < 0; one trip of four vectors and a single one); "pou": one vector.
SHAPES = [(24, "ragged"), (33, "ragged"), (33, "pou"), (44, "ragged")]
# one wave for everything; a grid that divides neither the work items nor the CUs; more waves than work items (8 to 80 of them)
GRIDS = [1, 7, 1024]


@pytest.fixture(scope="module")
def levels(ddm):
    """per shape: the two-level object and the full-grid chain's results for two defects, computed once"""
    import torch
    from dune_ddm_amd import synth
    from dune_ddm_amd.problem import build_structured
    from dune_ddm_amd.solver import TwoLevelSchwarz, pou_basis
    cache = {}

    def get(grid, coarse):
        if (grid, coarse) not in cache:
            dec = build_structured(synth.StructuredPoisson((grid,) * 3, (2, 2, 2)), overlap=2, pou_type="distance", shrink=0)
            tl = TwoLevelSchwarz(dec, coarse="none", mode="additive")
            tl.set_coarse_basis(ragged_basis(tl.rl) if coarse == "ragged" else pou_basis(tl.rl))
            rng = np.random.default_rng(grid)
            defects = [tl.to_device(rng.standard_normal(tl.rl.n)) for _ in range(2)]
            refs = [tl.galerkin.debug_chain(d, tl.K, 0) for d in defects]
            for part, d0, xov in refs:
                assert torch.isfinite(part).all() and torch.isfinite(xov).all() and d0.abs().max() > 0 and xov.abs().max() > 0
            cache[(grid, coarse)] = (tl, defects, refs)
        return cache[(grid, coarse)]
    return get


@pytest.mark.parametrize("spread_grid", GRIDS)
@pytest.mark.parametrize("grid,coarse", SHAPES)
def test_spread_chain_equals_full_grid_chain(levels, grid, coarse, spread_grid):
    import torch
    tl, defects, refs = levels(grid, coarse)
    for d, (part, d0, xov) in zip(defects, refs):
        got = tl.galerkin.debug_chain(d, tl.K, spread_grid)
        assert torch.equal(got[0], part)
        assert torch.equal(got[1], d0)
        assert torch.equal(got[2], xov)
