"""CPU: the cache-blocked processing order of the GenEO block products (csrc/csr.hpp: csr_row_order_tiled; kernels.hpp:
k_spmm_rowmajor4_tiled).  The order is a performance hint -- it must be a permutation whatever the matrix looks like -- and on the
matrices of the benchmark (27-point stencil on a lexicographic box, overlap shell appended) it must find the grid strides and visit
the rows brick by brick."""
import numpy as np
import scipy.sparse as sp


def _neumann_blocks(ddm, N, parts):
    from dune_ddm_amd import synth
    from dune_ddm_amd.problem import build_structured, _block_diag
    dec = build_structured(synth.StructuredPoisson(N, parts), overlap=2, pou_type="distance", neumann=True)
    A = _block_diag([sd.A_neu for sd in dec.subs])
    bp = np.concatenate([[0], np.cumsum([sd.n for sd in dec.subs])])
    return dec, sp.csr_matrix(A), bp


def test_structured_blocks_are_visited_brick_by_brick(ddm):
    dec, A, bp = _neumann_blocks(ddm, (40, 36, 34), (2, 1, 1))
    found, order = ddm.row_order_tiled_host(bp, A)
    assert found
    assert np.array_equal(np.sort(order), np.arange(A.shape[0]))                      # a permutation
    for b in range(len(bp) - 1):
        seg = order[bp[b]:bp[b + 1]]
        assert seg.min() == bp[b] and seg.max() == bp[b + 1] - 1                       # blocks keep their ranges
    # locality: the columns touched by 256 consecutive rows of the order (one brick) are far fewer than with 256 consecutive rows of
    # the natural order spread over ... the same count, but the bricks ALSO share them across y and z: count distinct columns
    def distinct_cols(rows):
        return len(np.unique(np.concatenate([A.indices[A.indptr[r]:A.indptr[r + 1]] for r in rows])))
    start = int(bp[0]) + 4096
    tiled = distinct_cols(order[start:start + 256])
    natural = distinct_cols(np.arange(start, start + 256))
    assert tiled < 0.75 * natural, (tiled, natural)                                    # 6 x 6 x 18 = 648 against ~9 x 258 = 2 300 at full size


def test_unstructured_matrix_keeps_the_natural_order(ddm):
    rng = np.random.default_rng(0)
    n = 6000
    M = sp.random(n, n, density=0.002, random_state=1, format="csr") + sp.eye(n, format="csr")
    M = sp.csr_matrix(M + M.T)
    M.sort_indices()
    found, order = ddm.row_order_tiled_host([0, n], M)
    assert not found and np.array_equal(order, np.arange(n))


def test_seven_point_and_two_dimensional_stencils(ddm):
    for shape in ((30, 28, 26), (90, 80)):
        n = int(np.prod(shape))
        idx = np.arange(n).reshape(shape[::-1])                                        # x fastest
        rows, cols = [np.arange(n)], [np.arange(n)]
        for ax in range(len(shape)):
            a = np.take(idx, np.arange(shape[::-1][ax] - 1), axis=ax).ravel()
            b = np.take(idx, np.arange(1, shape[::-1][ax]), axis=ax).ravel()
            rows += [a, b]
            cols += [b, a]
        M = sp.csr_matrix((np.ones(sum(len(r) for r in rows)), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
        M.sort_indices()
        found, order = ddm.row_order_tiled_host([0, n], M)
        assert found and np.array_equal(np.sort(order), np.arange(n))
        first = order[:64]                                                             # one 16 x 4 (x 1) patch of a brick: four grid lines
        assert len(np.unique(first // shape[0])) == 4
