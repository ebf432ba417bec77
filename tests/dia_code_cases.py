"""Matrices for the coded blocks of the diagonal-row-block operator product (tests/test_dia_code_host.py on the host,
tests/test_gpu_dia_code.py on the device): name -> (scipy CSR matrix with sorted indices and explicit zeros kept, x or None for the
default vector, expected (first row, end row, dictionary entries; 0 = not coded) per block or None where the test states what it
expects itself).  A block of a staged segment whose rows read at most 16 distinct bit patterns is coded."""
import numpy as np
import scipy.sparse as sp

from tests.dia_cases import box27

WG = 256


def q1_box(nodes):
    """27-point Q1 Laplace stencil (x12: centre 32, face neighbours a stored 0.0, edges -2, corners -1) on a box of nx x ny x nz
    nodes with constant coefficient, x fastest; the nodes on the faces are Dirichlet rows (1 on the diagonal, stored zeros beside
    it, and stored zeros in their columns)."""
    import __graft_entry__ as ge
    ge.import_package()
    from dune_ddm_amd import synth
    nx, ny, nz = nodes
    M = synth.stencil_to_csr(synth.assemble_stencil(np.ones((nz - 1, ny - 1, nx - 1)), 3), 3)
    z, y, x = np.indices((nz, ny, nx))
    face = (x == 0) | (x == nx - 1) | (y == 0) | (y == ny - 1) | (z == 0) | (z == nz - 1)
    M = sp.csr_matrix(synth.eliminate_dirichlet(M, face.ravel().astype(np.uint8)))
    M.sort_indices()
    return M


def _with_values(P, data):
    M = sp.csr_matrix((np.asarray(data, dtype=np.float64), P.indices.copy(), P.indptr.copy()), shape=P.shape)
    M.has_sorted_indices = True
    return M


def pooled(P, pools, seed):
    """P's pattern with the entries of the rows [a, b) drawn from `values`, every value at least once, for (a, b, values) in pools"""
    rng = np.random.default_rng(seed)
    data = np.empty(P.nnz)
    for a, b, values in pools:
        z0, z1 = P.indptr[a], P.indptr[b]
        values = np.asarray(values, dtype=np.float64)
        assert z1 - z0 >= len(values)
        pick = np.concatenate([np.arange(len(values)), rng.integers(0, len(values), z1 - z0 - len(values))])
        data[z0:z1] = values[rng.permutation(pick)]
    return _with_values(P, data)


def band_pattern(n, offsets):
    M = sp.diags([np.ones(n - abs(o)) for o in offsets], list(offsets), shape=(n, n), format="csr")
    M.sort_indices()
    return M


def special_vector(n, seed, at):
    """the default vector with -0.0 entries, and +inf, -inf, NaN at the rows `at`: only the blocks around them read these"""
    x = np.random.default_rng(seed).standard_normal(n)
    x[::5] = -0.0
    x[2::9] = 0.0
    x[at[0]], x[at[1]], x[at[2]] = np.inf, -np.inf, np.nan
    return x


def code_cases():
    out = {}
    # 1 320 rows: five full blocks and one of 40 rows, one segment on 27 diagonals; {0, 1, 32, -2, -1} and fewer per block
    box = q1_box((12, 11, 10))
    out["constant_box"] = (box, None, None)
    out["constant_box_special_x"] = (box, special_vector(1320, 41, (300, 700, 1290)), None)
    # two boxes of different size, block-diagonal: two segments, the first block ends early at the decoupling row 60
    out["two_constant_boxes"] = (sp.block_diag([q1_box((5, 4, 3)), q1_box((7, 6, 5))], format="csr"), None, None)
    # the box's pattern: block [0, 256) on exactly 16 values, block [256, 512) on 17, the rest on 3: one segment, mixed
    pool = [float(v) for v in np.arange(1, 18) * 0.375 - 2.0]
    out["16_and_17_values"] = (pooled(box, [(0, 256, pool[:16]), (256, 512, pool), (512, 1320, pool[:3])], 42), None,
                               [(0, 256, 16), (256, 512, 0), (512, 768, 3), (768, 1024, 3), (1024, 1280, 3), (1280, 1320, 3)])
    # +0.0 and -0.0 stored in one block: two dictionary entries; x has negative entries, so the sign of a zero sum depends on which
    out["zeros_and_signs"] = (pooled(band_pattern(100, [-1, 0, 1]), [(0, 100, [0.0, -0.0, 1.5, -2.0])], 43),
                              -np.abs(np.random.default_rng(44).standard_normal(100)) - 0.5, [(0, 100, 4)])
    # column c holds NaN in x: row c - 1 has a stored 0.0 there (NaN), row c + 1 has no entry there (finite), row c its diagonal
    B = sp.lil_matrix(pooled(band_pattern(300, [-1, 0, 1]), [(0, 300, [2.0, -1.0])], 45))
    c = 140
    B[c - 1, c] = 7.0                                                          # (made a stored zero below: lil drops an assigned 0.0)
    j = B.rows[c + 1].index(c)
    del B.rows[c + 1][j], B.data[c + 1][j]
    B = sp.csr_matrix(B)
    B.sort_indices()
    B.data[B.indptr[c - 1] + list(B.indices[B.indptr[c - 1]:B.indptr[c]]).index(c)] = 0.0
    x = np.random.default_rng(46).standard_normal(300)
    x[c] = np.nan
    out["stored_zero_and_absent_entry"] = (B, x, [(0, 256, 3), (256, 300, 2)])
    # 32 diagonals (the whole table: all 128 bits of a code word) on 16 values
    out["full_table"] = (pooled(band_pattern(600, range(-16, 16)), [(0, 600, pool[:16])], 47), None, [(0, 256, 16), (256, 512, 16), (512, 600, 16)])
    # random values on the box pattern: no block is coded
    out["random_values"] = (box27((12, 11, 10), 48), None, [(a, min(a + WG, 1320), 0) for a in range(0, 1320, WG)])
    return out
