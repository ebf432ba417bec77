"""Matrices for the diagonal-row-block operator product (tests/test_dia_host.py on the host, tests/test_gpu_dia_spmv.py on the
device): name -> (scipy CSR matrix with sorted indices, expected blocks as (first row, end row, diagonals; 0 = CSR-stream, slabs
stored: the offsets >= 0 only in a segment that is symmetric bit for bit) or None where only the product is checked).  Values hold stored zeros and -0.0 (present entries, not skipped)."""
import numpy as np
import scipy.sparse as sp


def box27(shape, seed, symmetric=True):
    """27-point stencil on a box in lexicographic numbering, truncated at the faces (boundary rows have absent entries)"""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    idx = np.arange(nx * ny * nz).reshape(nz, ny, nx)
    rows, cols = [], []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                a = idx[max(0, -dz):nz - max(0, dz), max(0, -dy):ny - max(0, dy), max(0, -dx):nx - max(0, dx)]
                b = idx[max(0, dz):nz + min(0, dz), max(0, dy):ny + min(0, dy), max(0, dx):nx + min(0, dx)]
                rows.append(a.ravel())
                cols.append(b.ravel())
    r, c = np.concatenate(rows), np.concatenate(cols)
    v = rng.standard_normal(len(r))
    v[::7] = 0.0                                   # stored zeros (the Q1 stencil's face neighbours)
    v[3::11] = -0.0
    M = sp.coo_matrix((v, (r, c)), shape=(idx.size, idx.size)).tocsr()
    if symmetric:                                  # mirror the upper triangle: bitwise symmetric values
        U = sp.triu(M, 1, format="csr")
        D = sp.csr_matrix((M.diagonal(), (np.arange(idx.size), np.arange(idx.size))), shape=M.shape)
        M = _with_pattern(U + U.T + D, M)
    M.sort_indices()
    return M


def _with_pattern(S, P):
    """S's values on P's pattern (scipy's sum drops nothing here, but a stored zero must stay a stored entry)"""
    S = sp.csr_matrix(S)
    S.sort_indices()
    P = sp.csr_matrix(P)
    P.sort_indices()
    out = P.copy()
    out.data[:] = 0.0
    lookup = {(i, j): S.data[z] for i in range(S.shape[0]) for z, j in zip(range(S.indptr[i], S.indptr[i + 1]), S.indices[S.indptr[i]:S.indptr[i + 1]])}
    for i in range(P.shape[0]):
        for z in range(P.indptr[i], P.indptr[i + 1]):
            out.data[z] = lookup.get((i, int(P.indices[z])), 0.0)
    return out


def band(n, half, seed):
    """rows with the offsets -half .. half, truncated at both ends"""
    rng = np.random.default_rng(seed)
    M = sp.diags([rng.standard_normal(n - abs(o)) for o in range(-half, half + 1)], list(range(-half, half + 1)), format="csr")
    M.sort_indices()
    return M


def _replace_rows(M, new_rows):
    """M with the rows in new_rows = {row: (cols, vals)} replaced"""
    M = sp.lil_matrix(M)
    for r, (c, v) in new_rows.items():
        order = np.argsort(c)
        M.rows[r] = [int(j) for j in np.asarray(c)[order]]
        M.data[r] = [float(a) for a in np.asarray(v)[order]]
    M = sp.csr_matrix(M)
    M.sort_indices()
    return M


def cases():
    rng = np.random.default_rng(42)
    out = {}
    # two boxes of different size: the table changes at row 60 (33 offsets together), so the first block ends early
    out["two_boxes"] = (sp.block_diag([box27((5, 4, 3), 1), box27((7, 6, 5), 2)], format="csr"), [(0, 60, 27, 14), (60, 270, 27, 14)])
    # 40 rows of 40 random columns each between stencil rows: a CSR-stream block in the middle
    rows = {r: (rng.choice(300, 40, replace=False), rng.standard_normal(40)) for r in range(130, 170)}
    out["csr_in_the_middle"] = (_replace_rows(band(300, 2, 3), rows), [(0, 130, 5, 5), (130, 170, 0, 0), (170, 300, 5, 5)])
    empty = {r: (np.zeros(0, dtype=int), np.zeros(0)) for r in [10, 11, 12, 13, 14, 97, 98, 99]}
    out["empty_rows"] = (_replace_rows(band(100, 2, 4), empty), [(0, 100, 5, 5)])
    out["all_empty"] = (sp.csr_matrix((10, 10)), [(0, 10, 0, 0)])
    long_row = {700: (np.arange(2100), rng.standard_normal(2100))}
    out["long_row"] = (_replace_rows(band(2200, 2, 5), long_row),
                       [(0, 256, 5, 5), (256, 512, 5, 5), (512, 700, 5, 5), (700, 701, 0, 0)] + [(a, min(a + 256, 2200), 5, 5) for a in range(701, 2200, 256)])
    B = band(600, 2, 10)
    B = sp.csr_matrix(sp.triu(B, 0) + sp.triu(B, 1).T)
    B.sort_indices()
    out["symmetric_band"] = (B, [(0, 256, 5, 3), (256, 512, 5, 3), (512, 600, 5, 3)])   # one segment of three blocks, half stored
    out["one_by_one"] = (sp.csr_matrix(np.array([[3.0]])), [(0, 1, 1, 1)])
    out["not_a_multiple_of_64"] = (band(333, 3, 6), [(0, 256, 7, 7), (256, 333, 7, 7)])
    M = box27((6, 5, 4), 7)
    z = M.indptr[50] + 2                                                        # one entry off by one ulp: no longer symmetric in value
    M.data[z] = np.nextafter(M.data[z] if M.data[z] != 0.0 else 1.0, np.inf)
    out["one_ulp_off_symmetry"] = (M, [(0, 120, 27, 27)])                     # full storage
    # symmetric, the offset table changes mid-way (at row 256: +-40..42 among the rows before, +-2..13 among the rows from there on,
    # 0, +-1, +-150 everywhere: 35 offsets together): the first segment is symmetric inside itself and keeps half; the entries
    # (r, r - 150) of the second point into the first, so it keeps all slabs
    rr, cc = [], []
    for r in range(512):
        for o in [0, 1, 150] + ([40, 41, 42] if r + 42 < 256 else []) + (list(range(2, 14)) if r >= 256 else []):
            if r + o < 512:
                rr.append(r)
                cc.append(r + o)
    U = sp.coo_matrix((rng.standard_normal(len(rr)), (rr, cc)), shape=(512, 512)).tocsr()
    S = sp.csr_matrix(U + sp.triu(U, 1).T)
    S.sort_indices()
    out["table_changes_midway"] = (S, [(0, 256, 11, 6), (256, 512, 29, 29)])
    r = np.repeat(np.arange(200), 45)                                           # 45 entries in every row (a band that wraps around)
    W = sp.coo_matrix((rng.standard_normal(9000), (r, (r + np.tile(np.arange(-22, 23), 200)) % 200)), shape=(200, 200)).tocsr()
    W.sort_indices()
    out["45_per_row"] = (W, [(a, min(a + 45, 200), 0, 0) for a in range(0, 200, 45)])   # (45 rows = 2025 entries per CSR-stream block)
    # irregular rows on few shared diagonals: slabs less than half full, so CSR-stream
    r = np.repeat(np.arange(200), 5)
    c = np.concatenate([rng.choice(200, 5, replace=False) for _ in range(200)])
    I = sp.coo_matrix((rng.standard_normal(1000), (r, c)), shape=(200, 200)).tocsr()
    I.sort_indices()
    out["irregular"] = (I, None)
    return out


def reference_mv(M, x):
    """row by row, products rounded and summed in column order from 0.0"""
    y = np.zeros(M.shape[0])
    for r in range(M.shape[0]):
        s = 0.0
        for z in range(M.indptr[r], M.indptr[r + 1]):
            s = s + float(M.data[z]) * float(x[M.indices[z]])
        y[r] = s
    return y


def vector(n, seed):
    x = np.random.default_rng(seed).standard_normal(n)
    x[::5] = -0.0
    x[2::9] = 0.0
    return x
