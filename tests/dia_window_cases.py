"""Matrices for the x windows of the diagonal-row-block operator product (tests/test_dia_window_host.py on the host,
tests/test_gpu_dia_window.py on the device), beside those of tests/dia_cases.py: name -> (scipy CSR matrix with sorted indices,
x or None for the default vector, expected segments as (staged, runs, window doubles) or None where only the invariants are
checked).  WG rows per full block and the capacity (doubles of window a staged segment may take) are what the library reports;
window_cases(capacity, wg) builds the two cases that depend on them."""
import numpy as np
import scipy.sparse as sp

from tests.dia_cases import band, box27


def offsets_matrix(n, offsets, seed):
    """rows with one entry at each of the given col - row, where the column exists"""
    rng = np.random.default_rng(seed)
    M = sp.diags([rng.standard_normal(n - abs(o)) for o in offsets], list(offsets), shape=(n, n), format="csr")
    M.sort_indices()
    return M


def fill_offsets(capacity, wg):
    """offsets whose windows take exactly `capacity` doubles: one run {0, wg (, wg + capacity % wg)} and single offsets 2 wg + 88 apart"""
    first = [0, wg] + ([wg + capacity % wg] if capacity % wg else [])
    singles = capacity // wg - 2
    return first + [first[-1] + (2 * wg + 88) * (j + 1) for j in range(singles)]


def window_cases(capacity=2048, wg=256):
    out = {}
    # 1 080 rows, plane 360: the offsets are three runs of span 82; five blocks, the last of 56 rows; half storage
    out["box_40_9_3"] = (box27((40, 9, 3), 31), None, [(True, 3, 3 * (wg + 82))])
    M = box27((6, 5, 4), 7)
    z = M.indptr[50] + 2                                                        # (as one_ulp_off_symmetry: full storage)
    M.data[z] = np.nextafter(M.data[z] if M.data[z] != 0.0 else 1.0, np.inf)
    out["box_6_5_4_full"] = (M, None, [(True, 1, wg + 74)])
    out["two_diagonals_one_run"] = (offsets_matrix(1000, [0, wg], 32), None, [(True, 1, 2 * wg)])          # the merge rule at its boundary
    out["two_diagonals_two_runs"] = (offsets_matrix(1000, [0, wg + 1], 33), None, [(True, 2, 2 * wg)])
    fill = fill_offsets(capacity, wg)
    out["fills_capacity"] = (offsets_matrix(10000, fill, 34), None, [(True, capacity // wg - 1, capacity)])
    out["one_past_capacity"] = (offsets_matrix(10000, fill + [fill[-1] + 3 * wg], 35), None, [(False, capacity // wg, capacity + wg)])
    far = [300 * k for k in range(-16, 16)]                                     # 32 offsets pairwise more than wg apart
    out["32_far_offsets"] = (offsets_matrix(10000, far, 36), None, [(False, 32, 32 * wg)])
    out["n_1"] = (sp.csr_matrix(np.array([[-2.5]])), None, [(True, 1, wg)])     # every window element but one is clamped
    out["n_63"] = (band(63, 3, 37), None, [(True, 1, wg + 6)])
    # a band with the empty column c: x[c] is in the windows of the rows around it, but no entry reads it
    B = sp.lil_matrix(band(300, 3, 38))
    c = 140
    for r in range(c - 3, c + 4):
        if c in B.rows[r]:
            j = B.rows[r].index(c)
            del B.rows[r][j], B.data[r][j]
    B = sp.csr_matrix(B)
    B.sort_indices()
    x = np.random.default_rng(39).standard_normal(300)
    x[c], x[c - 1], x[c + 1] = np.nan, np.inf, -np.inf
    out["empty_column"] = (B, x, [(True, 1, wg + 6)])
    return out
