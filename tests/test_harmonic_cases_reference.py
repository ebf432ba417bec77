"""CPU: pins tests/harmonic_cases.py -- the cases have the properties their table states, the float64 oracle agrees with the refined
reference far inside the tolerance on exactly these inputs, and every seeded fault is far outside it.  No case is filtered.

Measured here: the oracle's largest ratio to the tolerance is 1.1e-5 (a distance of 1.1e-15 of the column's largest entry); the
refinement settles after 1 or 2 steps; the smallest movement by a seeded fault is 1e9 tolerances (the largest over the columns of the
block: a single dropped entry moves a column in proportion to one random input value).

One fault of the list moves nothing and is pinned as such (hc.FAULT_WITHOUT_EFFECT): a neither column kept in A^ alone multiplies an
unknown whose row of A^ is an identity row with a zero right-hand side.  It shows in the symmetry of A^ instead (the device test
asserts `symmetric`, and that P^T is offered, on every symmetric case with neither rows); the neither column kept in G_ib is the
fault of this kind that moves results, and is in the list."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import harmonic_cases as hc


def test_matrices_are_what_the_table_says():
    for name in ("poisson", "dominant_sym", "dominant_gen", "nearly_sym_lo", "nearly_sym_hi", "uneven9"):
        M, bp, pos = hc.matrix(name)
        n = M.shape[0]
        assert M.has_sorted_indices and np.all(M.diagonal() > 0) and bp[0] == 0 and bp[-1] == n and n <= 2000
        blk = np.searchsorted(bp, np.arange(n), side="right") - 1
        C = sp.coo_matrix(M)
        assert np.all(blk[C.row] == blk[C.col]), "block diagonal"
        assert (abs(M) > 0).astype(int).nnz == M.nnz and (sp.csr_matrix(abs(M) > 0) != sp.csr_matrix(abs(M.T) > 0)).nnz == 0, "symmetric pattern"
        off = abs(M) - sp.diags(M.diagonal())
        if name == "dominant_gen":
            assert np.all(M.diagonal() > 1.05 * np.asarray(off.sum(axis=0)).ravel()), "strictly column dominant"
            assert abs(M - M.T).max() > 0.1
        elif name != "poisson":
            assert np.all(M.diagonal() > 1.04 * np.asarray(off.sum(axis=1)).ravel()), "strictly diagonally dominant"
        else:
            assert np.all(np.diff(bp) == [528, 396, 396]) and np.all(M.diagonal() == 6.0) and set(off.data) == {1.0}
    S, _, pos = hc.matrix("dominant_sym")
    assert abs(S - S.T).max() == 0.0
    i, j = hc.perturbed_pair(pos)
    for name, rel in (("nearly_sym_lo", 1e-13), ("nearly_sym_hi", 1e-9)):
        M = hc.matrix(name)[0]
        D = sp.coo_matrix(M - S)
        D.eliminate_zeros()
        assert D.nnz == 1 and (D.row[0], D.col[0]) == (i, j)
        got = abs(M[i, j] - M[j, i]) / (abs(M[i, j]) + abs(M[j, i]))
        assert 0.4 * rel < got < 0.6 * rel and (got > 1e-12) == (name == "nearly_sym_hi")
    assert list(np.diff(hc.matrix("uneven9")[1])) == [1584, 1, 60, 1, 36, 18, 120, 63, 8]


@pytest.mark.parametrize("name", hc.NAMES)
def test_classes_are_what_the_table_says(name):
    c = hc.case(name)
    s, cls, bp = c.spec, c.cls, c.block_ptr
    share = [np.mean(cls == k) for k in (0, 1, 2)]
    assert len(c.ii) > 0 and np.all(c.A.diagonal()[c.ii] != 0.0)
    assert c.values_symmetric() == s.symmetric
    if s.classes in ("shell", "dup", "blocks"):
        i, j = hc.perturbed_pair(c.pos)
        assert cls[i] == cls[j] == hc.INTERIOR
        # neither rows lie beside interior rows: G_ib and A^ must drop their columns
        C = sp.coo_matrix(c.A)
        assert np.any((cls[C.row] == hc.INTERIOR) & (cls[C.col] == hc.NEITHER))
    if s.classes == "all":
        assert share[2] == 0.0
    if s.classes == "random":
        assert abs(share[0] - 0.65) < 0.04 and abs(share[1] - 0.25) < 0.04 and abs(share[2] - 0.10) < 0.03
    if s.classes == "no_boundary":
        assert share[1] == 0.0 and c.embedded(False)[0][-1] == 0
    if s.classes == "dup":
        ii, bb = hc.index_lists(cls)
        assert len(bb) == len(c.bb) + (len(c.bb) + 4) // 5 and np.array_equal(np.unique(bb), c.bb) and np.array_equal(ii, c.ii)
        assert np.array_equal(cls, hc.case("poisson-shell").cls)
    if s.classes == "blocks":
        per = [cls[bp[b]:bp[b + 1]] for b in range(9)]
        assert per[1].tolist() == [hc.INTERIOR] and per[3].tolist() == [hc.BOUNDARY]
        assert np.all(per[4] == hc.INTERIOR) and np.all(per[5] == hc.BOUNDARY) and not np.any(per[8] == hc.INTERIOR)
        assert len(per[0]) >= 1500 and (per[0] == hc.INTERIOR).sum() > 64
        rp = c.embedded(False)[0]
        assert rp[bp[5]] == rp[bp[4]] and rp[bp[6]] == rp[bp[5]], "blocks 4 and 5 have no row of G_ib"


def test_error_case_has_an_interior_row_without_interior_entries():
    A, bp, cls, row = hc.error_case()
    cols = A.indices[A.indptr[row]:A.indptr[row + 1]]
    assert cls[row] == hc.INTERIOR and len(cols) == 6 and row not in cols and np.all(cls[cols] == hc.BOUNDARY)
    others = np.nonzero(cls == hc.INTERIOR)[0]
    assert all(r in A.indices[A.indptr[r]:A.indptr[r + 1]] for r in others if r != row)


def test_shape_table_predicts_kernels_and_panels():
    S = hc.Shapes
    quad, scalar = "k_spmm_rowmajor4", "k_spmm_rowmajor"
    assert [hc.extend_lds(k) for k in (1, 4, 48, 96, 97)] == [(1, 4, 8), (4, 7, 12), (48, 51, 56), (96, 99, 104), (97, 100, 104)]
    seen = set()
    for nrhs in hc.EXTEND_WIDTHS:
        for ldx in hc.extend_lds(nrhs):
            calls = S.extend_calls(nrhs, ldx)
            assert sum(w for _, w, _ in calls) == nrhs and len(calls) == -(-nrhs // 48) and all(c0 % 4 == 0 for c0, _, _ in calls)
            for c0, w, k in calls:
                assert (k == quad) == (w % 4 == 0 and ldx % 4 == 0)
                assert S.panels(w, "device") == [w] and S.panels(w, "host") == [w]
                seen.add((k, c0 > 0))
    assert seen == {(quad, False), (quad, True), (scalar, False), (scalar, True)}
    assert [k for _, _, k in S.extend_calls(97, 104)] == [quad, quad, scalar] and [k for _, _, k in S.extend_calls(96, 99)] == [scalar, scalar]
    assert [k for _, _, k in S.extend_calls(49, 56)] == [quad, scalar] and [k for _, _, k in S.extend_calls(4, 7)] == [scalar]
    for m in hc.PROJ_WIDTHS:
        for ld, slot in hc.proj_layouts(m):
            assert (S.proj_kernel(m, ld, slot) == quad) == (m % 4 == 0)
    assert S.panels(52, "device") == [48, 4] and S.panels(52, "host") == [52] and S.panels(48, "device") == [48]
    assert S.mm_kernel(4, 12, 4, 3) == scalar                              # what an unaligned offset would take


@pytest.mark.parametrize("name", hc.NAMES)
def test_oracle_is_within_a_quarter_of_the_tolerance(name):
    from oracle import coarse_oracle as co
    c = hc.case(name)
    ref = c.extend_ref(hc.WMAX)
    assert c.steps <= 3
    ext = co.EnergyMinimalExtension(c.A, c.ii, c.bb)
    got = np.stack([ext.extend(c.X[c.bb, j]) for j in range(hc.WMAX)], axis=1)
    ratio = hc.column_ratio(got, ref)
    print(f"\n[harmonic cases] {name}: oracle / tolerance {ratio.max():.2e}, refinement steps {c.steps}")
    assert ratio.max() <= 0.25
    # the float64 model of the library's steps is the same operation
    assert hc.column_ratio(c.model("extend", hc.WMAX)[c.ii], ref).max() <= 0.25
    assert hc.column_ratio(c.model("P", 52), c.P_ref(52)).max() <= 0.25
    assert hc.column_ratio(c.model("Pt", 52), c.Pt_ref(52)).max() <= 0.25
    if name in hc.SYMMETRIC:
        # T T^T from the dense T against the operator form D A_ii^-1 A_ib A_ib^T A_ii^-T D in float64
        z = c.lut.solve(c.d[c.ii, None] * c.R[c.ii])
        y = c.d[c.ii, None] * c.lu.solve(c.Aib @ (c.Aib.T @ z))
        assert hc.column_ratio(y, c.TTt_ref(52)[c.ii]).max() <= 0.25 and np.all(c.TTt_ref(52)[c.cls != hc.INTERIOR] == 0.0)


def _applies(fault, c):
    if fault in ("gib_entry_dropped", "gbi_entry_untransposed", "chunk_reads_first"):
        return len(c.embedded(False)[2]) > 0                               # (no_boundary: G_ib is empty, every result is zero)
    if fault in ("gib_keeps_neither", "keep_for_keep_b"):
        return len(c.nn) > 0 and len(c.bb) > 0
    if fault == "inverse_for_transposed_inverse":
        return c.spec.matrix == "dominant_gen"
    return True


@pytest.mark.parametrize("fault", hc.FAULTS)
def test_seeded_faults_move_the_result_a_thousand_tolerances(fault):
    ops = {"gib_entry_dropped": ("extend", "P"), "gbi_entry_untransposed": ("Pt",), "gib_keeps_neither": ("extend", "P"), "keep_for_keep_b": ("P", "Pt"),
           "inverse_for_transposed_inverse": ("Pt",), "chunk_reads_first": ("extend",)}[fault]
    ran, least = 0, np.inf
    for name in hc.NAMES:
        c = hc.case(name)
        if not _applies(fault, c):
            continue
        for op in ops:
            m = hc.WMAX if op == "extend" else 52
            got = c.model(op, m, fault)
            if op == "extend":
                moved = hc.column_ratio(got[c.ii], c.extend_ref(m))
                if fault == "chunk_reads_first":
                    moved = moved[48:]                                     # the columns of the later chunks
            else:
                moved = hc.column_ratio(got, c.P_ref(m) if op == "P" else c.Pt_ref(m))
            least = min(least, float(moved.max()))
            assert moved.max() >= 1000.0, (fault, name, op, moved.max())
            ran += 1
    print(f"\n[harmonic cases] {fault}: {ran} (case, operation) pairs, least movement {least:.2e} tolerances")
    assert ran >= 2


@pytest.mark.parametrize("name", hc.NAMES)
def test_a_neither_column_kept_in_the_interior_matrix_alone_moves_nothing(name):
    c = hc.case(name)
    C = sp.coo_matrix(c.A)
    k = (c.cls[C.row] == hc.INTERIOR) & (c.cls[C.col] == hc.NEITHER)
    for op, ref in (("extend", c.model("extend", 52)), ("P", c.model("P", 52)), ("Pt", c.model("Pt", 52))):
        got = c.model(op, 52, hc.FAULT_WITHOUT_EFFECT)
        assert hc.column_ratio(got, ref).max() <= 0.25, (name, op)
    if k.any():
        assert not c.values_symmetric(extra=list(zip(C.row[k], C.col[k], C.data[k]))[:1]), "but A^ is no longer symmetric"


@pytest.mark.parametrize("name", hc.NAMES)
def test_interior_matrix_as_input_of_the_supernodal_analysis(ddm, name):
    """A^ has an identity row for every row outside the interior: isolated vertices, so the elimination forest of a block has many
    roots and one-column supernodes without rows below.  The host half of the device engine (ordering, supernodes, row lists,
    levels) must stay consistent on it: this is what the factorisation and solve kernels index with."""
    c = hc.case(name)
    Ah = c.Ahat()
    bp = c.block_ptr
    roots = bare = 0
    for b, d in enumerate(ddm.sn_symbolic_host(Ah, bp)):
        nb = int(bp[b + 1] - bp[b])
        first, rptr, rows, parent, level = d["first"], d["rptr"], d["rows"], d["parent"], d["level"]
        nsn = len(parent)
        assert sorted(d["perm"].tolist()) == list(range(nb)), (name, b, "perm is no permutation of the block")
        assert first[0] == 0 and first[-1] == nb and np.all(np.diff(first) >= 1)
        assert rptr[0] == 0 and rptr[-1] == len(rows) and np.all(np.diff(rptr) >= 0)
        assert len(rows) == 0 or (rows.min() >= 0 and rows.max() < nb)
        for s in range(nsn):
            r = rows[rptr[s]:rptr[s + 1]]
            w = first[s + 1] - first[s]
            # a supernode's row list begins with its own columns (when it lists them) and goes on strictly above them
            below = r[r >= first[s + 1]]
            assert np.all(np.diff(r) > 0) and np.all(r >= first[s]) and len(r) - len(below) in (0, w), (name, b, s)
            assert parent[s] == -1 or (s < parent[s] < nsn and level[parent[s]] > level[s])
            if len(below):
                assert parent[s] != -1 and first[parent[s]] <= below[0] < first[parent[s] + 1]
            roots += parent[s] == -1
            bare += w == 1 and len(below) == 0
        assert level.min() == 0 and d["levels"] == level.max() + 1
    outside = c.n - len(c.ii)
    assert roots >= min(outside, 1) and bare >= min(outside, 1)
    print(f"\n[harmonic cases] {name}: {roots} roots, {bare} one-column supernodes without rows below ({outside} identity rows)")
