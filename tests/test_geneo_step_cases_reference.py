"""CPU: pins the cases and the host references of tests/geneo_step_cases.py, which tests/test_gpu_geneo_steps.py compares the device
steps of the GenEO block eigensolver with.

  1. every reason a width of WIDTHS is in the list holds for the restated dispatch conditions (Shapes), and the matrix of the
     sparse steps has the properties its docstring claims (row order found and not the identity on the grid block, row lengths,
     ragged tiled grid, symmetric positive definite / diagonally dominant first values, unrelated second values);
  2. every host reference stays within its own bound of a long-double evaluation, with room to spare; the ratios are printed;
  3. the splitmix64 restatement of k_geneo_random lies in [-0.5, 0.5) and its columns are not constant."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import geneo_step_cases as gc


def test_widths_reach_what_they_are_listed_for():
    sh = {m: gc.Shapes(m) for m in gc.WIDTHS}
    assert gc.WIDTHS == (6, 7, 8, 24, 28, 32, 36, 48)
    # 6: ld = 18 is not a multiple of 4 -> scalar product and sweep kernels in every slot
    assert sh[6].ld == 18 and sh[6].ld % 4 != 0
    for k in range(3):
        assert sh[6].product_kernels(k, True, True) == ["k_spmm_rowmajor"] * 2 and sh[6].product_kernels(k, False, True) == ["k_spmm_rowmajor"]
    assert sh[6].level_kernel(False, 27) == sh[6].level_kernel(True, 27) == "k_trsv_level_multi"
    # 7: odd, and the W slot starts 56 bytes into a row
    assert 8 * gc.slot(7, 1).start == 56 and not sh[7].aligned(1) and not sh[7].quad_product(1) and not sh[7].quad_solve()
    assert sh[7].product_kernels(1, True, True) == ["k_spmm_rowmajor"] * 2 and sh[7].level_kernel(True, 27) == "k_trsv_level_multi"
    # 8: the smallest quad case, tiled with a row order, untiled without
    assert sh[8].nq == 2 and all(sh[8].quad_product(k) for k in range(3)) and sh[8].quad_solve()
    assert sh[8].product_kernels(1, True, True) == ["k_spmm_rowmajor4_tiled<true>"] and sh[8].product_kernels(1, True, False) == ["k_spmm_rowmajor4<true>"]
    assert sh[8].product_kernels(1, False, True) == ["k_spmm_rowmajor4<false>"]
    assert sh[8].level_kernel(False, 27) == "k_trsv_level_multi4" and sh[8].level_kernel(True, 27) == "k_trsv_level_multi4_f32"
    # 24: the benchmark's width; one rotation launch; single-precision sweeps
    assert sh[24].nq == 6 and (sh[24].p, sh[24].q) == (72, 48)
    assert sh[24].rayleigh_ritz_rotation() == [(0, 48, 0, 72, 0, "k_rotate_mfma<20, 3>")]
    assert sh[24].level_kernel(True, 27) == "k_trsv_level_multi4_f32" and sh[24].level_kernel(True, 27, contiguous=True) == "k_trsv_level_multi4_f32"
    assert sh[24].gram_kernel(24, 24, True) == "k_gram_small<true, true, true>" and sh[24].gram_kernel(24, 24, False) == "k_gram_small<false, true, true>"
    # 28: inner pieces 72 + 12 (modes 0, 3), output panels 48 + 8, the gap inside the first panel
    assert sh[28].p == 84 > gc.ROT_KMAX and sh[28].q == 56 and sh[28].nq == 7
    assert sh[28].rayleigh_ritz_rotation() == [(0, 48, 0, 72, 0, "k_rotate_mfma<20, 3>"), (0, 48, 72, 12, 3, "k_rotate_mfma<20, 3>"),
                                               (48, 8, 0, 72, 0, "k_rotate_mfma<20, 1>"), (48, 8, 72, 12, 3, "k_rotate_mfma<20, 1>")]
    assert 0 < 28 < gc.ROT_PANEL
    assert sh[28].gram_kernel(28, 28, True) == "k_gram_small<true, true, true>" and sh[28].product_kernels(2, True, True) == ["k_spmm_rowmajor4_tiled<true>"]
    # 32: the last width of k_gram_small and of the tiled product
    assert sh[32].nq == 8 == gc.SPMM_TILED_NQ and sh[32].product_kernels(0, True, True) == ["k_spmm_rowmajor4_tiled<true>"]
    assert sh[32].gram_kernel(32, 32, True).startswith("k_gram_small<true") and sh[32].gram_kernel(33, 33, True) == "k_gram_mfma<2, 5>"
    # 36: untiled although a row order exists; Gram on the general kernel; q = 72
    assert sh[36].nq == 9 and sh[36].product_kernels(1, True, True) == ["k_spmm_rowmajor4<true>"]
    assert sh[36].gram_kernel(36, 36, True) == "k_gram_mfma<2, 5>" and sh[36].q == 72
    assert [(j0, qq) for j0, qq, k0, _, _, _ in sh[36].rayleigh_ritz_rotation() if k0 == 0] == [(0, 48), (48, 24)]
    # 48: p = 144 as 72 + 72, q = 96 with the gap at the panel boundary
    rot = sh[48].rayleigh_ritz_rotation()
    assert [(k0, kk, mode) for j0, _, k0, kk, mode, _ in rot if j0 == 0] == [(0, 72, 0), (72, 72, 3)]
    assert [(j0, qq) for j0, qq, k0, _, _, _ in rot if k0 == 0] == [(0, 48), (48, 48)] and gc.ROT_PANEL == 48
    # the orthogonalisation W <- W - X G is one launch in mode 1 at every width
    for m in gc.WIDTHS:
        orth = sh[m].orthogonalisation()
        assert len(orth) == 1 and orth[0][:5] == (0, m, 0, m, 1)
    # every launch geometry of the rotation kernel that the widths produce: both staging variants, 1 to 3 output tiles
    kernels = {l[5] for m in gc.WIDTHS for l in sh[m].rayleigh_ritz_rotation() + sh[m].orthogonalisation()}
    assert kernels == {f"k_rotate_mfma<20, {t}>" for t in (1, 2, 3)}, kernels


def test_dense_rows_are_ragged():
    assert gc.SIZES == (4099, 17, 2048, 1, 6150)
    ch = gc.chunks()
    assert len(ch) == 3 + 1 + 1 + 1 + 4
    assert any((r1 - r0) % 4 for r0, r1, _ in ch) and any((r1 - r0) % 16 for r0, r1, _ in ch) and any(r1 - r0 == gc.CHUNK_ROWS for r0, r1, _ in ch)
    d = gc.dense(7)
    assert len({d.mu[s].tobytes() for s in range(d.nsub)}) == d.nsub and np.any(d.w == 0.0)


def test_sparse_case_is_what_it_claims(ddm):
    sc = gc.sparse()
    assert (sc.n0, sc.n1, sc.n) == (4624, 700, 5324) and sc.n0 >= gc.ROW_ORDER_MIN > sc.n1
    assert sc.n % 64 == 12 and -(-sc.n // gc.SPMM_TILED_ROWS) == 84 and 84 % 8 == 4
    found, order = ddm.row_order_tiled_host(sc.block_ptr, sc.M)
    assert found and sorted(order.tolist()) == list(range(sc.n))
    assert not np.array_equal(order[:sc.n0], np.arange(sc.n0)) and sorted(order[:sc.n0].tolist()) == list(range(sc.n0))
    assert np.array_equal(order[sc.n0:], np.arange(sc.n0, sc.n))          # the irregular rows keep the natural order
    # row lengths: the interior of the grid has 27 entries; block 1 cycles through LENGTHS
    assert sc.lengths[:sc.n0].max() == 27 and sc.lengths[:sc.n0].min() == 8
    assert np.array_equal(sc.lengths[sc.n0:], np.resize(gc.LENGTHS, sc.n1))
    assert {3, 4, 5} <= set(gc.LENGTHS) and {5, 8, 9} <= set(gc.LENGTHS)  # on both sides of the unroll depths 4 and 8
    assert sorted(gc.UNROLL.values()) == [4, 8, 8]
    assert 0 in gc.LENGTHS and max(gc.LENGTHS) > 3 * 8
    # block diagonal
    coo = sc.M.tocoo()
    assert np.all((coo.row < sc.n0) == (coo.col < sc.n0))
    # first values: grid block symmetric with a positive, strictly dominant diagonal; block 1 strictly row dominant
    A0 = sc.M[:sc.n0][:, :sc.n0]
    assert abs(A0 - A0.T).max() == 0.0
    dg = sc.M.diagonal()
    offsum = np.asarray(abs(sc.M).sum(axis=1)).ravel() - np.abs(dg)
    nonempty = sc.lengths > 0
    assert np.all(dg[nonempty] > offsum[nonempty]) and np.all(dg[~nonempty] == 0.0)
    F = sc.factor_matrix
    assert F.nnz == sc.M.nnz + int(np.sum(~nonempty)) and np.all(F.diagonal() > offsum)
    # second values: unrelated to the first and asymmetric
    C0 = sc.C[:sc.n0][:, :sc.n0]
    assert abs(C0 - C0.T).max() > 0.1 and abs(np.corrcoef(sc.va, sc.vc)[0, 1]) < 0.2 and np.all(sc.va != sc.vc)
    assert np.all(sc.va != 0.0) and np.all(sc.vc != 0.0)


@pytest.mark.parametrize("m", gc.WIDTHS)
def test_product_restatement_is_within_its_bound(m):
    sc = gc.sparse()
    X, out = gc.products(m)
    assert np.all(X != 0.0)
    worst = 0.0
    for k in range(3):
        for name, va in (("A", sc.va), ("C", sc.vc)):
            Yl, Bl = gc.spmm_longdouble(sc.rp, sc.ci, va, np.ascontiguousarray(X[:, gc.slot(m, k)]))
            bound = (sc.lengths[:, None] + 1) * gc.U64 * Bl
            err = np.abs(out[k, name].astype(np.longdouble) - Yl)
            assert np.all(err <= bound)
            worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0])))
            assert np.all(out[k, name][sc.lengths == 0] == 0.0) and not np.any(np.signbit(out[k, name][sc.lengths == 0]))
        assert not np.array_equal(out[k, "A"], out[k, "C"])
    print(f"\n[geneo steps] m = {m}: restated products, largest error / bound {worst:.3f}")
    # to first order a row of w entries can reach w / (w + 1) of its bound, a one-entry row (one rounding against 2 u |a x|) 1 / 2
    assert worst <= 27.0 / 28.0


@pytest.mark.parametrize("m", gc.WIDTHS)
def test_dense_references_are_within_their_bounds(m):
    d = gc.dense(m)
    Wb, Xb = d.S[:, gc.slot(m, 1)], d.AS[:, gc.slot(m, 0)]
    ratios = []
    for U, V in ((d.R, d.R), (Xb, Xb), (d.R, Wb)):                        # the three Gram call forms of the iteration
        G, B = gc.gram_ref(U, V)
        Gl, _ = gc.gram_ref(U, V, dtype=np.longdouble)
        ratios.append(float(np.max(np.abs(G - Gl) / (1e-13 * B + 1e-300))))
    rows = gc.sample_rows()
    for U in (d.S, d.AS, d.CS):                                          # the Rayleigh-Ritz rotation, both output blocks
        ref, bnd = gc.rotate_ref(U, d.Y)
        refl, _ = gc.rotate_ref(U, d.Y, rows=rows, dtype=np.longdouble)
        ratios.append(float(np.max(np.abs(ref[rows] - refl) / (1e-13 * bnd[rows]))))
    ref, bnd = gc.rotate_ref(d.S[:, gc.slot(m, 0)], d.G)                 # the orthogonalisation W - X G
    refl, _ = gc.rotate_ref(d.S[:, gc.slot(m, 0)], d.G, rows=rows, dtype=np.longdouble)
    out = Wb - ref
    outl = Wb[rows].astype(np.longdouble) - refl
    ratios.append(float(np.max(np.abs(out[rows] - outl) / (1e-13 * (np.abs(Wb[rows]) + bnd[rows])))))
    print(f"\n[geneo steps] m = {m}: float64 references against long double, error / bound: Gram {ratios[0]:.3f} {ratios[1]:.3f} {ratios[2]:.3f}, "
          f"rotation {ratios[3]:.3f} {ratios[4]:.3f} {ratios[5]:.3f}, orthogonalisation {ratios[6]:.3f}")
    assert max(ratios) < 0.5, ratios


def test_helper_references():
    n, m = 1000, 7
    mask = np.ones(n)
    mask[::3] = 0.0
    for seed in (0, 1, gc.GENEO_SEED_BASE):
        R = gc.random_block(n, m, seed, np.ones(n))
        assert R.min() >= -0.5 and R.max() < 0.5
        assert np.all(R.std(axis=0) > 0.25) and abs(R.mean()) < 0.02       # uniform: standard deviation 0.289
        assert len(np.unique(R)) == R.size
        Rm = gc.random_block(n, m, seed, mask)
        assert np.all(Rm[::3] == 0.0) and np.array_equal(Rm[1::3], R[1::3])
    assert not np.array_equal(gc.random_block(n, m, 0, mask), gc.random_block(n, m, 1, mask))
    # the first entry by hand: splitmix64(seed = 0) of t + 1 = 1
    z = 0x9E3779B97F4A7C15
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
    z ^= z >> 31
    assert gc.random_block(1, 1, 0, [1.0])[0, 0] == (z >> 11) / 2.0 ** 53 - 0.5
    # inverse square roots of the diagonals: the three special values give exactly 0.0
    G = gc.gram_diagonals(5, 6)
    s = gc.invsqrt_diag_ref(G)
    assert s[0, 0] == 0.0 and s[1, 5] == 0.0 and s[2, 3] == 0.0 and s[3, 1] == 0.5
    assert np.array_equal(s == 0.0, np.einsum("sjj->sj", G) <= 1e-300) and np.sum(s == 0.0) == 3 and np.all(np.isfinite(s))
    # residual and finalisation against a plain loop
    d = gc.dense(6)
    r = gc.residual_ref(d.mu, d.sub_of_row, d.AS[:, :6], d.CS[:, :6])
    i = 4099 + 5
    assert d.sub_of_row[i] == 1 and r[i, 2] == d.CS[i, 2] - d.mu[1, 2] * d.AS[i, 2]
    f = gc.finalize_ref(d.mu, d.sub_of_row, d.R, 4)
    assert f.shape == (4, d.n) and f[3, i] == d.mu[1, 3] * d.R[i, 3]
