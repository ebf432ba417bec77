"""CPU: the host twins of the kept GenEO eigensolver's pencil (ddm_geneo_pencil_host, ddm_geneo_pencil_refresh_host) and the inputs of
tests/test_gpu_geneo_refresh.py.  The pencil refreshed through the origin map must be, byte for byte, the pencil assembled on the new
values, and both a numpy statement of the formula in the same operation order; the oracle margins the GPU tests rely on are proved
here, where no GPU is needed."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import geneo_refresh_cases as gc


def _same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _check(ddm, A0, B0, A1, B1, pou, dm, sigma):
    rp, ci, vt0, vc0, org = ddm.geneo_pencil_host(A0, B0, pou, dm, sigma)
    rp1, ci1, vt1, vc1, org1 = ddm.geneo_pencil_host(A1, B1, pou, dm, sigma)
    assert _same_bytes(rp, rp1) and _same_bytes(ci, ci1) and _same_bytes(org, org1)          # same patterns, same map
    vt, vc = ddm.geneo_pencil_refresh_host(rp, ci, org, A1, B1, pou, dm, sigma)
    assert _same_bytes(vt, vt1) and _same_bytes(vc, vc1)                                     # refreshed == assembled anew
    nrp, nci, nvt, nvc = gc.pencil_numpy(A1, B1, pou, dm, sigma)
    assert _same_bytes(rp, nrp) and _same_bytes(ci, nci)
    assert _same_bytes(vt1, nvt) and _same_bytes(vc1, nvc)                                   # == the formula
    vtb, vcb = ddm.geneo_pencil_refresh_host(rp, ci, org, A0, B0, pou, dm, sigma)            # and back
    assert _same_bytes(vtb, vt0) and _same_bytes(vcb, vc0)
    assert not _same_bytes(vt0, vt1)
    # the map: every entry comes from A, from B or from both, at the offset it says
    A0, B0 = sp.csr_matrix(A0), sp.csr_matrix(B0)
    oa, ob = (org & 0xffff).astype(np.int64), (org >> 16).astype(np.int64)
    assert ((oa > 0) | (ob > 0)).all()
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    ia = A0.indptr[rows] + oa - 1
    ib = B0.indptr[rows] + ob - 1
    assert (A0.indices[ia[oa > 0]] == ci[oa > 0]).all() and (B0.indices[ib[ob > 0]] == ci[ob > 0]).all()
    assert (oa > 0).sum() == A0.nnz and (ob > 0).sum() == B0.nnz
    return rp, org


@pytest.mark.parametrize("name", ["B_inside_A", "A_inside_B", "dirichlet_rows_only_in_B", "long_row"])
def test_built_pencils(ddm, name):
    A0, B0, A1, B1, pou, dm = gc.pencil_cases()[name]
    rp, org = _check(ddm, A0, B0, A1, B1, pou, dm, 0.37)
    oa, ob = org & 0xffff, org >> 16
    if name == "B_inside_A":
        assert (oa > 0).all() and (ob == 0).any()
    if name == "A_inside_B":
        assert (ob > 0).all() and (oa == 0).any()
    if name == "dirichlet_rows_only_in_B":
        for r in (3, 17, 30):
            assert A0.indptr[r + 1] == A0.indptr[r] and rp[r + 1] > rp[r] and dm[r]
            assert (oa[rp[r]:rp[r + 1]] == 0).all()
    if name == "long_row":
        lens = np.diff(rp)
        assert lens.max() > 64 and (lens == 1).sum() > 100


def test_islands_problem_pencil(ddm):
    A0, B0, pou, dm = gc.block_pencil_input("old")
    A1, B1, pou1, dm1 = gc.block_pencil_input("new")
    assert np.array_equal(pou, pou1) and np.array_equal(dm, dm1)
    _check(ddm, A0, B0, A1, B1, pou, dm, gc.SHIFT)


def test_islands_problem_margins():
    """What the GPU tests take for granted: the patterns are kept by the new coefficient in all eight subdomains, B_neu is a matrix of
    its own, the four wanted eigenvalues stay below 1 - 1e-6 on either set of values (no decoupled unit mode among them), and the gap
    behind the fourth is at least 0.08 everywhere -- so the criteria of tests/test_gpu_geneo.py (eigenvalues rtol 1e-6, sine of the
    largest angle < 2e-3: eigenvector error ~ tolerance / gap) apply unchanged."""
    old, new = gc.decomposition("old"), gc.decomposition("new")
    assert len(old.subs) == 8
    for a, b in zip(old.subs, new.subs):
        for Ma, Mb in ((a.A_neu, b.A_neu), (a.B_neu, b.B_neu)):
            Ma, Mb = sp.csr_matrix(Ma).sorted_indices(), sp.csr_matrix(Mb).sorted_indices()
            assert np.array_equal(Ma.indptr, Mb.indptr) and np.array_equal(Ma.indices, Mb.indices)
            assert not np.array_equal(Ma.data, Mb.data)
        assert a.B_neu is not a.A_neu and (sp.csr_matrix(a.A_neu) - sp.csr_matrix(a.B_neu)).nnz > 0
        assert np.array_equal(a.pou, b.pou) and np.array_equal(a.dirichlet_ovlp, b.dirichlet_ovlp)
    import scipy.sparse.linalg as spl
    largest = 0.0
    for which in ("old", "new"):
        dec = gc.decomposition(which)
        wanted = gc.oracle(which)
        for sd in dec.subs:
            lam = wanted[sd.id][1]
            assert len(lam) == gc.NEV and lam.max() < 1.0 - 1e-6
            largest = max(largest, float(lam.max()))
            # the gap behind the fourth, in the pencil the library iterates on: C~ = D B D WITHOUT the rows / columns of Dirichlet DoFs
            # (their decoupled unit modes lambda = 1 / pou^2 >= 1, which the oracle's nev = 5 would return, are deflated: DESIGN 5)
            free = (sd.dirichlet_ovlp == 0).astype(float)
            D = sp.diags(sd.pou * free)
            C = (D @ sp.csr_matrix(sd.B_neu) @ D).tocsc()
            At = (sp.csr_matrix(sd.A_neu) + gc.SHIFT * C).tocsc()
            mu = spl.eigsh(C, k=gc.NEV + 1, M=At, which="LA", tol=1e-10, return_eigenvectors=False)
            lam5 = np.sort(1.0 / mu - gc.SHIFT)
            assert np.allclose(lam5[:gc.NEV], lam, rtol=1e-6)
            assert lam5[gc.NEV] - lam5[gc.NEV - 1] >= 0.08, (which, sd.id, lam5)
    assert largest < 0.93
    # threshold mode on the new values: the subdomains keep different numbers of vectors (so a doubling is needed)
    counts = [len(v[0]) for v in gc.oracle("new", threshold=True).values()]
    assert min(counts) >= 1 and max(counts) <= 8
