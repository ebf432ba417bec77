"""Dune::HipBiCGSTABSolver::apply_queue (std::vector<X> of right-hand sides through a block of fixed width ->
ddm_bicgstab_solve_queue; apply_queue itself sits in the base class of the device Krylov solvers) compiled against the mock DUNE
headers (tests/cpp/mock) with the flags of tests/cpp/Makefile, and run against TwoLevelSchwarz.solve_many(solver="bicgstabsolver") on
the same problem and columns."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
XTOL = 1e-8          # x of a block column against another solve of it (tests/test_gpu_multi_rhs.py)


def _compile(out_dir):
    exe = os.path.join(str(out_dir), "bicgstab_queue_adaptor")
    cmd = ["g++", "-std=c++20", "-O2", "-Wall", "-DDUNE_DDM_HAVE_TASKFLOW=1", "-I" + os.path.join(CPP, "mock"), "-I" + os.path.join(ROOT, "dune-ddm_amd"),
           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(CPP, "bicgstab_queue_adaptor.cc"), "-L" + os.path.join(ROOT, "dune-ddm_amd"), "-lddm_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "dune-ddm_amd"), "-Wl,-rpath,/opt/rocm/lib"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    return exe


def test_bicgstab_queue_adaptor_compiles_and_links(ddm, tmp_path):
    ddm.load_library()
    exe = _compile(tmp_path)
    out = subprocess.run(["nm", "-D", "--undefined-only", exe], capture_output=True, text=True).stdout
    used = sorted({ln.split()[-1] for ln in out.splitlines() if " ddm_" in ln})
    assert "ddm_bicgstab_solve_queue" in used and all(u in ddm.SYMBOLS for u in used), used


@pytest.mark.gpu
def test_bicgstab_queue_adaptor_matches_solve_many(ddm, tmp_path):
    """M = 9 columns through w = 4 slots, multiplicative combination: iteration counts equal those of solve_many on the same columns, x
    within 1e-8 of the largest entry; the adaptor leaves b as it was, refuses an empty column list and a width of 33, and
    HipRestartedGMResSolver::apply_queue throws Dune::NotImplemented."""
    from dune_ddm_amd import synth
    from dune_ddm_amd.problem import build_structured
    from dune_ddm_amd.solver import TwoLevelSchwarz
    M, w = 9, 4
    exe = _compile(tmp_path)
    dec = build_structured(synth.StructuredPoisson((14, 13, 12), (1, 1, 1)), overlap=1, pou_type="distance")
    sd = dec.subs[0]
    A = sd.A.tocsr()
    np.asarray(A.indptr, dtype=np.int64).tofile(tmp_path / "rowptr.bin")
    np.asarray(A.indices, dtype=np.int32).tofile(tmp_path / "col.bin")
    np.asarray(A.data, dtype=np.float64).tofile(tmp_path / "val.bin")
    sd.dirichlet_ovlp.astype(np.uint8).tofile(tmp_path / "dirichlet.bin")
    sd.pou.astype(np.float64).tofile(tmp_path / "pou.bin")
    # right-hand sides: seeded random ones that are zero on the Dirichlet rows (not the problem's own: the load vector of f = 1 is a
    # genuine BiCGSTAB breakdown under the multiplicative combination, tests/test_gpu_parity.py)
    B = np.ascontiguousarray(np.random.default_rng(12345).standard_normal((sd.n, M)) * (sd.dirichlet_ovlp == 0)[:, None])
    B.tofile(tmp_path / "rhs.bin")
    p = subprocess.run([exe, str(tmp_path), str(M), str(w)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "queue_ok" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    assert "b_unchanged 1" in p.stdout and "errors_caught 3" in p.stdout
    cols = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("col ")]
    assert len(cols) == M
    Xc = np.fromfile(tmp_path / "x_queue.bin", dtype=np.float64).reshape(sd.n, M)
    tl = TwoLevelSchwarz(dec, coarse="pou", schwarz_type="standard", mode="multiplicative")
    assert tl.rl.n_o == sd.n
    res, _, X = tl.solve_many(B, width=w, reduction=1e-9, maxit=200, solver="bicgstabsolver")
    Xh = X.cpu().numpy()
    for j in range(M):
        assert int(cols[j][2]) == res[j].iterations and cols[j][3] == "1" and res[j].converged == 1, (j, cols[j], res[j].iterations)
        assert np.max(np.abs(Xc[:, j] - Xh[:, j])) <= XTOL * np.max(np.abs(Xh[:, j])), j
    tl.ctx.close()
