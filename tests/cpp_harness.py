"""What the tests/test_cpp_*.py modules share: building one program of tests/cpp through its Makefile (the one place the compile line
lives), the check of the C-ABI symbols a binary uses, the dump of a one-rank problem in the layout tests/cpp/adaptor_fixture.hh reads,
and the run of a program as a fresh child process."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def build(name):
    """make -C tests/cpp <name>: recompiles only when a source or header changed.  Returns the path of the binary (of the file itself
    for a target with a suffix, e.g. mpi_exchange_check.o)."""
    p = subprocess.run(["make", "-C", CPP, name], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    return os.path.join(CPP, name if "." in name else os.path.join("build", name))


def ddm_symbols_used(exe):
    """The undefined ddm_* symbols of a binary, sorted."""
    out = subprocess.run(["nm", "-D", "--undefined-only", exe], capture_output=True, text=True).stdout
    return sorted({ln.split()[-1] for ln in out.splitlines() if " ddm_" in ln})


def dump_csr(path, M, prefix=""):
    M = M.tocsr()
    np.asarray(M.indptr, dtype=np.int64).tofile(path / f"{prefix}rowptr.bin")
    np.asarray(M.indices, dtype=np.int32).tofile(path / f"{prefix}col.bin")
    np.asarray(M.data, dtype=np.float64).tofile(path / f"{prefix}val.bin")


def dump_one_rank_problem(path, sd, b=True):
    dump_csr(path, sd.A)
    if b:
        sd.b.astype(np.float64).tofile(path / "b.bin")
    sd.dirichlet_ovlp.astype(np.uint8).tofile(path / "dirichlet.bin")
    sd.pou.astype(np.float64).tofile(path / "pou.bin")


def run(exe, *args, env=None, timeout=300):
    p = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=timeout, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return p
