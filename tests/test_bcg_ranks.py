"""Block CG (ddm_bcg_solve_multi, m = 4) on two ranks that share one GPU through the callback exchange -- the column-by-column halo
exchange, the K x m coarse all-reduce, the all-reduce of the 2 m^2 coupling entries and the one of m^2 + m -- against the single-rank
block solve: the same iteration counts and ranks of the coupling matrix, on every rank the same history, x within 1e-8 of its
largest entry per column."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_two_rank_block_cg_matches_single_rank():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29597", os.path.join(ROOT, "tests", "mp_bcg_worker.py")]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "BCG_RANKS_OK 2" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
