"""Block CG (ddm_cg_solve_multi, m = 4) on two ranks that share one GPU through the callback exchange: the column-by-column halo
exchange through the unchanged alltoall callback and the K x m coarse all-reduce, against the single-rank block solve."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_two_rank_block_cg_matches_single_rank():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29587", os.path.join(ROOT, "tests", "mp_multi_rhs_worker.py")]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "MULTI_RANKS_OK 2" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
