"""Block GMRES (ddm_bgmres_solve_multi, m = 4, restart 6) on two ranks that share one GPU through the callback exchange -- the
column-by-column halo exchange, the K x m coarse all-reduce, the all-reduces of the Gram matrices and of the two projections -- against
the single-rank block solve: the same iteration counts and cycle widths, on every rank the same history, x within 1e-8 of its largest
entry per column."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_two_rank_block_gmres_matches_single_rank():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29598", os.path.join(ROOT, "tests", "mp_bgmres_worker.py")]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "BGMRES_RANKS_OK 2" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
