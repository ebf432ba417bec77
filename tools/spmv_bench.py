"""Times CsrMatrix.mv (k_spmv_stream) and, next to it, the operator path NonOverlappingOperator.apply (k_spmv_dia on diagonal row
blocks, or k_spmv_stream again under DDM_SPMV_FORMAT=csr) on a 27-point stencil matrix of N^3 rows (diagnostic).
usage: python tools/spmv_bench.py [N]"""
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ddm = ge.import_package()
import torch  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 216
T = sp.diags([np.ones(N - 1), 2.0 * np.ones(N), np.ones(N - 1)], [-1, 0, 1], format="csr")
t0 = time.time()
M = sp.kron(T, sp.kron(T, T, format="csr"), format="csr")
M.sort_indices()
print(f"matrix {M.shape[0]} rows {M.nnz} nnz built in {time.time() - t0:.1f}s", flush=True)
ctx = ddm.torch_context(0)
A = ddm.CsrMatrix(ctx, M)
x = torch.as_tensor(np.random.default_rng(0).standard_normal(M.shape[0])).cuda()
y = torch.zeros_like(x)
op = ddm.NonOverlappingOperator(ctx, A, None, np.ones(M.shape[0], dtype=np.uint8))
yo = torch.zeros_like(x)
reps = 30


def timed(f):
    for _ in range(5):
        f()
    ctx.sync()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


ms = timed(lambda: A.mv(x, y))
ms_op = timed(lambda: op.apply(x, yo))
staged = "x windows in LDS" if os.environ.get("DDM_SPMV_STAGE_X") != "0" else "x per diagonal (DDM_SPMV_STAGE_X=0)"
print(f"operator apply ({os.environ.get('DDM_SPMV_FORMAT', 'diagonal blocks, ' + staged)}) {ms_op:.4f} ms bit-equal to CsrMatrix.mv: {torch.equal(y.view(torch.int64), yo.view(torch.int64))}")
ref = M @ x.cpu().numpy()
err = np.abs(y.cpu().numpy() - ref).max() / np.abs(ref).max()
print(f"spmv {ms:.4f} ms  {12.0 * M.nnz / ms / 1e6:.1f} GB/s (12 B per non-zero)  max rel dev vs scipy {err:.2e}")
ctx.close()
