"""-m gpu: the operator product on diagonal row blocks (k_spmv_dia behind ddm_op_apply / ddm_op_applyscaleadd) against the
CSR-stream product of the same matrix (CsrMatrix.mv / usmv, k_spmv_stream), on the matrices of tests/dia_cases.py: more than one
block, early block ends, CSR-stream blocks inside the launch, a row longer than the stream kernel's LDS stage, empty rows, stored
zeros, -0.0 in the matrix and in x.  Same products in the same order: torch.equal, no tolerance.  Once with the default layout
and once with DDM_SPMV_FORMAT=csr (read when the operator is created)."""
import numpy as np
import pytest

from tests.dia_cases import cases, vector

pytestmark = pytest.mark.gpu

CASES = cases()


def _bits(t):
    import torch
    return t.view(torch.int64)


@pytest.mark.parametrize("fmt", ["default", "csr"])
def test_operator_product_equals_csr_stream(ddm, monkeypatch, fmt):
    import torch
    if fmt == "csr":
        monkeypatch.setenv("DDM_SPMV_FORMAT", "csr")
    else:
        monkeypatch.delenv("DDM_SPMV_FORMAT", raising=False)
    ctx = ddm.torch_context(0)
    for name in sorted(CASES):
        M = CASES[name][0]
        n = M.shape[0]
        A = ddm.CsrMatrix(ctx, M)
        op = ddm.NonOverlappingOperator(ctx, A, None, np.ones(n, dtype=np.uint8))
        x = torch.as_tensor(vector(n, 21)).cuda()
        y_ref = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        y = y_ref.clone()
        A.mv(x, y_ref)
        op.apply(x, y)
        ctx.sync()
        assert torch.equal(_bits(y), _bits(y_ref)), (name, fmt)                 # bit patterns: the sign of a zero counts
        alpha = -0.75
        y0 = torch.as_tensor(vector(n, 22) + 1.0).cuda()
        t = torch.zeros(n, dtype=torch.float64, device="cuda")
        A.usmv(1.0, x, t)                                                       # t = 0 + 1.0 * (A x)
        ctx.sync()
        at = alpha * t                                                          # the operator's axpy: product rounded, then added
        z_ref = y0 + at
        z = y0.clone()
        op.applyscaleadd(alpha, x, z)
        ctx.sync()
        assert torch.equal(_bits(z), _bits(z_ref)), (name, fmt)
        del op, A
    ctx.close()
