"""-m gpu: the operator product on coded blocks (the fourth branch of k_spmv_dia behind ddm_op_apply: a dictionary of 16 doubles
per block in LDS, a 16-byte word of 4-bit codes per row) on the matrices of tests/dia_code_cases.py, against the CSR-stream
product (an operator created with DDM_SPMV_FORMAT=csr) and against the slab branches (DDM_SPMV_CODE=0): constant-coefficient
boxes coded throughout, with a last block of 40 rows and a block that ends at a decoupling row; a block on exactly 16 values next
to one on 17 in one segment; +0.0 and -0.0 in one dictionary; a stored 0.0 next to an absent entry under a NaN in x; all 32
diagonals; random values (nothing coded).  x holds -0.0 and, in one case, +-inf and NaN at rows that only some blocks read.  The same
doubles multiplied in the same order: torch.equal on the bit patterns, no tolerance.  The switches are read when the operator is
created."""
import numpy as np
import pytest

from tests.dia_cases import vector
from tests.dia_code_cases import code_cases

pytestmark = pytest.mark.gpu


def _bits(t):
    import torch
    return t.view(torch.int64)


def test_coded_product_equals_csr_stream_and_slabs(ddm, monkeypatch):
    import torch
    monkeypatch.delenv("DDM_SPMV_STAGE_X", raising=False)
    cases = code_cases()
    ctx = ddm.torch_context(0)
    for name in sorted(cases):
        M, x_host, expected = cases[name]
        n = M.shape[0]
        monkeypatch.delenv("DDM_SPMV_CODE", raising=False)
        info = ddm.dia_codes_host(M, arrays=False)                              # the layout under test is the one the case was made for
        if expected is not None:
            assert info["entries"].tolist() == [e for _, _, e in expected], name
        else:
            assert info["coded"].all(), name
        A = ddm.CsrMatrix(ctx, M)
        owner = np.ones(n, dtype=np.uint8)
        ops = {}
        for kind, var, value in (("coded", None, None), ("slabs", "DDM_SPMV_CODE", "0"), ("csr", "DDM_SPMV_FORMAT", "csr")):
            if var:
                monkeypatch.setenv(var, value)
            ops[kind] = ddm.NonOverlappingOperator(ctx, A, None, owner)
            if var:
                monkeypatch.delenv(var)
        x = torch.as_tensor(vector(n, 21) if x_host is None else x_host).cuda()
        y = {kind: torch.full((n,), float("nan"), dtype=torch.float64, device="cuda") for kind in ops}
        for kind, op in ops.items():
            op.apply(x, y[kind])
        ctx.sync()
        assert torch.equal(_bits(y["coded"]), _bits(y["csr"])), name            # bit patterns: the sign of a zero counts
        assert torch.equal(_bits(y["coded"]), _bits(y["slabs"])), name
        if x_host is not None and np.isnan(x_host).any():
            assert bool(torch.isnan(y["coded"]).any()) and bool(torch.isfinite(y["coded"]).any()), name
        alpha = -0.75                                                           # the operator's axpy on top of the coded product
        y0 = torch.as_tensor(vector(n, 22) + 1.0).cuda()
        z = {kind: y0.clone() for kind in ("coded", "csr")}
        for kind in z:
            ops[kind].applyscaleadd(alpha, x, z[kind])
        ctx.sync()
        assert torch.equal(_bits(z["coded"]), _bits(z["csr"])), name
        del ops, A
    ctx.close()
