"""-m gpu: the operator product with the x windows of a block staged in LDS (k_spmv_dia behind ddm_op_apply /
ddm_op_applyscaleadd) against the CSR-stream product of the same matrix (CsrMatrix.mv / usmv, k_spmv_stream), on the matrices of
tests/dia_cases.py and tests/dia_window_cases.py: one, two and three runs, the merge rule at its boundary, windows that exactly
fill the LDS array and one diagonal more (unstaged), half and full storage, CSR-stream and staged blocks in one launch, windows
clamped at both ends of the vector, non-finite x next to an absent entry.  Same products in the same order: torch.equal on the bit
patterns, no tolerance.  Once with the default and once with DDM_SPMV_STAGE_X=0 (read when the operator is created)."""
import numpy as np
import pytest

from tests.dia_cases import cases, vector
from tests.dia_window_cases import window_cases

pytestmark = pytest.mark.gpu

WG = 256


def _bits(t):
    import torch
    return t.view(torch.int64)


@pytest.mark.parametrize("stage", ["default", "0"])
def test_operator_product_equals_csr_stream(ddm, monkeypatch, stage):
    import torch
    if stage == "0":
        monkeypatch.setenv("DDM_SPMV_STAGE_X", "0")
    else:
        monkeypatch.delenv("DDM_SPMV_STAGE_X", raising=False)
    monkeypatch.delenv("DDM_SPMV_FORMAT", raising=False)
    _, capacity = ddm.dia_windows_host(cases()["one_by_one"][0])
    all_cases = {**{name: (M, None, None) for name, (M, _) in cases().items()}, **window_cases(capacity, WG)}
    ctx = ddm.torch_context(0)
    for name in sorted(all_cases):
        M, x_host, expected = all_cases[name]
        n = M.shape[0]
        if expected is not None:                                                # the layout under test is the one the case was made for
            segs, _ = ddm.dia_windows_host(M)
            assert [s["staged"] for s in segs] == [st and stage == "default" for st, _, _ in expected], (name, stage)
        A = ddm.CsrMatrix(ctx, M)
        op = ddm.NonOverlappingOperator(ctx, A, None, np.ones(n, dtype=np.uint8))
        x = torch.as_tensor(vector(n, 21) if x_host is None else x_host).cuda()
        y_ref = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        y = y_ref.clone()
        A.mv(x, y_ref)
        op.apply(x, y)
        ctx.sync()
        assert torch.equal(_bits(y), _bits(y_ref)), (name, stage)               # bit patterns: the sign of a zero counts
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
        assert torch.equal(_bits(z), _bits(z_ref)), (name, stage)
        del op, A
    ctx.close()
