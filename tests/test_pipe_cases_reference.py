"""CPU (-m "not gpu"): the cases of tests/pipe_cases.py reach the branches of the pipe schedule builder and kernel they exist for, and
the bit comparison that tests/test_gpu_pipe_shapes.py makes on the device would see a kernel that loses one operand there.

Per case, on what the host builder itself (pipe::build through tests/cpp/pipe_host_test.cpp, the device's default options: delta 24,
max_span 256, vote 1, pack_steps 64) makes of the oracle's factor:

  * every PRECONDITIONS predicate holds (without this a case can silently stop reaching its branch), the caps n <= 60 000 and
    1.5 M factor entries hold;
  * accepted cases: pipe::emulate -- the kernel's data flow on the tile stream: LDS result ring, position arrays, progress
    requirements -- writes the oracle's sequential solve into a NaN-filled x, bit for bit;
  * declined cases: rc 1 and the builder's reason.

Sensitivity, per accepted case and (sweep, entry-slot class, operand kind) of MUTATIONS: the harness zeroes one factor value of
that class in the tile stream before the emulation (an active lane, a real operand whose value in the solve is not zero).  The
result must then differ from the oracle's in the mutated row, nowhere outside the rows that depend on it (a difference can die out
further down: each dependant scales it by a multiplier below 1 and rounds), and must miss check (a) of the GPU test,
residual ratio <= C = 2 (w_L + w_U + 3), by a factor of 100 or more (measured: 10^10 .. 10^15 times C).

`test_trsv_cases_engines` records which cases of tests/trsv_cases.py the pipe builder takes (TRSV_CASES_ENGINE, which
tests/test_gpu_trsv_shapes.py asserts of F.engine() in pipe mode)."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import pipe_cases as pc
from tests import trsv_cases as tc

U64 = 2.0 ** -53


@pytest.mark.parametrize("name", pc.NAMES)
def test_case_reaches_its_branches_and_the_emulation_is_the_oracle(ddm, name):
    c = pc.case(name)
    r = pc.ref(name)
    s = pc.schedule(name)
    print(f"\n{name}: n = {c.n}, {c.nblocks} block(s), {c.entries} factor entries, w_L = {c.widths.wL}, w_U = {c.widths.wU}, C = {c.C}, expected engine {pc.EXPECT[name]}")
    assert c.M.has_sorted_indices and c.block_ptr[0] == 0 and c.block_ptr[-1] == c.n and (np.diff(c.block_ptr) > 0).all()
    assert c.n <= pc.MAX_N and c.entries <= pc.MAX_ENTRIES
    offsum = np.asarray(abs(c.M).sum(axis=1)).ravel() - np.abs(c.M.diagonal())
    assert name.startswith("tc_") or (np.abs(c.M.diagonal()) > offsum).all()   # strictly dominant (the cases taken from trsv_cases: as they are there)
    assert np.isfinite(r.lu).all() and all(np.isfinite(x).all() for x in r.x)
    if name in pc.DECLINES:
        print(f"  declined: {s.err}")
        assert s.rc == 1 and s.err == pc.DECLINES[name], (s.rc, s.err)
    else:
        assert s.rc == 0, (s.rc, s.err)
        print("  " + s.figures())
        assert s.st["rows"] == c.n and s.st["entries"] == c.entries == s.st["local"] + s.st["self_global"] + s.st["remote"]
        assert int(s.ops[:, :, :3].sum()) == c.entries and int(s.steps.sum()) == s.st["nstepsL"] + s.st["nstepsU"]
        assert np.array_equal(s.x, r.x[0])                        # same order of operations as the sequential solve
        ratio = tc.Residual(c.M, r.lu).ratio(r.d[0], r.x[0], U64)
        print(f"  oracle residual ratio {ratio:.2f} (C = {c.C})")
        assert ratio <= c.C
    failed = [what for what, holds in pc.PRECONDITIONS[name] if not holds(c, s)]
    assert not failed, failed


@pytest.mark.parametrize("name", pc.ACCEPTED)
def test_one_lost_operand_is_seen(ddm, name):
    c = pc.case(name)
    r = pc.ref(name)
    res = tc.Residual(c.M, r.lu)
    for sweep, slot, kind in pc.MUTATIONS[name]:
        s = pc.run_builder(c.M, c.block_ptr, r.lu, r.diag, r.d[0], mutate=(sweep, slot, kind))
        m = s.mutation
        what = f"{name}: {'LU'[sweep]} sweep, entry slots {pc.CLASS_NAMES[slot]}, {pc.KIND_NAMES[kind] if kind >= 0 else 'any'} operand"
        assert s.rc == 0 and m["row"] >= 0, (what, "no such operand in the schedule", s.err)
        assert (slot, kind) == (0 if m["slot"] < 14 else (1 if m["slot"] < 20 else 2), m["kind"] if kind >= 0 else kind), (what, m)
        differ = s.x != r.x[0]
        dep = pc.dependants(c.M, m["row"], sweep)
        ratio = res.ratio(r.d[0], s.x, U64)
        print(f"\n{what}: row {m['row']} (task {m['task']}, step {m['step']}, lane {m['lane']}, entry {m['slot']}, {pc.KIND_NAMES[m['kind']]}): "
              f"{int(differ.sum())} entries differ, {int(dep.sum())} rows depend on it; residual ratio {ratio:.2e} = {ratio / c.C:.2e} C")
        assert differ[m["row"]], what
        assert not (differ & ~dep).any(), (what, np.flatnonzero(differ & ~dep)[:8])
        assert ratio >= 100 * c.C, (what, ratio, c.C)


def test_sixteen_bit_step_cap():
    """a single chain of 65 537 rows: one task of more steps than a 16-bit progress requirement holds (CPU only: the factor never
    reaches the device as a pipe schedule)"""
    n = 65537
    M = pc.band(n, (1,), 46)
    f, lu, diag = pc.oracle_factor(M)
    s = pc.run_builder(M, [0, n], lu, diag, np.ones(n))
    assert s.rc == 1 and s.err == pc.STEPS16, (s.rc, s.err)


@pytest.mark.parametrize("name", tc.NAMES)
def test_trsv_cases_engines(ddm, name):
    """which cases of tests/trsv_cases.py the pipe builder takes with the device's options"""
    c = tc.case(name)
    f, lu, diag = pc.oracle_factor(sp.csr_matrix(c.M))
    d = np.random.default_rng(2).standard_normal(c.n)
    s = pc.run_builder(c.M, c.block_ptr, lu, diag, d)
    print(f"\n{name}: " + (s.figures() if s.rc == 0 else f"declined: {s.err}"))
    assert ("pipe" if s.rc == 0 else "xcd2") == pc.TRSV_CASES_ENGINE[name], (s.rc, s.err)
    assert s.rc != 1 or s.err == pc.WIDE
    if s.rc == 0:
        assert np.array_equal(s.x, pc.oracle_solve(f, d))
