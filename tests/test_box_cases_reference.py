"""CPU (-m "not gpu"): the cases of tests/box_cases.py reach the branches of the box builder and kernel they exist for, and the checks
that tests/test_gpu_box_shapes.py makes on the device would see a kernel that loses one operand there.

Per case, on what the host builder itself (box::build through tests/cpp/box_host_test.cpp: box_test_case) makes of the oracle's factor:

  * every PRECONDITIONS predicate holds (without this a case can silently stop reaching its branch), the caps n <= 60 000 and
    1.5 M factor entries hold; printed: the dimensions, the histogram of shell entries per box row, planes given back;
  * accepted cases: box::emulate (rows in the order of the device kernels) and box::emulate_lanes (the kernel's index arithmetic:
    lane = J mod 64, register windows, two-slot neighbour ring, position-ordered hand-over, ten two-double product slots) write the
    oracle's sequential solve into a NaN-filled x, bit for bit, and the oracle's own residual ratio is <= C = 2 (w_L + w_U + 3);
    the nested factor ends on NESTED[name] (the pipe builder's verdict on the shell system);
  * declined cases: rc 1, exactly the recorded reason, and the pipe builder's verdict on the whole matrix is EXPECT[name].

Sensitivity, per accepted case and (sweep, value slot, lines) of MUTATIONS: the harness zeroes one stream value -- entry e = 0 .. 12,
the stored inverse pivot -- or one product (slots q < 7 / q >= 7) of a row whose value there is not zero, before the lane-by-lane walk.
The result must then differ from the oracle's in the mutated row, nowhere outside the rows that depend on it, and must miss check (a)
of the GPU test, residual ratio <= C, by a factor of 100 or more (measured: 2.9 10^10 .. 6.9 10^14 times C; the smallest is a
previous-plane entry of the upper sweep on shrink20)."""
import numpy as np
import pytest

from tests import box_cases as bc
from tests import pipe_cases as pc
from tests import trsv_cases as tc

U64 = 2.0 ** -53


@pytest.mark.parametrize("name", bc.NAMES)
def test_case_reaches_its_branches_and_the_emulation_is_the_oracle(ddm, name):
    c = bc.case(name)
    r = bc.ref(name)
    s = bc.built(name)
    print(f"\n{name}: n = {c.n}, {c.nblocks} block(s), {c.entries} factor entries, w_L = {c.widths.wL}, w_U = {c.widths.wU}, C = {c.C}, expected engine {bc.EXPECT[name]}")
    assert c.M.has_sorted_indices and c.block_ptr[0] == 0 and c.block_ptr[-1] == c.n and (np.diff(c.block_ptr) > 0).all()
    assert c.n <= bc.MAX_N and c.entries <= bc.MAX_ENTRIES
    assert ((c.M != 0) != (c.M != 0).T).nnz == 0               # symmetric pattern
    offsum = np.asarray(abs(c.M).sum(axis=1)).ravel() - np.abs(c.M.diagonal())
    assert (np.abs(c.M.diagonal()) > offsum).all()             # strictly dominant
    assert np.isfinite(r.lu).all() and all(np.isfinite(x).all() for x in r.x)
    if name in bc.DECLINES:
        print(f"  declined: {s.err}")
        assert s.rc == 1 and s.err == bc.DECLINES[name], (s.rc, s.err)
        p = pc.run_builder(c.M, c.block_ptr, r.lu, r.diag, r.d[0])   # what settle_engine hands the matrix to
        print("  pipe builder: " + ("accepted" if p.rc == 0 else f"declined: {p.err}"))
        assert ("pipe" if p.rc == 0 else "xcd2") == bc.EXPECT[name], (p.rc, p.err)
        assert p.rc == 0 or p.err == pc.WIDE
    else:
        assert s.rc == 0, (s.rc, s.err)
        print("  " + s.figures())
        print(f"  product slots {s.st['ext_products']}, stream bytes {s.st['stream_bytes']}, nested factor: {s.st['nested_entries']} entries, widest triangle row {s.st['nested_widest']}; "
              f"turns past the last step {sorted(bc.turns_past(s))}")
        assert bc.EXPECT[name] == "box"
        assert s.st["box_rows"] + s.st["shell_rows"] == c.n and s.st["shell_rows"] == sum(B.shell for B in s.blocks)
        assert all(int(B.hist.sum()) == B.nx * B.ny * B.nz and B.nsteps == B.nx + 2 * (B.ny - 1) for B in s.blocks)
        assert np.array_equal(s.x, r.x[0])                        # same order of operations as the sequential solve
        ratio = tc.Residual(c.M, r.lu).ratio(r.d[0], r.x[0], U64)
        print(f"  oracle residual ratio {ratio:.2f} (C = {c.C})")
        assert ratio <= c.C
        sh = bc.shell_system(c.M, c.block_ptr, r.lu, r.diag)
        if sh is None:
            assert bc.NESTED[name] is None
        else:
            Ms, fbp, fdiag = sh
            p = pc.run_builder(Ms, fbp, Ms.data, fdiag, np.ones(Ms.shape[0]))
            print("  nested factor, pipe builder: " + ("accepted" if p.rc == 0 else f"declined: {p.err}"))
            assert ("pipe" if p.rc == 0 else "xcd2") == bc.NESTED[name], (p.rc, p.err)
    failed = [what for what, holds in bc.PRECONDITIONS[name] if not holds(c, s)]
    assert not failed, failed


def test_the_table_as_a_whole(ddm):
    """across the accepted cases the three-turn step loop ends with zero, one and two turns past the last step, and every count of
    shell entries 0 .. 20 and every number of lines per lane 1, 2, 3 and 8 occurs"""
    turns, lines, counts = set(), set(), np.zeros(21, dtype=np.int64)
    for name in bc.ACCEPTED:
        s = bc.built(name)
        turns |= bc.turns_past(s)
        lines |= {B.lines for B in s.blocks}
        counts += sum(B.hist for B in s.blocks)
    assert turns == {0, 1, 2} and {1, 2, 3, 8} <= lines and (counts > 0).all(), (turns, lines, counts)
    # the mutations the table must hold: a product in slots q >= 7 on ext20, a previous-plane operand (L: e = 0 .. 8) on tall70, a
    # line-(J - 1) operand (L: e = 9 .. 11) of lane 0's second line (J = 64) on ny65
    assert any(m[:2] == (bc.U, bc.PRODUCT_HIGH) for m in bc.MUTATIONS["ext20"])
    assert any(m[0] == bc.L and 0 <= m[1] <= 8 for m in bc.MUTATIONS["tall70"])
    assert any(m[0] == bc.L and 9 <= m[1] <= 11 and m[2:] == (64, 64) for m in bc.MUTATIONS["ny65"])
    assert set(bc.TAIL) | set(bc.CHAINED) <= set(bc.ACCEPTED)


@pytest.mark.parametrize("name", bc.ACCEPTED)
def test_one_lost_value_is_seen(ddm, name):
    c = bc.case(name)
    r = bc.ref(name)
    res = tc.Residual(c.M, r.lu)
    for sweep, e, jmin, jmax in bc.MUTATIONS[name]:
        s = bc.run_builder(c.M, c.block_ptr, r.lu, r.diag, r.d[0], mutate=(sweep, e, jmin, jmax))
        m = s.mutation
        kind = {bc.PIVOT: "inverse pivot", bc.PRODUCT_LOW: "product in slots q < 7", bc.PRODUCT_HIGH: "product in slots q >= 7"}.get(e, f"entry {e}")
        what = f"{name}: {'LU'[sweep]} sweep, {kind}, lines {jmin} .. {min(jmax, 9999)}"
        assert s.rc == 0 and m["row"] >= 0, (what, s.rc, s.err)
        assert m["product"] == (e < 0) and (e >= 0 or (m["slot"] // 2 >= 7) == (e == bc.PRODUCT_HIGH)), (what, m)
        differ = ~((s.x == r.x[0]) | (np.isnan(s.x) & np.isnan(r.x[0])))
        dep = pc.dependants(c.M, m["row"], sweep)
        ratio = res.ratio(r.d[0], s.x, U64)
        print(f"\n{what}: row {m['row']} (block {m['block']}, plane {m['plane']}, step {m['step']}, lane {m['lane']}, slot {m['slot']}): "
              f"{int(differ.sum())} entries differ, {int(dep.sum())} rows depend on it; residual ratio {ratio:.2e} = {ratio / c.C:.2e} C")
        assert not np.isnan(s.x).any(), what
        assert differ[m["row"]], what
        assert not (differ & ~dep).any(), (what, np.flatnonzero(differ & ~dep)[:8])
        assert ratio >= 100 * c.C, (what, ratio, c.C)
