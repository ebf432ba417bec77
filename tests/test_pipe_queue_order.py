"""Queue order of the pipe schedule (dune-ddm_amd/csrc/trsv_pipe_host.hpp, "Queue order"): tasks that the creation order leaves far
behind their start level are queued in front of some of their producers.  Checked on the CPU with the slot-limited emulation of
the device data flow: bit-exact against the oracle's sequential ILU(0) solve with as few workgroups per queue as the builder's
argument allows (moved tasks + 1) and with more, the detector of a deadlocking order, and the creation order with nothing moved.
No GPU needed; the GPU test (tests/test_gpu_pipe_queue.py) runs the orders accepted here."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from tests import pipe_cases as pc

CPP = pc.CPP
DELTA, GAP, MOVE_MAX = 24, 24, 32                                # pipe::Options defaults / the bound of the benchmark's launch


@functools.lru_cache(maxsize=None)
def harness():
    """tests/cpp/pipe_queue_test.cpp with the flags of the libpipe_host_test.so line of tests/cpp/Makefile"""
    out = os.path.join(CPP, "build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libpipe_queue_test.so")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-O2", "-Wall", "-fPIC", "-ffp-contract=off", "-shared",
                           "-I" + os.path.join(pc.ROOT, "dune-ddm_amd", "csrc"), "-o", so, os.path.join(CPP, "pipe_queue_test.cpp"), "-lpthread"])
    lib = ctypes.CDLL(so)
    lib.pipe_queue_case.restype = ctypes.c_int
    lib.pipe_queue_same_tasks.restype = ctypes.c_int
    return lib


class Problem:
    """a block-diagonal matrix, its oracle factor, one right-hand side and the oracle's solve of it (computed once, shared)"""

    def __init__(self, M, block_ptr, seed=3):
        self.M = sp.csr_matrix(M)
        self.M.sort_indices()
        self.bp = np.asarray(block_ptr, dtype=np.int64)
        self.n = self.M.shape[0]
        f, lu, diag = pc.oracle_factor(self.M)
        self.lu = np.ascontiguousarray(lu, dtype=np.float64)
        self.diag = np.ascontiguousarray(diag, dtype=np.int64)
        self.d = np.random.default_rng(seed).standard_normal(self.n)
        self.x_ref = pc.oracle_solve(f, self.d)
        self.rp = np.asarray(self.M.indptr, dtype=np.int64)
        self.ci = np.asarray(self.M.indices, dtype=np.int32)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def run(pb, slots=0, move_max=MOVE_MAX, gap=GAP, delta=DELTA):
    x = np.full(pb.n, np.nan)
    out = np.zeros(8, dtype=np.int64)
    info = np.zeros((4096, 4), dtype=np.int32)
    err = ctypes.create_string_buffer(256)
    rc = harness().pipe_queue_case(ctypes.c_int64(pb.n), _p(pb.rp), _p(pb.ci), _p(pb.lu), _p(pb.diag), ctypes.c_int(len(pb.bp) - 1), _p(pb.bp),
                                   ctypes.c_int(delta), ctypes.c_int(gap), ctypes.c_int(move_max), ctypes.c_int(slots), _p(pb.d), _p(x), _p(out),
                                   _p(info), ctypes.c_int64(len(info)), err, 256)
    names = ("movedL", "movedU", "max_moved", "ntasks", "in_front", "in_front_unflagged", "foreign_producers", "stream_bytes")
    st = dict(zip(names, out.tolist()))
    assert st["ntasks"] <= len(info)
    return rc, err.value.decode(), x, st, info[:st["ntasks"]]


def _subdomains(N, P, which=None):
    from dune_ddm_amd import synth
    from dune_ddm_amd.problem import build_structured
    dec = build_structured(synth.StructuredPoisson(N, P), overlap=2, pou_type="distance", shrink=0)
    mats = [dec.subs[k].A_dir.tocsr() for k in (range(len(dec.subs)) if which is None else which)]
    return sp.block_diag(mats, format="csr"), np.concatenate([[0], np.cumsum([m.shape[0] for m in mats])])


@functools.lru_cache(maxsize=None)
def corner_subdomains():
    """subdomains 0 and 7 of 64^3 / 2x2x2, overlap 2: the overlap shell on the far / on the near faces"""
    return Problem(*_subdomains((64, 64, 64), (2, 2, 2), (0, 7)))


def test_tasks_are_moved_and_the_solve_is_bit_exact_at_every_slot_count(ddm):
    pb = corner_subdomains()
    rc, err, x, st, info = run(pb)                               # slots = moved + 1 per queue
    assert rc == 0, err
    print(f"\nmoved {st['movedL']}+{st['movedU']} of {st['ntasks']} tasks, most in one queue {st['max_moved']}; {st['in_front']} stand in front of a producer")
    fwd0 = info[(info[:, 0] == 0) & (info[:, 1] == 0), 3].sum()
    bwd7 = info[(info[:, 0] == 1) & (info[:, 1] == 1), 3].sum()
    assert fwd0 > 0 and bwd7 > 0                                 # not vacuous: the creation order leaves tasks more than 24 levels out of place
    assert st["max_moved"] > 0 and st["max_moved"] <= MOVE_MAX
    assert st["in_front"] > 0 and st["in_front_unflagged"] == 0 and st["foreign_producers"] == 0
    assert np.array_equal(x, pb.x_ref)
    for slots in (2 * st["max_moved"], 64):
        rc, err, x, st2, _ = run(pb, slots=slots)
        assert rc == 0, (slots, err)
        assert st2 == st
        assert np.array_equal(x, pb.x_ref), slots


def test_moved_tasks_keep_the_order_rules(ddm):
    """unmoved tasks of a queue ascend as the creation order does wherever a moved task was taken out; every moved task stands in front
    of the first unmoved task with a larger start level, moved tasks among themselves by start level"""
    pb = corner_subdomains()
    rc, err, _, st, info = run(pb)
    assert rc == 0, err
    for g in (0, 1):
        for sw in (0, 1):
            q = info[(info[:, 0] == g) & (info[:, 1] == sw)]
            start, moved = q[:, 2], q[:, 3].astype(bool)
            for k in np.where(moved)[0]:
                later = np.where(~moved[k:])[0]
                assert len(later) and start[k + later[0]] > start[k]          # in front of an unmoved task that starts later
                earlier = np.where(~moved[:k])[0]
                assert not len(earlier) or start[earlier].max() <= start[k]   # ... the first such task
                if k and moved[k - 1]:
                    assert start[k - 1] <= start[k]


def test_nothing_moved_is_the_creation_order(ddm):
    pb = corner_subdomains()
    rc, err, x, st, info = run(pb, move_max=0)
    assert rc == 0, err
    assert st["movedL"] == st["movedU"] == st["max_moved"] == 0 and not info[:, 3].any()
    assert st["in_front"] == 0                                   # no task stands in front of a producer: one slot serves the queue
    assert np.array_equal(x, pb.x_ref)
    out = np.zeros(4, dtype=np.int64)
    assert harness().pipe_queue_same_tasks(ctypes.c_int64(pb.n), _p(pb.rp), _p(pb.ci), _p(pb.lu), _p(pb.diag), ctypes.c_int(len(pb.bp) - 1), _p(pb.bp),
                                           ctypes.c_int(DELTA), ctypes.c_int(GAP), ctypes.c_int(MOVE_MAX), _p(out)) == 0
    assert out[1] == 1 and out[2] == out[3]                      # moving renumbers the tasks and changes nothing else about them


def test_one_slot_deadlocks_and_is_reported(ddm):
    """the detector: a moved task in front of a producer, served by a single workgroup, waits for a task nobody can dequeue"""
    pb = corner_subdomains()
    rc, err, _, st, _ = run(pb, slots=1)
    assert st["in_front"] > 0
    assert rc == 2 and err == "queue order deadlocks with 1 slots", (rc, err)


def test_small_bound_moves_the_largest_gaps(ddm):
    pb = corner_subdomains()
    rc, err, x, st, info = run(pb, move_max=1)
    assert rc == 0, err
    assert st["max_moved"] == 1 and np.array_equal(x, pb.x_ref)


@pytest.mark.parametrize("N,P", [((64, 64, 64), (2, 2, 2)), ((48, 48, 48), (3, 2, 2))])
def test_the_decompositions_of_the_gpu_test(ddm, N, P):
    """every subdomain, pipe::Options defaults, moved + 1 slots: what tests/test_gpu_pipe_queue.py then runs on the device (there
    with 32 or more workgroups per queue)"""
    pb = Problem(*_subdomains(N, P))
    rc, err, x, st, _ = run(pb)
    assert rc == 0, err
    print(f"\n{N} / {P}: moved {st['movedL']}+{st['movedU']} of {st['ntasks']} tasks, most in one queue {st['max_moved']}")
    assert st["movedL"] + st["movedU"] > 0 and st["max_moved"] <= 16          # (16: the bound of two queues per XCD)
    assert np.array_equal(x, pb.x_ref)


def test_block_diagonal_of_12_blocks(ddm):
    """12 queues of different depth (bands of different reach, so chains start at different levels), a small gap so that tasks move"""
    rng = np.random.default_rng(4)
    mats = []
    for b in range(12):
        n = 900 + 150 * b
        offs = sorted(set([1, 7 + b, 30 + 3 * b]))
        B = sp.diags([rng.uniform(-1.0, -0.1, n - k) for k in offs], offs, shape=(n, n), format="csr")
        mats.append(sp.csr_matrix(B + B.T + sp.eye(n) * 8.0))
    pb = Problem(sp.block_diag(mats, format="csr"), np.concatenate([[0], np.cumsum([m.shape[0] for m in mats])]))
    for gap, delta in ((24, 24), (2, 4), (0, 1)):
        rc, err, x, st, _ = run(pb, gap=gap, delta=delta)
        assert rc == 0, (gap, delta, err)
        assert st["foreign_producers"] == 0 and st["in_front_unflagged"] == 0
        assert np.array_equal(x, pb.x_ref), (gap, delta)
        rc, err, x, _, _ = run(pb, gap=gap, delta=delta, slots=64)
        assert rc == 0 and np.array_equal(x, pb.x_ref), (gap, delta, err)


def test_random_sparse_cases(ddm):
    """the matrices of tests/test_pipe_schedule.py::test_random_sparse_and_edge_cases, gaps down to 0"""
    rng = np.random.default_rng(11)
    probs = []
    for n, dens in ((1, 1.0), (2, 1.0), (65, 0.2), (700, 0.01), (3000, 0.002)):
        R = sp.random(n, n, density=dens, random_state=np.random.RandomState(5), format="csr")
        probs.append((sp.csr_matrix(R + R.T + sp.eye(n) * (4.0 + 2.0 * n * dens)), [0, n]))
    probs.append((sp.diags(np.arange(1.0, 301.0)).tocsr(), [0, 100, 300]))
    probs.append(((sp.eye(500) * 2.0 + sp.eye(500, k=-1) * -1.0 + sp.eye(500, k=1) * -1.0).tocsr(), [0, 500]))
    moved = 0
    for M, bp in probs:
        pb = Problem(M, bp, seed=int(rng.integers(1 << 30)))
        for gap, delta in ((24, 16), (0, 1), (3, 2)):
            for slots in (0, 64):
                rc, err, x, st, _ = run(pb, slots=slots, gap=gap, delta=delta)
                if rc == 1:                                      # not applicable (e.g. too many producers): reported, never wrong
                    assert err
                    continue
                assert rc == 0, (M.shape, gap, delta, slots, err)
                assert st["in_front_unflagged"] == 0 and np.array_equal(x, pb.x_ref), (M.shape, gap, delta, slots)
                moved += st["movedL"] + st["movedU"]
    print(f"\nmoved tasks over all cases: {moved}")
