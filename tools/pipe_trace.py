"""Timeline of one pipe-engine ILU(0) solve from the stamped kernel build (diagnostic).
usage: python tools/pipe_trace.py N PX PY PZ [K=V ...]   (K=V sets DDM_PIPE_K)"""
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ddm = ge.import_package()
import torch  # noqa: E402
from dune_ddm_amd import synth  # noqa: E402
from dune_ddm_amd.problem import build_structured  # noqa: E402

N = int(sys.argv[1])
P = tuple(int(a) for a in sys.argv[2:5])
os.environ["DDM_TRSV_MODE"] = "pipe"
for kv in sys.argv[5:]:
    k, v = kv.split("=")
    os.environ["DDM_PIPE_" + k] = v
dec = build_structured(synth.StructuredPoisson((N, N, N), P), overlap=2, pou_type="distance", shrink=0)
mats = [sd.A_dir.tocsr() for sd in dec.subs]
M = sp.block_diag(mats, format="csr")
M.sort_indices()
bp = np.concatenate([[0], np.cumsum([m.shape[0] for m in mats])]).astype(np.int64)
ctx = ddm.torch_context(0)
F = ddm.Ilu0(ctx, ddm.CsrMatrix(ctx, M), bp)
d = torch.as_tensor(np.random.default_rng(0).standard_normal(M.shape[0])).cuda()
x = torch.zeros_like(d)
for _ in range(3):
    F.solve(d, x)
ctx.sync()
st, meta = F.pipe_trace(d, x)
st, meta = F.pipe_trace(d, x)
ctx.sync()
st = st.astype(np.float64)
t0 = st[:, 0].min()
start, first, end = (st[:, 0] - t0) / 100.0, (st[:, 1] - t0) / 100.0, (st[:, 2] - t0) / 100.0   # us
steps = st[:, 6]
print(f"tasks {len(st)}  kernel span {end.max():.1f} us  status {F.status()}")
for g in sorted(set(meta[:, 0]))[:2]:
    for sw in (0, 1):
        m = (meta[:, 0] == g) & (meta[:, 1] == sw)
        dur = end[m] - first[m]
        print(f"group {g} sweep {sw}: tasks {m.sum()} steps {int(steps[m].sum())} span [{start[m].min():.1f}, {end[m].max():.1f}] us; "
              f"per-step us: median {np.median(dur / steps[m]):.3f} mean {dur.sum() / steps[m].sum():.3f}; "
              f"cycles/step: tile-wait {st[m, 3].sum() / steps[m].sum():.0f} producer-wait {st[m, 4].sum() / steps[m].sum():.0f}; "
              f"wave-0 segments per step: top->gathers {st[m, 8].sum() / steps[m].sum():.0f} ->row sum done {st[m, 9].sum() / steps[m].sum():.0f} post {st[m, 11].sum() / steps[m].sum():.0f}; steps (behind the first) that polled producers: {st[m, 12].sum() / steps[m].sum():.2%}, {st[m, 13].sum() / np.maximum(st[m, 12].sum(), 1):.0f} cycles each")
        idx = np.where(m)[0]
        sel = idx[:: max(1, len(idx) // 12)]
        for i in sel:
            print(f"    task {i - idx[0]:4d}: dequeued {start[i]:8.1f} first {first[i]:8.1f} end {end[i]:8.1f} steps {int(steps[i]):4d} "
                  f"us/step {(end[i] - first[i]) / steps[i]:.3f} tile {st[i, 3] / steps[i]:.0f} prod {st[i, 4] / steps[i]:.0f} | a {st[i, 8] / steps[i]:.0f} b {st[i, 9] / steps[i]:.0f} d {st[i, 11] / steps[i]:.0f} cyc/step xcc {int(st[i, 7])}")
# queue order (csrc/trsv_pipe_host.hpp, "Queue order"): span of every sweep, and the moved tasks' wait in their slot.  With nothing
# moved (MOVE=0) the tasks the builder WOULD move are listed instead: same rule, from the start levels in queue order.
info = F.pipe_info()
lvl, moved = info["start_level"], info["moved"].astype(bool)
would = not moved.any()
print(f"queue order: bound {info['move_max']} gap {info['move_gap']} moved {info['moved_forward']}+{info['moved_backward']} (most in one queue {info['max_moved']})")
gap, bound = int(os.environ.get("DDM_PIPE_MOVE_GAP", "24")), 32
for g in sorted(set(meta[:, 0])):
    line = f"group {g}:"
    for sw in (0, 1):
        idx = np.where((meta[:, 0] == g) & (meta[:, 1] == sw))[0]
        line += f"  {'backward' if sw else 'forward'} [{start[idx].min():7.1f}, {end[idx].max():7.1f}] = {end[idx].max() - start[idx].min():7.1f} us"
        if would:
            runmax = np.maximum.accumulate(np.concatenate([[0], lvl[idx][:-1]]))
            cand = np.where(runmax - lvl[idx] > gap)[0]
            cand = cand[np.argsort(-(runmax - lvl[idx])[cand], kind="stable")][:bound]
            moved[idx[cand]] = True
    print(line)
for g in sorted(set(meta[:, 0])):
    for sw in (0, 1):
        idx = np.where((meta[:, 0] == g) & (meta[:, 1] == sw))[0]
        m = idx[moved[idx]]
        if not len(m):
            continue
        w, wall = first[m] - start[m], first[idx] - start[idx]
        print(f"group {g} sweep {sw}: {len(m)} tasks {'that would be moved' if would else 'moved'}: first - dequeued median {np.median(w):.1f} max {w.max():.1f} us "
              f"(all {len(idx)} tasks of the queue: median {np.median(wall):.1f} us); those of more than 150 steps:")
        for i in m[steps[m] > 150]:
            print(f"    task {i - idx[0]:4d}: start level {lvl[i]:4d} steps {int(steps[i]):4d} dequeued {start[i]:8.1f} first {first[i]:8.1f} (waited {first[i] - start[i]:6.1f}) end {end[i]:8.1f}")
np.savez(os.path.join(ROOT, 'gpurun_out', f'pipe_trace{N}.npz'), st=st, meta=meta)
ctx.close()
