"""What tests/test_trsv_multi_plan.py (CPU) and tests/test_gpu_trsv_multi_xcd.py (GPU) share: the cases of the single-launch block
solve (engine `xcd` of the multi-RHS path, csrc/engine_multi_xcd.hpp).  They are the factors of tests/trsv_cases.py plus one matrix of
this module's own, `loop8`: no case there has a level of one diagonal block with more (row, column quad) items at m = 32 than a team
of ONE XCD has threads, which is the only shape at which a thread of k_trsv_multi_xcd takes a second item of a level.  Nothing here
needs a GPU."""
import functools

import numpy as np

from tests import trsv_cases as tc

WG = 256                          # threads of a workgroup of k_trsv_multi_xcd
GRID = 256                        # persistent_grid on a 256-CU device: one workgroup per CU
XCD_TEAM_THREADS = GRID // 8 * WG  # threads of a team that is one XCD (8 or more diagonal blocks)
WIDTHS = (1, 3, 4, 7, 24, 32)


def _loop8():
    # 8 blocks of two layers of 1100 rows: levels of 1100 rows per block, 1100 * 32 / 4 = 8800 quad items > 8192 threads
    return tc._diag_blocks([tc.layered([1100, 1100], 2, 50 + b) for b in range(8)])


class LoopCase(tc.Case):
    def __init__(self):
        self.name = "loop8"
        self.M, self.block_ptr = _loop8()
        self.n = self.M.shape[0]
        self.table = tc.level_table(self.M, self.block_ptr)
        self.whole = tc.level_table(self.M, [0, self.n])
        self.C = tc.bound(self.table)


@functools.lru_cache(maxsize=None)
def case(name):
    return LoopCase() if name == "loop8" else tc.case(name)


def teams(c):
    """teams the kernel forms on a device where every XCD hosts workgroups"""
    return min(len(c.block_ptr) - 1, 8)


def team_threads(c):
    """threads of the smallest team: XCD x belongs to team x % T"""
    T = teams(c)
    return min(sum(1 for x in range(8) if x % T == t) for t in range(T)) * XCD_TEAM_THREADS


def max_block_level_rows(c):
    return max(int(t.m.max()) for t in c.table.triangles)


def has_wide_level(c):
    return any(bool(np.any(t.w >= tc.WIDE_W)) for t in c.whole.triangles)
