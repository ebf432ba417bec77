"""Share of coded blocks in the operator's diagonal-row-block layout, on the matrix the benchmark hands to ddm_op_create (host only,
no device needed): blocks, coded blocks, the distribution of the dictionary entries in use, and the bytes of the operator's
device arrays with and without the codes (DDM_SPMV_CODE=0).  One JSON line.

usage: python tools/dia_code_coverage.py [--grid 216] [--parts 2] [--overlap 2] [--kappa constant|islands]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--grid", type=int, default=216)
ap.add_argument("--parts", type=int, default=2)
ap.add_argument("--overlap", type=int, default=2)
ap.add_argument("--kappa", default="constant", choices=["constant", "islands"])
args = ap.parse_args()
ddm = ge.import_package()
from dune_ddm_amd import synth  # noqa: E402
from dune_ddm_amd.problem import RankLocal, build_structured  # noqa: E402

G, P = args.grid, args.parts
kappa = synth.islands_kappa((G - 1,) * 3) if args.kappa == "islands" else None
grid = synth.StructuredPoisson((G, G, G), (P, P, P), kappa)
dec = build_structured(grid, overlap=args.overlap, pou_type="distance", shrink=0, neumann=False)
A = RankLocal(dec, 0, 1).A
A.sort_indices()
n = A.shape[0]
_, kinds, counts = ddm.dia_build_and_apply_host(A, np.ones(n))
info = ddm.dia_codes_host(A, arrays=False)
dia = kinds[:, 2] > 0
rows = (kinds[:, 1] - kinds[:, 0]).astype(np.int64)
hist = np.bincount(info["entries"][info["coded"]], minlength=17)
masks = 4 * n                                                                # (the segment tables are a few KiB)
out = {"grid": G, "parts": P, "overlap": args.overlap, "kappa": args.kappa, "rows": int(n), "nnz": int(A.nnz), "blocks": int(len(kinds)),
       "diagonal_blocks": int(dia.sum()), "coded_blocks": int(info["coded"].sum()),
       "coded_share_of_diagonal_blocks": float(info["coded"].sum() / max(1, dia.sum())),
       "rows_in_coded_blocks": int(rows[info["coded"]].sum()), "segments": counts["segments"],
       "blocks_in_segments_with_slabs": int(info["slabs"].sum()),
       "dictionary_entries_histogram": {str(k): int(v) for k, v in enumerate(hist) if v},
       "operator_device_bytes": {"slab_layout": int(8 * counts["slots"] + masks + 32 * len(kinds)),     # 32-byte block descriptors
                                 "coded_layout": int(8 * info["slots_built"] + masks + 40 * len(kinds)
                                                     + (16 * n + 128 * int(info["coded"].sum()) if info["coded"].any() else 0))}}
print(json.dumps(out))
