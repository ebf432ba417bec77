"""Condenses rocprofv3 counter passes of the operator kernel into one JSON document (profiles/dia_window_pmc_*.json, profiles/dia_code_pmc_*.json).

usage: dia_pmc_json.py OUT.json LABEL COUNTER_CSV [COUNTER_CSV ...]

Each CSV is the *_counter_collection.csv of one run of its own:
  rocprofv3 --pmc <counters> --kernel-include-regex k_spmv_dia --output-format csv -- python bench.py --gpus 1 --steps 20 --warmup 5
(no tracing beside it).  Per counter: launches, mean, min, max per launch; then the figures derived from them."""
import collections
import csv
import json
import statistics
import sys

out, label, files = sys.argv[1], sys.argv[2], sys.argv[3:]
vals = collections.defaultdict(list)
grid = None
for f in files:
    for r in csv.DictReader(open(f)):
        if "k_spmv_dia" in r["Kernel_Name"]:
            vals[r["Counter_Name"]].append(float(r["Counter_Value"]))
            grid = int(r["Grid_Size"])
counters = {k: {"launches": len(v), "mean": statistics.mean(v), "min": min(v), "max": max(v)} for k, v in sorted(vals.items())}
m = {k: c["mean"] for k, c in counters.items()}
derived = {}
if "TCC_HIT_sum" in m and "TCC_MISS_sum" in m:
    derived["l2_hit_rate"] = m["TCC_HIT_sum"] / (m["TCC_HIT_sum"] + m["TCC_MISS_sum"])
    derived["l2_miss_bytes_at_128_per_request"] = 128 * m["TCC_MISS_sum"]
if "FETCH_SIZE" in m:
    derived["fetch_bytes_reported"] = 1024 * m["FETCH_SIZE"]
if "WRITE_SIZE" in m:
    derived["write_bytes_reported"] = 1024 * m["WRITE_SIZE"]
if "TCP_TOTAL_CACHE_ACCESSES_sum" in m and "TCP_TCC_READ_REQ_sum" in m:
    derived["l1_hit_rate"] = 1.0 - m["TCP_TCC_READ_REQ_sum"] / m["TCP_TOTAL_CACHE_ACCESSES_sum"]
if "GRBM_GUI_ACTIVE" in m:
    cycles = m["GRBM_GUI_ACTIVE"] / 8                                              # the counter is summed over the 8 XCDs
    derived["gpu_cycles_per_launch"] = cycles
    if "TA_BUSY_avr" in m:
        derived["address_unit_busy"] = m["TA_BUSY_avr"] / cycles
    if "TCP_TCP_TA_DATA_STALL_CYCLES_sum" in m:
        derived["memory_unit_stalled"] = m["TCP_TCP_TA_DATA_STALL_CYCLES_sum"] / 256 / cycles   # mean over the 256 L1 caches
    if "TA_ADDR_STALLED_BY_TC_CYCLES_sum" in m:
        derived["address_unit_stalled_by_l1"] = m["TA_ADDR_STALLED_BY_TC_CYCLES_sum"] / 256 / cycles
if "SQ_LDS_IDX_ACTIVE" in m and "SQ_LDS_BANK_CONFLICT" in m:                      # (summed over the 256 CUs)
    derived["lds_bank_conflict_share_of_lds_cycles"] = m["SQ_LDS_BANK_CONFLICT"] / max(m["SQ_LDS_IDX_ACTIVE"], 1.0)
    if "GRBM_GUI_ACTIVE" in m:
        derived["lds_busy"] = m["SQ_LDS_IDX_ACTIVE"] / 256 / (m["GRBM_GUI_ACTIVE"] / 8)
doc = {"kernel": "k_spmv_dia", "build": label, "cmd": "python bench.py --gpus 1 --steps 20 --warmup 5", "grid_threads": grid,
       "note": "one run per counter set, counters only (no tracing); values per launch",
       "counters": counters, "derived": derived}
json.dump(doc, open(out, "w"), indent=1)
print(json.dumps(derived, indent=1))
