"""JSON mode kernel time at V = 128,256 (the Llama-3 token table) for 1, 16 and 64 JSON rows: mask + advance
(ops/csrc/json_mask.hip) beside the sampler's own time for the same rows (T = 0.7, each row a mode-1 mask row), one
JSON line per row count. Device events around 200 back-to-back launches; the two things measured alternate round by
round (5 rounds each) and the medians are reported.

  --state NAME   the automaton state every row stands in: in-string (most tokens live, the longest walks; default),
                 start, after-value, done
"""
import argparse
import json
import statistics

import numpy as np
import torch

from kafka_llm_service_amd import ops
from kafka_llm_service_amd.engine import json_mode as jm
from kafka_llm_service_amd.engine.tokenizer import get_tokenizer
from kafka_llm_service_amd.ops import reference as ref

STATES = {"in-string": b'{"k":"va', "start": b"", "after-value": b'{"k":[1 ', "done": b"{}"}
ap = argparse.ArgumentParser()
ap.add_argument("--state", choices=sorted(STATES), default="in-string")
ap.add_argument("--rows", type=int, nargs="*", default=[1, 16, 64])
ap.add_argument("--tag", default="")
a = ap.parse_args()

dev = torch.device("cuda:0")
tok = get_tokenizer()
table = jm.table_for(tok, tok.eos_ids)
tabs = ops.JsonTables(table, dev)
V, ROW0 = table.V, 512
st = ref.json_walk(jm.START_STATE, STATES[a.state])
live = int(np.unpackbits(ref.json_mask_ref(st, table).view(np.uint8)).sum())


def window(fn) -> float:
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(200):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / 200


for B in a.rows:
    lg = (torch.randn(B, V, generator=torch.Generator().manual_seed(0)) * 3).to(torch.bfloat16).to(dev)
    state0 = torch.from_numpy(np.tile(jm.state_record(st), (B, 1))).to(dev)
    state = state0.clone()
    rows = torch.from_numpy(np.stack([np.arange(B), np.arange(B)], axis=1).astype(np.int32)).to(dev)
    mask_tab = torch.zeros(ROW0 + B, table.W, dtype=torch.int32, device=dev)
    proc = np.zeros((B, 8), dtype=np.int32)
    proc[:, 0], proc[:, 1], proc[:, 2] = 1, ROW0 + np.arange(B), -1
    proc = torch.from_numpy(proc).to(dev)
    t = torch.full((B,), 0.7, device=dev)
    sd = torch.arange(B, dtype=torch.int64, device=dev)
    out = torch.zeros(B, dtype=torch.int64, device=dev)
    bias = torch.zeros(1, 2 * ops.LOGIT_BIAS_MAX, dtype=torch.int32, device=dev)
    ops.json_mask(tabs, rows, state, mask_tab, ROW0)
    ops.sample(lg, t, seeds=sd, out=out, proc=proc, mask_tab=mask_tab, bias_tab=bias)  # the ids the advance walks

    def json_kernels():
        state.copy_(state0)  # (the advance moves the state: every launch starts from the same one)
        ops.json_mask(tabs, rows, state, mask_tab, ROW0)
        ops.json_advance(tabs, rows, out, state)

    def reset_only():
        state.copy_(state0)

    def mask_only():
        ops.json_mask(tabs, rows, state0, mask_tab, ROW0)

    def sampler():
        ops.sample(lg, t, seeds=sd, out=out, proc=proc, mask_tab=mask_tab, bias_tab=bias)

    res = {"json": [], "reset": [], "mask": [], "sample": []}
    for _ in range(5):  # interleaved rounds
        res["json"].append(window(json_kernels))
        res["sample"].append(window(sampler))
        res["mask"].append(window(mask_only))
        res["reset"].append(window(reset_only))
    med = {k: statistics.median(v) for k, v in res.items()}
    print(json.dumps({"bench": "json_mask", "tag": a.tag, "rows": B, "vocab": V, "state": a.state, "live_tokens": live,
                      "mask_plus_advance_us": round(med["json"] - med["reset"], 2), "mask_us": round(med["mask"], 2),
                      "state_reset_us": round(med["reset"], 2), "sampler_us": round(med["sample"], 2),
                      "json_min_max": [round(min(res["json"]), 2), round(max(res["json"]), 2)],
                      "sampler_min_max": [round(min(res["sample"]), 2), round(max(res["sample"]), 2)]}), flush=True)
