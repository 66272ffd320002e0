"""Sampler time at 64 rows x 128,256 bf16 logits, greedy and T = 0.7, one JSON line per case (device events around
200 back-to-back launches, median of 5 windows).

  --proc none      no logits processing (the headline path)
  --proc penalty   every row a penalty-only processing row (presence 0.5, frequency 1.5, zero counts)
  --logit-bias N   every row carries N bias entries (its own table row; implies a processing row); 0 = none
  --min-p P        every row carries min_p = P in proc[7] (implies a processing row): under T = 0.7 a split two-pass
                   row, or one more test in the rejection loop with --top-p; greedy rows ignore it; 0 = none
  --top-p P        every row samples with top_p = P (the one-workgroup rejection loop under T = 0.7); 1 = none
  --repetition R   every row a penalty slot with repetition_penalty = R in rep_tab and a random third of the vocabulary
                   seen (half as prompt flags, half as counts); combines with --proc penalty; 1 = none
  --ones-table     with --proc penalty: pass an all-ones rep_tab, the launch the engine makes for a penalty row while
                   some other request has a repetition penalty (the kernel instantiation with the table)

The script also runs on a tree from before logit_bias (``ops.sample`` without ``bias_tab``): there --logit-bias must
be 0, which is how the parent's numbers beside this tree's were taken."""
import argparse
import inspect
import json
import statistics

import numpy as np
import torch

from kafka_llm_service_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--proc", choices=("none", "penalty"), default="none")
ap.add_argument("--logit-bias", type=int, default=0)
ap.add_argument("--min-p", type=float, default=0.0)
ap.add_argument("--top-p", type=float, default=1.0)
ap.add_argument("--repetition", type=float, default=1.0)
ap.add_argument("--ones-table", action="store_true")
ap.add_argument("--rows", type=int, default=64)
ap.add_argument("--vocab", type=int, default=128256)
ap.add_argument("--tag", default="")
a = ap.parse_args()

dev = torch.device("cuda:0")
B, V = a.rows, a.vocab
lg = (torch.randn(B, V, generator=torch.Generator().manual_seed(0)) * 3).to(torch.bfloat16).to(dev)
sd = torch.arange(B, dtype=torch.int64, device=dev)
has_bias = "bias_tab" in inspect.signature(ops.sample).parameters
kw = {}
if a.top_p < 1.0:
    kw["top_p"] = torch.full((B,), a.top_p, device=dev)
if a.proc != "none" or a.logit_bias or a.min_p or a.repetition != 1.0:
    proc = np.zeros((B, 8), dtype=np.int32)
    proc[:, 2] = -1
    if a.min_p:
        from kafka_llm_service_amd.engine.logits_proc import min_p_bits  # (a tree before min_p has none: an error)

        proc[:, 7] = min_p_bits(a.min_p)
    kw["mask_tab"] = torch.zeros(1, -(-V // 32), dtype=torch.int32, device=dev)
    if a.proc == "penalty":
        proc[:, 2] = np.arange(B)
        proc[:, 3:5] = np.array([0.5, 1.5], dtype=np.float32).view(np.int32)
        kw["counts"] = torch.zeros(B, -(-V // 8) * 8, dtype=torch.int32, device=dev)
    if a.ones_table and a.proc == "penalty" and a.repetition == 1.0:
        kw["rep_tab"] = torch.ones(B, 2, device=dev)
    if a.repetition != 1.0:
        from kafka_llm_service_amd.engine.logits_proc import rep_factors  # (a tree before the penalty has none)
        from kafka_llm_service_amd.engine.step_plan import COUNT_SEEN_PROMPT

        proc[:, 2] = np.arange(B)
        rng = np.random.default_rng(2)
        cnt = np.zeros((B, -(-V // 8) * 8), dtype=np.int32)
        for i in range(B):
            ids = rng.choice(V, V // 3, replace=False)
            cnt[i, ids[:V // 6]] = COUNT_SEEN_PROMPT
            cnt[i, ids[V // 6:]] = rng.integers(1, 4, ids.size - V // 6)
        kw["counts"] = torch.from_numpy(cnt).to(dev)
        kw["rep_tab"] = torch.from_numpy(np.tile(rep_factors(a.repetition), (B, 1))).to(dev)
    if has_bias:
        n, M = a.logit_bias, ops.LOGIT_BIAS_MAX
        tab = np.zeros((B, 2 * M), dtype=np.int32)
        rng = np.random.default_rng(1)
        for i in range(B if n else 0):
            tab[i, :n] = np.sort(rng.choice(V, n, replace=False))
            tab[i, M:M + n] = (rng.integers(-32, 33, n) / 8.0).astype(np.float32).view(np.int32)
            proc[i, 5:7] = (i, n)
        kw["bias_tab"] = torch.from_numpy(tab).to(dev)  # (always passed: without it ops.sample checks proc on the host)
    elif a.logit_bias:
        raise SystemExit("this tree's sampler has no logit_bias")
    kw["proc"] = torch.from_numpy(proc).to(dev)

for name, temp in (("greedy", 0.0), ("T0.7", 0.7)):
    t = torch.full((B,), temp, device=dev)
    res = []
    for r in range(5):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(20):
            ops.sample(lg, t, seeds=sd, **kw)
        torch.cuda.synchronize()
        s.record()
        for _ in range(200):
            ops.sample(lg, t, seeds=sd, **kw)
        e.record()
        torch.cuda.synchronize()
        res.append(s.elapsed_time(e) * 1e3 / 200)
    print(json.dumps({"bench": "sample", "tag": a.tag, "rows": B, "vocab": V, "mode": name, "proc": a.proc,
                      "logit_bias": a.logit_bias, "min_p": a.min_p, "top_p": a.top_p, "repetition": a.repetition, "ones_table": a.ones_table,
                      "us_per_call": round(statistics.median(res), 2), "min": round(min(res), 2), "max": round(max(res), 2)}), flush=True)
