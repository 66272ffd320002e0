"""Time of the token-logprobs kernel (ops/csrc/logprobs.hip) at a decode batch: 64 rows x 128,256 bf16 logits for
K = 0, 5 and 20 alternatives, next to the greedy ``ops.sample`` launch on the same tensor — the yardstick: both
stream the same bytes once. Device-event time over 200 back-to-back calls, median of 7 repeats, the variants
interleaved. Writes one JSON line per variant (profiles/logprobs/kernel_bench.jsonl by default).

    python benchmarks/logprobs_bench.py [--out FILE] [--rows 64] [--vocab 128256]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kafka_llm_service_amd import ops  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/logprobs/kernel_bench.jsonl")
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("logprobs_bench needs a GPU")
    dev = torch.device("cuda:0")
    B, V = a.rows, a.vocab
    g = torch.Generator(device=dev).manual_seed(0)
    lg = (torch.randn(B, V, device=dev, generator=g) * 4).to(torch.bfloat16)
    zero_t = torch.zeros(B, device=dev)
    toks = ops.sample(lg, zero_t).clone()
    variants = {"sample_greedy": lambda: ops.sample(lg, zero_t)}
    for k in (0, 5, 20):
        out = ops.unpack_logprob_records(ops.logprob_records(B, k, dev), k)
        variants[f"logprobs_k{k}"] = (lambda k=k, out=out: ops.token_logprobs(lg, toks, None, k, out=out))
    for f in variants.values():  # warm every variant (code objects, workspaces)
        for _ in range(10):
            f()
    torch.cuda.synchronize()
    times = {n: [] for n in variants}
    for _ in range(a.repeats):
        for n, f in variants.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.calls):
                f()
            e.record()
            torch.cuda.synchronize()
            times[n].append(s.elapsed_time(e) * 1e3 / a.calls)
    base = statistics.median(times["sample_greedy"])
    nbytes = B * V * 2
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        for n, ts in times.items():
            us = statistics.median(ts)
            rec = {"bench": "logprobs_kernel", "variant": n, "rows": B, "vocab": V, "dtype": "bf16",
                   "us_per_call": round(us, 2), "us_min": round(min(ts), 2), "us_max": round(max(ts), 2),
                   "ratio_to_sample_greedy": round(us / base, 3), "logit_gb_per_s": round(nbytes / us / 1e3, 1),
                   "calls": a.calls, "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
            print(json.dumps(rec))
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
