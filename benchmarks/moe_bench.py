#!/usr/bin/env python3
"""Mixtral-8x7B MoE layer microbenchmark on one MI355X: router (HIP) + grouped gate_up GEMM + SiLU*mul + grouped
down GEMM with the fused weighted combine, at decode-like token counts (BASELINE config 5: 128 threads) and a
prefill chunk. Reports us/layer and the expert-weight streaming rate (every expert with >= 1 token is read once) for
the LDS-tiled grouped GEMM and, at decode sizes (T <= 512), for the grouped weight-streaming kernel.
``--weight-dtype fp8`` streams e4m3 expert tiles (ops.tile_experts_fp8; the LDS-tiled grouped GEMM then runs on the
dequantised bf16 experts, and stream_weight_TB/s counts the fp8 bytes actually streamed).

  python benchmarks/moe_bench.py            # T = 1, 16, 64, 128, 512, 2048
  python benchmarks/moe_bench.py 1,64,256 --weight-dtype fp8
"""
from __future__ import annotations

import argparse
import json
import statistics

import torch

from kafka_llm_service_amd import ops


def timeit(fn, iters=20, rounds=5):
    res = []
    for _ in range(rounds):
        fn()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        res.append(s.elapsed_time(e) * 1e3 / iters)
    return statistics.median(res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("Ts", nargs="?", default="1,16,64,128,512,2048", help="comma-separated token counts")
    ap.add_argument("--weight-dtype", default="bf16", choices=["bf16", "fp8"])
    args = ap.parse_args()
    Ts = [int(x) for x in args.Ts.split(",")]
    fp8 = args.weight_dtype == "fp8"
    dev = torch.device("cuda:0")
    E, K, d, F = 8, 2, 4096, 14336
    torch.manual_seed(0)
    router = (torch.randn(E, d, device=dev) * d ** -0.5).to(torch.bfloat16)
    w13 = (torch.randn(E, 2 * F, d, device=dev) * d ** -0.5).to(torch.bfloat16)
    w2 = (torch.randn(E, d, F, device=dev) * F ** -0.5).to(torch.bfloat16)
    w13s = w2s = None
    if fp8:  # (tiles, scales); w13 / w2 become the dequantised experts the LDS-tiled grouped GEMM reads
        (w13t, w13s), (w2t, w2s) = ops.tile_experts_fp8(w13, glu=True), ops.tile_experts_fp8(w2)
        w13, w2 = ops.untile_experts_fp8(w13t, w13s, glu=True), ops.untile_experts_fp8(w2t, w2s)
    else:
        w13t, w2t = ops.tile_experts(w13, glu=True), ops.tile_experts(w2)  # grouped weight-streaming layout
    for T in Ts:
        x = torch.randn(T, d, device=dev, dtype=torch.bfloat16)

        def layer():
            r = ops.moe_route(torch.nn.functional.linear(x, router), K)
            h = ops.grouped_gemm(x, w13, r, gather=True)
            a = ops.silu_mul(h)
            out = torch.zeros(T, d, dtype=torch.float32, device=dev)
            ops.grouped_gemm(a, w2, r, gather=False, combine_out=out)
            return out

        def layer_stream():
            r = ops.moe_route(torch.nn.functional.linear(x, router), K)
            a = ops.grouped_stream_glu(x, w13t, r, scale=w13s)
            out = torch.zeros(T, d, dtype=torch.float32, device=dev)
            ops.grouped_stream_combine(a, w2t, r, T, out, scale=w2s)
            return out

        us = timeit(layer)
        us_s = timeit(layer_stream) if T <= 512 else None
        us_u = None
        if us_s:  # the grouped streaming kernel without the pinned prefetch (A/B of ops.GROUPED_PIN)
            ops.GROUPED_PIN = False
            us_u = timeit(layer_stream)
            ops.GROUPED_PIN = True
        r = ops.moe_route(torch.nn.functional.linear(x, router), K)
        used = int((r.expert_off[1:] - r.expert_off[:-1] > 0).sum().item())
        bytes_w = used * (2 * F * d + d * F) * 2
        bytes_s = used * (3 * F * d + 4 * (2 * F + d)) if fp8 else bytes_w  # fp8: one byte + the row scales
        print(json.dumps({"weight_dtype": args.weight_dtype, "T": T, "experts_used": used,
                          "us_per_layer": round(us, 1),
                          "weight_TB/s": round(bytes_w / us / 1e6, 2),
                          "TFLOP/s": round(2 * T * K * 3 * F * d / us / 1e6, 1),
                          "stream_us_per_layer": round(us_s, 1) if us_s else None,
                          "stream_weight_TB/s": round(bytes_s / us_s / 1e6, 2) if us_s else None,
                          "stream_unpinned_us_per_layer": round(us_u, 1) if us_u else None}), flush=True)


if __name__ == "__main__":
    main()
