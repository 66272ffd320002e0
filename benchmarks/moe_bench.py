#!/usr/bin/env python3
"""Mixtral-8x7B MoE layer microbenchmark on one MI355X: router (HIP) + grouped gate_up GEMM + SiLU*mul + grouped
down GEMM with the fused weighted combine, at decode-like token counts (BASELINE config 5: 128 threads) and a
prefill chunk. Reports us/layer and the expert-weight streaming rate (every expert with >= 1 token is read once) for
the LDS-tiled grouped GEMM and, at decode sizes (T <= 512), for the grouped weight-streaming kernel.
``--weight-dtype fp8`` streams e4m3 expert tiles (ops.tile_experts_fp8; the LDS-tiled grouped GEMM then runs on the
dequantised bf16 experts, and stream_weight_TB/s counts the fp8 bytes actually streamed); ``--weight-dtype mxfp4`` the
e2m1 tiles with their e8m0 block-scale images (ops.tile_experts_mxfp4) the same way.
``--compare bf16,fp8,mxfp4`` times the grouped streaming kernel on those expert formats of the SAME weights, inputs and
routing in one process, the formats interleaved within every timing round: one JSON line per T with us/layer and the
effective TB/s over the bytes actually streamed (tiles + scales of the experts with >= 1 token) per format.

  python benchmarks/moe_bench.py            # T = 1, 16, 64, 128, 512, 2048
  python benchmarks/moe_bench.py 1,64,256 --weight-dtype fp8
  python benchmarks/moe_bench.py 64,128,256,512 --compare bf16,fp8,mxfp4
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


def expert_bytes(fmt: str, d: int, F: int) -> int:
    """Bytes the streaming kernel reads for one expert: the tiles of w13 and w2 and their scales."""
    return ops.tiled_weight_bytes((2 * F, d), fmt) + ops.tiled_weight_bytes((d, F), fmt)


def compare(Ts, fmts, dev, E, K, d, F, router, w13, w2, iters=20, rounds=5):
    """The grouped streaming kernel on every format of ``fmts``, interleaved: round by round, format by format."""
    tiles = {f: (ops.tile_experts_as(w13, f, True), ops.tile_experts_as(w2, f)) for f in fmts}
    for T in Ts:
        x = torch.randn(T, d, device=dev, dtype=torch.bfloat16)

        def layer_stream(f):
            (w13t, w13s), (w2t, w2s) = tiles[f]
            r = ops.moe_route(torch.nn.functional.linear(x, router), K)
            a = ops.grouped_stream_glu(x, w13t, r, scale=w13s)
            out = torch.zeros(T, d, dtype=torch.float32, device=dev)
            ops.grouped_stream_combine(a, w2t, r, T, out, scale=w2s)
            return out

        res = {f: [] for f in fmts}
        for _ in range(rounds):
            for f in fmts:
                res[f].append(timeit(lambda: layer_stream(f), iters=iters, rounds=1))
        r = ops.moe_route(torch.nn.functional.linear(x, router), K)
        used = int((r.expert_off[1:] - r.expert_off[:-1] > 0).sum().item())
        row = {"T": T, "experts_used": used, "max_rows_per_expert": int((r.expert_off[1:] - r.expert_off[:-1]).max())}
        for f in fmts:
            us = statistics.median(res[f])
            row[f + "_stream_us_per_layer"] = round(us, 1)
            row[f + "_stream_weight_TB/s"] = round(used * expert_bytes(f, d, F) / us / 1e6, 2)
            row[f + "_rounds_us"] = [round(v, 1) for v in res[f]]
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("Ts", nargs="?", default="1,16,64,128,512,2048", help="comma-separated token counts")
    ap.add_argument("--weight-dtype", default="bf16", choices=["bf16", "fp8", "mxfp4"])
    ap.add_argument("--compare", default="", help="comma-separated expert formats to time interleaved (streaming kernel)")
    args = ap.parse_args()
    Ts = [int(x) for x in args.Ts.split(",")]
    wd = args.weight_dtype
    dev = torch.device("cuda:0")
    E, K, d, F = 8, 2, 4096, 14336
    torch.manual_seed(0)
    router = (torch.randn(E, d, device=dev) * d ** -0.5).to(torch.bfloat16)
    w13 = (torch.randn(E, 2 * F, d, device=dev) * d ** -0.5).to(torch.bfloat16)
    w2 = (torch.randn(E, d, F, device=dev) * F ** -0.5).to(torch.bfloat16)
    if args.compare:
        fmts = [ops.weight_format(f).name for f in args.compare.split(",")]
        if any(T > 512 for T in Ts):
            ap.error("--compare times the streaming kernel: T <= 512")
        return compare(Ts, fmts, dev, E, K, d, F, router, w13, w2)
    # (tiles, scales or None) in the grouped weight-streaming layout; quantised: w13 / w2 become the dequantised experts
    # the LDS-tiled grouped GEMM reads
    (w13t, w13s), (w2t, w2s) = ops.tile_experts_as(w13, wd, True), ops.tile_experts_as(w2, wd)
    if w13s is not None:
        w13, w2 = ops.untile_experts_as(w13t, w13s, True), ops.untile_experts_as(w2t, w2s)
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
        bytes_s = used * expert_bytes(wd, d, F)  # the tiles and scales actually streamed
        print(json.dumps({"weight_dtype": wd, "T": T, "experts_used": used,
                          "us_per_layer": round(us, 1),
                          "weight_TB/s": round(bytes_w / us / 1e6, 2),
                          "TFLOP/s": round(2 * T * K * 3 * F * d / us / 1e6, 1),
                          "stream_us_per_layer": round(us_s, 1) if us_s else None,
                          "stream_weight_TB/s": round(bytes_s / us_s / 1e6, 2) if us_s else None,
                          "stream_unpinned_us_per_layer": round(us_u, 1) if us_u else None}), flush=True)


if __name__ == "__main__":
    main()
