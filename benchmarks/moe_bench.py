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

``--tiles-only`` times prefill-sized steps (T = 1024 .. 8192) on the grouped tile GEMM (ops.grouped_tiles_*, the tiles of
``--weight-dtype``) beside ops.grouped_gemm + silu_mul on the dequantised row-major experts, two interleaved rounds.
With ``--weight-dtype mxfp4 --act-dtype mxfp8`` it times instead the MXFP8-activation layer on the grouped scaled-MFMA
kernel (csrc/grouped_tile_gemm_mx.hip, quantiser launch included) beside the bf16-MFMA grouped tile kernel and beside
itself with ``quant_out`` off. With ``--weight-dtype fp8 --act-dtype fp8`` it times the per-row-fp8-activation layer on
the grouped e4m3 x e4m3 MFMA kernel (csrc/grouped_tile_gemm_f8.hip, both quantiser launches included) beside the
bf16-MFMA grouped tile kernel on the same fp8 tiles.

``--fused-router`` times the router alone — ``ops.moe_gate_route`` (one launch) beside ``F.linear`` + ``ops.moe_route``
(two) — and the whole layer with either router (the streaming kernel up to T = 640, the LDS-tiled grouped GEMM above),
two interleaved rounds; ``--d`` sets the model width (6144 = Mixtral-8x22B), ``--router-only`` skips the layer.

  python benchmarks/moe_bench.py            # T = 1, 16, 64, 128, 512, 2048
  python benchmarks/moe_bench.py --fused-router --d 6144 --router-only
  python benchmarks/moe_bench.py --tiles-only --weight-dtype mxfp4
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


def tiles_only(Ts, wd, dev, E, K, d, F, router, w13, w2, rounds=2):
    """Prefill-sized steps: the layer on the grouped tile GEMM (ops.grouped_tiles_*, the experts' tiles of format ``wd``)
    beside ops.grouped_gemm + silu_mul on the dequantised row-major experts, interleaved round by round; every round's
    us per layer is printed, with the achieved TFLOP/s of the medians. Also the largest output difference of the two.
    (``--act-dtype mxfp8``: tiles_act_mx below instead.)"""
    (w13t, w13s), (w2t, w2s) = ops.tile_experts_as(w13, wd, True), ops.tile_experts_as(w2, wd)
    if w13s is not None:
        w13, w2 = ops.untile_experts_as(w13t, w13s, True), ops.untile_experts_as(w2t, w2s)
    for T in Ts:
        x = torch.randn(T, d, device=dev, dtype=torch.bfloat16)

        def layer_rows():
            r = ops.moe_route(torch.nn.functional.linear(x, router), K)
            a = ops.silu_mul(ops.grouped_gemm(x, w13, r, gather=True))
            out = torch.zeros(T, d, dtype=torch.float32, device=dev)
            return ops.grouped_gemm(a, w2, r, gather=False, combine_out=out)

        def layer_tiles():
            r = ops.moe_route(torch.nn.functional.linear(x, router), K)
            a = ops.grouped_tiles_glu(x, w13t, r, scale=w13s)
            out = torch.zeros(T, d, dtype=torch.float32, device=dev)
            return ops.grouped_tiles_combine(a, w2t, r, T, out, scale=w2s)

        o_r, o_t = layer_rows(), layer_tiles()
        diff = float((o_r - o_t).abs().max() / o_r.abs().max())
        res = {"rows": [], "tiles": []}
        for _ in range(rounds):
            res["rows"].append(timeit(layer_rows, iters=10, rounds=3))
            res["tiles"].append(timeit(layer_tiles, iters=10, rounds=3))
        flop = 2 * T * K * 3 * F * d
        med = {k: statistics.median(v) for k, v in res.items()}
        print(json.dumps({"weight_dtype": wd, "T": T,
                          "grouped_gemm_us_per_layer": [round(v, 1) for v in res["rows"]],
                          "grouped_tiles_us_per_layer": [round(v, 1) for v in res["tiles"]],
                          "grouped_gemm_TFLOP/s": round(flop / med["rows"] / 1e6, 1),
                          "grouped_tiles_TFLOP/s": round(flop / med["tiles"] / 1e6, 1),
                          "max_rel_diff": round(diff, 5)}), flush=True)


def tiles_act_mx(Ts, dev, E, K, d, F, router, w13, w2, rounds=2):
    """Prefill-sized steps on the MXFP4 expert tiles, three layers interleaved round by round: ``mx`` = MXFP8 activations
    on the grouped scaled-MFMA kernel with the quantising GLU epilogue (ops.grouped_tiles_*(act="mxfp8"), the quantiser's
    launch included), ``tiles`` = the bf16-MFMA grouped tile kernel, ``mx_bf16_mid`` = ``mx`` with ``quant_out`` off (a
    bf16 intermediate and a second quantiser launch: what the fused epilogue buys). Every round's us is printed."""
    (w13t, w13s), (w2t, w2s) = ops.tile_experts_as(w13, "mxfp4", True), ops.tile_experts_as(w2, "mxfp4")
    del w13, w2
    for T in Ts:
        x = torch.randn(T, d, device=dev, dtype=torch.bfloat16)

        def layer(act, quant_out):
            r = ops.moe_route(torch.nn.functional.linear(x, router), K)
            a = ops.grouped_tiles_glu(x, w13t, r, scale=w13s, act=act, quant_out=quant_out)
            out = torch.zeros(T, d, dtype=torch.float32, device=dev)
            return ops.grouped_tiles_combine(a, w2t, r, T, out, scale=w2s, act=act)

        paths = {"mx": lambda: layer("mxfp8", True), "tiles": lambda: layer("bf16", False),
                 "mx_bf16_mid": lambda: layer("mxfp8", False)}
        o_t, o_m = paths["tiles"](), paths["mx"]()
        diff = float((o_t - o_m).abs().max() / o_t.abs().max())
        res = {k: [] for k in paths}
        for _ in range(rounds):
            for k, fn in paths.items():
                res[k].append(timeit(fn, iters=10, rounds=3))
        flop = 2 * T * K * 3 * F * d
        row = {"weight_dtype": "mxfp4", "act_dtype": "mxfp8", "T": T}
        for k, v in res.items():
            row[k + "_us_per_layer"] = [round(u, 1) for u in v]
            row[k + "_TFLOP/s"] = round(flop / statistics.median(v) / 1e6, 1)
        row["mx_vs_tiles_max_rel_diff"] = round(diff, 5)
        print(json.dumps(row), flush=True)


def tiles_act_f8(Ts, dev, E, K, d, F, router, w13, w2, rounds=2):
    """Prefill-sized steps on the fp8 expert tiles, two layers interleaved round by round: ``f8`` = per-row fp8
    activations on the grouped e4m3 x e4m3 MFMA kernel (ops.grouped_tiles_*(act="fp8"): both quantiser launches, of x and
    of the bf16 intermediate, included), ``tiles`` = the bf16-MFMA grouped tile kernel on the same tiles. Every round's us
    is printed."""
    (w13t, w13s), (w2t, w2s) = ops.tile_experts_as(w13, "fp8", True), ops.tile_experts_as(w2, "fp8")
    del w13, w2
    for T in Ts:
        x = torch.randn(T, d, device=dev, dtype=torch.bfloat16)

        def layer(act):
            r = ops.moe_route(torch.nn.functional.linear(x, router), K)
            a = ops.grouped_tiles_glu(x, w13t, r, scale=w13s, act=act)
            out = torch.zeros(T, d, dtype=torch.float32, device=dev)
            return ops.grouped_tiles_combine(a, w2t, r, T, out, scale=w2s, act=act)

        paths = {"f8": lambda: layer("fp8"), "tiles": lambda: layer("bf16")}
        o_t, o_f = paths["tiles"](), paths["f8"]()
        diff = float((o_t - o_f).abs().max() / o_t.abs().max())
        res = {k: [] for k in paths}
        for _ in range(rounds):
            for k, fn in paths.items():
                res[k].append(timeit(fn, iters=10, rounds=3))
        flop = 2 * T * K * 3 * F * d
        row = {"weight_dtype": "fp8", "act_dtype": "fp8", "T": T}
        for k, v in res.items():
            row[k + "_us_per_layer"] = [round(u, 1) for u in v]
            row[k + "_TFLOP/s"] = round(flop / statistics.median(v) / 1e6, 1)
        row["f8_vs_tiles_max_rel_diff"] = round(diff, 5)
        print(json.dumps(row), flush=True)


def fused_router(Ts, dev, E, K, d, router, layer_of, rounds=2):
    """Router alone and whole layer, fused launch beside F.linear + moe_route, interleaved round by round; every round's
    us is printed. ``layer_of(x, route)`` runs the experts on a routing, or is None (router only)."""
    for T in Ts:
        x = torch.randn(T, d, device=dev, dtype=torch.bfloat16)
        routes = {"two_launch": lambda: ops.moe_route(torch.nn.functional.linear(x, router), K),
                  "fused": lambda: ops.moe_gate_route(x, router, K)}
        a, b = routes["two_launch"](), routes["fused"]()
        same = all(torch.equal(getattr(a, f), getattr(b, f)) for f in ("topk_e", "perm_tok", "expert_off", "tile_off"))
        res = {k + sfx: [] for k in routes for sfx in ("_router_us", "_layer_us")}
        for _ in range(rounds):
            for k, fn in routes.items():
                res[k + "_router_us"].append(round(timeit(fn, iters=50, rounds=5), 2))
            for k, fn in routes.items():
                if layer_of is not None:
                    res[k + "_layer_us"].append(round(timeit(lambda: layer_of(x, fn()), iters=10, rounds=3), 1))
        print(json.dumps({"T": T, "d": d, "E": E, "k": K, "same_routing": same, **res}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("Ts", nargs="?", default="1,16,64,128,512,2048", help="comma-separated token counts")
    ap.add_argument("--weight-dtype", default="bf16", choices=["bf16", "fp8", "mxfp4"])
    ap.add_argument("--compare", default="", help="comma-separated expert formats to time interleaved (streaming kernel)")
    ap.add_argument("--tiles-only", action="store_true",
                    help="prefill sizes (default T = 1024, 2048, 4096, 8192): the grouped tile GEMM on the expert tiles "
                         "of --weight-dtype beside grouped_gemm on the dequantised row-major experts")
    ap.add_argument("--act-dtype", default="bf16", choices=list(ops.ACT_DTYPES),
                    help="with --tiles-only --weight-dtype mxfp4: mxfp8 times the grouped scaled-MFMA kernel beside the "
                         "bf16-MFMA grouped tile kernel and beside itself without the quantising epilogue; with "
                         "--tiles-only --weight-dtype fp8: fp8 times the grouped e4m3 x e4m3 MFMA kernel (both "
                         "quantiser launches included) beside the bf16-MFMA grouped tile kernel on the same tiles")
    ap.add_argument("--fused-router", action="store_true",
                    help="the router alone and the whole layer: ops.moe_gate_route beside F.linear + ops.moe_route "
                         "(default T = 1, 16, 64, 128, 256, 640, 2048, 8192)")
    ap.add_argument("--router-only", action="store_true", help="with --fused-router: no expert weights, no layer timing")
    ap.add_argument("--d", type=int, default=4096, help="model width (Mixtral-8x7B 4096, 8x22B 6144)")
    args = ap.parse_args()
    if args.fused_router and args.Ts == ap.get_default("Ts"):
        args.Ts = "1,16,64,128,256,640,2048,8192"
    if args.tiles_only and args.Ts == ap.get_default("Ts"):
        args.Ts = "1024,2048,4096,8192"
    Ts = [int(x) for x in args.Ts.split(",")]
    wd = args.weight_dtype
    dev = torch.device("cuda:0")
    E, K, d, F = 8, 2, args.d, 14336
    torch.manual_seed(0)
    router = (torch.randn(E, d, device=dev) * d ** -0.5).to(torch.bfloat16)
    if args.fused_router and args.router_only:
        return fused_router(Ts, dev, E, K, d, router, None)
    w13 = (torch.randn(E, 2 * F, d, device=dev) * d ** -0.5).to(torch.bfloat16)
    w2 = (torch.randn(E, d, F, device=dev) * F ** -0.5).to(torch.bfloat16)
    if args.compare:
        fmts = [ops.weight_format(f).name for f in args.compare.split(",")]
        if any(T > 512 for T in Ts):
            ap.error("--compare times the streaming kernel: T <= 512")
        return compare(Ts, fmts, dev, E, K, d, F, router, w13, w2)
    if args.act_dtype == "mxfp8":
        if not (args.tiles_only and wd == "mxfp4"):
            ap.error("--act-dtype mxfp8 needs --tiles-only --weight-dtype mxfp4")
        return tiles_act_mx(Ts, dev, E, K, d, F, router, w13, w2)
    if args.act_dtype == "fp8":
        if not (args.tiles_only and wd == "fp8"):
            ap.error("--act-dtype fp8 needs --tiles-only --weight-dtype fp8")
        return tiles_act_f8(Ts, dev, E, K, d, F, router, w13, w2)
    if args.tiles_only:
        return tiles_only(Ts, wd, dev, E, K, d, F, router, w13, w2)
    # (tiles, scales or None) in the grouped weight-streaming layout; quantised: w13 / w2 become the dequantised experts
    # the LDS-tiled grouped GEMM reads
    (w13t, w13s), (w2t, w2s) = ops.tile_experts_as(w13, wd, True), ops.tile_experts_as(w2, wd)
    if w13s is not None:
        w13, w2 = ops.untile_experts_as(w13t, w13s, True), ops.untile_experts_as(w2t, w2s)
    if args.fused_router:
        def layer_of(x, r):
            T = x.shape[0]
            out = torch.zeros(T, d, dtype=torch.float32, device=dev)
            if T <= 640:
                a = ops.grouped_stream_glu(x, w13t, r, scale=w13s)
                return ops.grouped_stream_combine(a, w2t, r, T, out, scale=w2s)
            a = ops.silu_mul(ops.grouped_gemm(x, w13, r, gather=True))
            return ops.grouped_gemm(a, w2, r, gather=False, combine_out=out)

        return fused_router(Ts, dev, E, K, d, router, layer_of)
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
