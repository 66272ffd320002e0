"""Dense tile GEMM (csrc/tile_gemm.hip, ops.linear_tiles) on the Llama-3-8B / 70B projections at prefill row counts,
in every tile format, against yardsticks from outside the code under test:
  (a) blas_copy:   F.linear on the stored (dequantised) bf16 row-major copy (+ silu_mul for gate_up): a two-copy model;
  (b) untile_blas: ops.untile_weight_as + F.linear (+ silu_mul): what a tiled-only model does today on such a step;
  (c) grouped:     gate_up only, ops.grouped_tiles_glu with one expert and an identity routing (the 2 x 2-block kernel).
Interleaved rounds: every round times all paths of a cell back to back, so a comparison holds only where it has the
same sign in every round by more than the cell moves between rounds. ``--act-dtype mxfp8`` (MXFP4 tiles only) adds the
scaled-MFMA path of csrc/tile_gemm_mx.hip: ``mx`` = ops.linear_tiles(act="mxfp8"), the quantiser's launch included,
``mx_gemm`` = the GEMM alone on activations quantised beforehand, ``quant`` = the quantiser alone. ``--act-dtype fp8`` (fp8 tiles only) does the same for the e4m3 x e4m3 path of
csrc/tile_gemm_f8.hip (``f8``, ``f8_gemm``, ``quant``), beside the bf16-MFMA kernel on the same fp8 tiles (``tiles``) and
hipBLASLt on the dequantised copy (``blas_copy``). Each timed call of a path reads another copy of
the weight (>= 600 MB rotated, so the MALL does not serve repeats). One JSON line per (round, cell); TFLOP/s over
2 M N K.
``--fused-quant`` (with ``--act-dtype mxfp8|fp8``) times instead the chains of a layer with and without the fused
quantisers (models/llama.py FUSE_ACT_QUANT): ``norm_qkv`` / ``norm_gate_up`` = fused_add_rmsnorm -> quantiser -> GEMM
against the quantising norm -> GEMM, and under mxfp8 ``glu_down`` = gate_up + GLU -> quantiser -> down against the
quantising epilogue -> down. One JSON line per (round, cell) with ``unfused_us`` and ``fused_us``."""
import argparse
import json

import torch
import torch.nn.functional as F

from kafka_llm_service_amd import ops

# (name, N, K, glu) at TP = 1
MODELS = {"8b": [("qkv", 6144, 4096, False), ("o", 4096, 4096, False), ("gate_up", 28672, 4096, True),
                 ("down", 4096, 14336, False)],
          "70b": [("qkv", 10240, 8192, False), ("o", 8192, 8192, False), ("gate_up", 57344, 8192, True),
                  ("down", 8192, 28672, False)]}


def timeit(fn, iters):
    for i in range(2):
        fn(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def identity_routing(M, dev):
    """One expert that owns every row, each row routed to itself with weight 1 (the router's stable order)."""
    return ops.moe_route(torch.zeros(M, 1, dtype=torch.bfloat16, device=dev), 1)


def fused_quant(args, dev="cuda"):
    act, fmt = args.act_dtype, ops.ACT_TILES[args.act_dtype]
    quant = ops.mxfp8_quant if act == "mxfp8" else ops.fp8_act_quant

    def tiles(N, K, glu):  # >= 600 MB of copies of one projection, rotated by the timed calls
        n = max(2, (600 << 20) // ops.tiled_weight_bytes((N, K), fmt) + 1)
        return [ops.tile_weight_as((torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16), fmt, glu) for _ in range(n)]

    for model in args.models.split(","):
        shp = {name: (N, K, glu) for name, N, K, glu in MODELS[model]}
        d = shp["qkv"][1]
        nw = torch.ones(d, dtype=torch.bfloat16, device=dev)
        cells = [("norm_" + g, g) for g in ("qkv", "gate_up") if g in args.gemms.split(",")]
        if act == "mxfp8" and "down" in args.gemms.split(","):
            cells.append(("glu_down", "gate_up"))
        for cell, g in cells:
            N, K, glu = shp[g]
            wts = tiles(N, K, glu)
            dts = tiles(*shp["down"]) if cell == "glu_down" else None
            for M in (int(m) for m in args.rows.split(",")):
                delta, res = ((torch.randn(M, d, device=dev) * 0.5).to(torch.bfloat16) for _ in range(2))
                lin = lambda x, w, **kw: ops.linear_tiles(x, w[0], scale=w[1], act=act, **kw)
                if cell == "glu_down":
                    xq, xe = quant(delta)
                    paths = {"unfused": lambda i: lin(lin(xq, wts[i % len(wts)], glu=True, x_scale=xe), dts[i % len(dts)]),
                             "fused": lambda i: (lambda a: lin(a[0], dts[i % len(dts)], x_scale=a[1]))(
                                 lin(xq, wts[i % len(wts)], glu=True, x_scale=xe, quant_out=True))}
                else:
                    paths = {"unfused": lambda i: lin(ops.fused_add_rmsnorm(delta, res, nw, 1e-5), wts[i % len(wts)], glu=glu),
                             "fused": lambda i: (lambda a: lin(a[0], wts[i % len(wts)], glu=glu, x_scale=a[1]))(
                                 ops.fused_add_rmsnorm(delta, res, nw, 1e-5, quant=act))}
                for rnd in range(args.rounds):
                    us = {k: timeit(fn, args.iters) for k, fn in paths.items()}
                    print(json.dumps({"model": model, "cell": cell, "act_dtype": act, "M": M, "N": N, "K": K, "round": rnd,
                                      "unfused_us": round(us["unfused"], 1), "fused_us": round(us["fused"], 1),
                                      "gain_pct": round(100 * (1 - us["fused"] / us["unfused"]), 2)}), flush=True)
            del wts, dts
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="8b,70b")
    ap.add_argument("--formats", default="bf16,fp8,mxfp4")
    ap.add_argument("--rows", default="512,1024,2048,4096,8192")
    ap.add_argument("--gemms", default="qkv,o,gate_up,down")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--act-dtype", default="bf16", choices=ops.ACT_DTYPES)
    ap.add_argument("--fused-quant", action="store_true")
    args = ap.parse_args()
    if args.fused_quant:
        if args.act_dtype == "bf16" or not torch.cuda.is_available():
            raise SystemExit("--fused-quant needs --act-dtype mxfp8 or fp8 and a GPU")
        return fused_quant(args)
    mx = args.act_dtype == "mxfp8"
    qa = args.act_dtype != "bf16"  # quantised activations: "mx" on the mxfp4 tiles, "f8" on the fp8 tiles
    tag = "mx" if mx else "f8"
    if qa:
        args.formats = ops.ACT_TILES[args.act_dtype]
    if not torch.cuda.is_available():
        raise SystemExit("tile_gemm_bench needs a GPU")
    dev = "cuda"
    rows = [int(m) for m in args.rows.split(",")]
    for model in args.models.split(","):
        for name, N, K, glu in MODELS[model]:
            if name not in args.gemms.split(","):
                continue
            for fmt in args.formats.split(","):
                copies = max(2, (600 << 20) // ops.tiled_weight_bytes((N, K), fmt) + 1)
                qs, deqs = [], []
                for _ in range(copies):
                    w = (torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16)
                    qs.append(ops.tile_weight_as(w, fmt, glu))
                    deqs.append(ops.untile_weight_as(*qs[-1], glu))
                    del w
                act = ops.silu_mul if glu else (lambda y: y)
                for M in rows:
                    x = (torch.randn(M, K, device=dev) * 0.5).to(torch.bfloat16)
                    route = identity_routing(M, dev) if glu else None
                    S = ops.tile_gemm_plan(M, N, K, 1 if glu else 8)
                    paths = {"tiles": lambda i: ops.linear_tiles(x, qs[i % copies][0], glu=glu, scale=qs[i % copies][1]),
                             "blas_copy": lambda i: act(F.linear(x, deqs[i % copies])),
                             "untile_blas": lambda i: act(F.linear(x, ops.untile_weight_as(*qs[i % copies], glu)))}
                    if qa:
                        quant = ops.mxfp8_quant if mx else ops.fp8_act_quant
                        xq, xe = quant(x)
                        raw = [(q[0].view(torch.uint8), q[1].view(torch.uint8)) for q in qs] if mx else qs
                        gemm = ops.ext().tile_gemm_mx if mx else ops.ext().tile_gemm_f8

                        def q_gemm(i):
                            y = torch.empty(M, N // 2 if glu else N, dtype=x.dtype, device=dev) if S == 1 else None
                            p = torch.empty(S, M, N, dtype=torch.float32, device=dev) if S > 1 else None
                            gemm(xq, xe.view(torch.uint8) if mx else xe, *raw[i % copies], y, p, S, glu)

                        paths = {"tiles": paths["tiles"], "blas_copy": paths["blas_copy"], tag + "_gemm": q_gemm,
                                 tag: lambda i: ops.linear_tiles(x, qs[i % copies][0], glu=glu, scale=qs[i % copies][1],
                                                                 act=args.act_dtype),
                                 "quant": lambda i: quant(x)}
                    elif glu:
                        paths["grouped"] = lambda i: ops.grouped_tiles_glu(
                            x, qs[i % copies][0][None], route, scale=None if qs[i % copies][1] is None
                            else qs[i % copies][1][None])
                    for rnd in range(args.rounds):
                        us = {k: timeit(fn, args.iters) for k, fn in paths.items()}
                        line = {"model": model, "gemm": name, "weight_dtype": fmt, "M": M, "N": N, "K": K, "splits": S,
                                "round": rnd}
                        for k, t in us.items():
                            line[k + "_us"] = round(t, 1)
                            if k != "quant":
                                line[k + "_TFLOP/s"] = round(2.0 * M * N * K / t / 1e6, 1)
                        print(json.dumps(line), flush=True)
                del qs, deqs
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
