"""``ops.grouped_tiles_glu`` / ``ops.grouped_tiles_combine`` (csrc/grouped_tile_gemm.hip): the expert MLP of prefill-sized
steps on the expert tiles of every format, against the fp32 reference on the dequantised experts.

Tolerances are the project's for this comparison (``_check_grouped_fp8`` / ``_check_grouped_mxfp4``: GLU atol 0.03 / rtol
0.02, combine 0.02 / 0.01): the reference runs on the same dequantised weights, so what is left is bf16 output rounding
and accumulation order. Weights follow the mxfp4 ``_experts`` recipe (a power of two per row and per 32-column block,
seeds differing per expert), so a tile or scale read for the global instead of the local expert fails. The two halves
take independent inputs: the combine's K is the GLU's F only where F % 256 == 0, and N % 128 == 64 needs F = 160."""
import functools

import pytest
import torch
from test_weight_fp8_moe import _cpu_routing
from test_weight_mxfp4 import _close
from test_weight_mxfp4_moe import _experts

from kafka_llm_service_amd import ops
from kafka_llm_service_amd.ops import reference as ref

BM = ops.GT_BM
FORMATS = ["bf16", "fp8", "mxfp4"]
# every row-tile edge in one routing, on the expert-parallel subset [1, 7) of 8 experts (experts 0 and 7 take each
# token's other pick): an empty segment, one row, a tile less one, a whole tile, a tile plus one, two tiles plus three
EDGE_LENS = [0, 1, BM - 1, BM, BM + 1, 2 * BM + 3]
# (routing, GLU K, F, combine N, combine K): N % 128 == 64 on both halves with a single K group of 256; K = 768; a random
# routing over all experts at K = 512 (8 stages: the 3-stage rings end mid-ring at 256 and 512, on the boundary at 768)
CASES = [("edges", 256, 160, 192, 256), ("edges", 768, 256, 256, 768), ("random", 512, 256, 384, 512)]


@functools.lru_cache(maxsize=None)
def _routing(kind):
    """(logits bf16 [T, E], e_lo, e_n): each token's two experts carry the logits 4 and 3, the others -8."""
    if kind == "random":
        torch.manual_seed(5)
        return torch.randn(700, 4).to(torch.bfloat16), 0, 4
    picks = [1 + i for i, n in enumerate(EDGE_LENS) for _ in range(n)]
    logits = torch.full((len(picks), 8), -8.0)
    for t, e in enumerate(picks):
        logits[t, e], logits[t, 7 * (t & 1)] = 4.0, 3.0
    return logits.to(torch.bfloat16), 1, 6


@functools.lru_cache(maxsize=None)
def _tiles(fmt, e_n, N, K, glu):
    """(tiles, scales, tiles' dequantised experts fp32 on the CPU) on the GPU, built once per shape."""
    w = _experts(e_n, N, K, seed=N + K, std=K ** -0.5, device=torch.device("cuda:0"))
    wt, st = ops.tile_experts_as(w, fmt, glu)
    return wt, st, ops.untile_experts_as(wt, st, glu).float().cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,Kg,F,Nc,Kc", CASES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_grouped_tiles_vs_reference(cuda, fmt, kind, Kg, F, Nc, Kc):
    logits, e_lo, e_n = _routing(kind)
    T = logits.shape[0]
    r = ops.moe_route(logits.to(cuda), 2)
    rc = _cpu_routing(r)
    eo = rc.expert_off.tolist()
    lo, hi = eo[e_lo], eo[e_lo + e_n]
    if kind == "edges":
        assert [eo[e_lo + i + 1] - eo[e_lo + i] for i in range(e_n)] == EDGE_LENS
    torch.manual_seed(9)
    x = torch.randn(T, Kg, device=cuda, dtype=torch.bfloat16)
    wt, st, deq = _tiles(fmt, e_n, 2 * F, Kg, True)
    y = ops.grouped_tiles_glu(x, wt, r, e_lo=e_lo, scale=st)
    h_ref = torch.zeros(2 * T, 2 * F)
    ref.grouped_gemm(x.cpu().float(), deq, rc.perm_tok, rc.perm_w, rc.expert_off, e_lo, True, h_ref, None)
    _close(y[lo:hi], ref.silu_mul(h_ref[lo:hi]), atol=0.03, rtol=0.02, msg=f"glu {fmt} {kind} K={Kg} F={F}")
    a = torch.randn(2 * T, Kc, device=cuda, dtype=torch.bfloat16)
    wt, st, deq = _tiles(fmt, e_n, Nc, Kc, False)
    out = torch.zeros(T, Nc, device=cuda)
    ops.grouped_tiles_combine(a, wt, r, T, out, e_lo=e_lo, scale=st)
    out_ref = torch.zeros(T, Nc)
    ref.grouped_gemm(a.cpu().float(), deq, rc.perm_tok, rc.perm_w, rc.expert_off, e_lo, False, None, out_ref)
    _close(out, out_ref, atol=0.02, rtol=0.01, msg=f"combine {fmt} {kind} N={Nc} K={Kc}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind,Kg,F", [c[:3] for c in CASES[:2]])
@pytest.mark.parametrize("fmt", FORMATS[1:])
def test_grouped_tiles_glu_bit_equals_bf16_tiles(cuda, fmt, kind, Kg, F):
    """Same B fragments (the dequantised values are exact in bf16), same MFMA order per accumulator, same epilogue."""
    logits, e_lo, e_n = _routing(kind)
    r = ops.moe_route(logits.to(cuda), 2)
    torch.manual_seed(9)
    x = torch.randn(logits.shape[0], Kg, device=cuda, dtype=torch.bfloat16)
    wt, st, _ = _tiles(fmt, e_n, 2 * F, Kg, True)
    yq = ops.grouped_tiles_glu(x, wt, r, e_lo=e_lo, scale=st)
    y16 = ops.grouped_tiles_glu(x, ops.tile_experts(ops.untile_experts_as(wt, st, True), glu=True), r, e_lo=e_lo)
    eo = r.expert_off.tolist()
    lo, hi = eo[e_lo], eo[e_lo + e_n]
    assert yq[lo:hi].float().abs().max() > 0 and torch.equal(yq[lo:hi], y16[lo:hi])


@pytest.mark.gpu
def test_grouped_tile_gemm_binding_refusals(cuda):
    from kafka_llm_service_amd.ops._ext import ext

    T, E = 8, 2
    r = ops.moe_route(torch.randn(T, E).to(torch.bfloat16).to(cuda), 2)
    y = torch.full((2 * T, 64), 7.0, device=cuda, dtype=torch.bfloat16)

    def refused(K, fmt, scale):
        w = _experts(E, 128, K, seed=3, device=cuda)
        wt, st = ops.tile_experts_as(w, fmt, True)
        sc = {"own": st, "none": None, "rows": torch.ones(E, 128, device=cuda)}[scale]
        x = torch.zeros(T, K, device=cuda, dtype=torch.bfloat16)
        with pytest.raises(RuntimeError):
            ext().grouped_tile_gemm(x, wt.view(torch.uint8) if fmt == "mxfp4" else wt,
                                    sc.view(torch.uint8) if fmt == "mxfp4" and sc is st else sc,
                                    ops.weight_format(fmt).abi, r.perm_tok, r.perm_w, r.expert_off, 0, True, y, None)

    refused(256, "fp8", "none")    # a quantised format without its scales
    refused(256, "mxfp4", "none")
    refused(256, "bf16", "rows")   # bf16 tiles with scales
    for fmt in FORMATS:
        refused(384, fmt, "own")   # K % 256 != 0
    torch.cuda.synchronize()
    assert (y == 7.0).all(), "a refused call wrote its output"


@pytest.mark.parametrize("fmt", FORMATS)
def test_grouped_tiles_cpu_equals_grouped_stream_cpu(fmt):
    T, d, F, E, e_lo, e_n = 9, 512, 256, 8, 2, 4
    g = torch.Generator().manual_seed(4)
    x = torch.randn(T, d, generator=g).to(torch.bfloat16)
    r = ops.moe_route(torch.randn(T, E, generator=g).to(torch.bfloat16), 2)
    w13t, w13s = ops.tile_experts_as(_experts(e_n, 2 * F, d, seed=5), fmt, True)
    w2t, w2s = ops.tile_experts_as(_experts(e_n, d, F, seed=6), fmt)
    a = ops.grouped_tiles_glu(x, w13t, r, e_lo=e_lo, scale=w13s)
    eo = r.expert_off.tolist()
    lo, hi = eo[e_lo], eo[e_lo + e_n]
    assert hi > lo and torch.equal(a[lo:hi], ops.grouped_stream_glu(x, w13t, r, e_lo=e_lo, scale=w13s)[lo:hi])
    a[:lo].zero_()  # (rows of the other ranks' experts are undefined: the combine does not read them)
    a[hi:].zero_()
    out, out_s = torch.zeros(T, d), torch.zeros(T, d)
    ops.grouped_tiles_combine(a, w2t, r, T, out, e_lo=e_lo, scale=w2s)
    ops.grouped_stream_combine(a, w2t, r, T, out_s, e_lo=e_lo, scale=w2s)
    assert out.abs().max() > 0 and torch.equal(out, out_s)
    if fmt != "bf16":
        with pytest.raises(ValueError):
            ops.grouped_tiles_glu(x, w13t, r, e_lo=e_lo)  # quantised tiles without their scales
