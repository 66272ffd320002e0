"""``ops.linear_tiles`` (csrc/tile_gemm.hip): y = x . W^T for any row count from the wave tiles of every format, and the
``tile_prefill`` mode in which a dense model lives in its tiles alone.

Tolerances are the project's for these comparisons, unchanged: the float64 product with the dequantised weight at
atol = rtol = 2e-2 (tests/test_skinny_quant.py), the activated GLU output at atol 0.03 / rtol 0.02 (``_close``,
tests/test_grouped_tiles.py), greedy tokens within 0.15 (CPU) / 0.25 (GPU) logits of the dense oracle. Weights carry a
power of two per row (and, for bf16 and mxfp4 tiles, per 32-column block), so a wrong scale, block or tile fails."""
import dataclasses
import functools

import pytest
import torch
from test_weight_fp8 import _weight as _weight_rows
from test_weight_mxfp4 import _assert_greedy_gap, _close, _cpu_cfg
from test_weight_mxfp4 import _weight as _weight_blocks

from kafka_llm_service_amd import ops
from kafka_llm_service_amd.ops import reference as ref

FORMATS = ["bf16", "fp8", "mxfp4"]
# (M, N, K, glu, max_splits). M: one row, a tile less one, a whole tile, a tile plus one, two tiles plus three. N: a lone
# pair, a full block plus a 64 tail, two blocks. K: the 3-stage rings end mid-ring (256) / on their boundary (768).
CASES = [(1, 64, 256, False, 1), (255, 320, 768, False, 1), (256, 512, 256, False, 1), (257, 64, 768, False, 1),
         (515, 320, 256, False, 1), (515, 512, 768, False, 8), (257, 320, 2048, False, 8), (1, 512, 2048, False, 8),
         (1, 64, 256, True, 8), (255, 320, 768, True, 1), (256, 64, 768, True, 1), (257, 512, 256, True, 1),
         (515, 320, 768, True, 8)]


@functools.lru_cache(maxsize=None)
def _case(fmt, N, K, glu):
    """(x [515, K] * 0.5 on the GPU, tiles, scale, the tiles' dequantised weight in float64 on the CPU)"""
    dev = torch.device("cuda:0")
    w = (_weight_rows if fmt == "fp8" else _weight_blocks)(N, K, seed=N + K + glu, device=dev)
    wt, s = ops.tile_weight_as(w, fmt, glu)
    x = (torch.randn(515, K, generator=torch.Generator().manual_seed(K)) * 0.5).to(torch.bfloat16).to(dev)
    return x, wt, s, ops.untile_weight_as(wt, s, glu).double().cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,glu,ms", CASES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_linear_tiles_vs_float64(cuda, fmt, M, N, K, glu, ms):
    x515, wt, s, deq = _case(fmt, N, K, glu)
    x = x515[:M]
    S = ops.tile_gemm_plan(M, N, K, 1 if glu else ms)
    assert (S > 1) == (K == 2048) and S == ops._ext.load().tile_gemm_plan(M, N, K, 1 if glu else ms)
    y = ops.linear_tiles(x, wt, max_splits=ms, glu=glu, scale=s)
    want = x.double().cpu() @ deq.t()
    if glu:
        assert y.dtype == torch.bfloat16 and y.shape == (M, N // 2)
        _close(y, ref.silu_mul(want), atol=0.03, rtol=0.02, msg=f"glu {fmt} M={M} N={N} K={K}")
        return
    assert y.shape == ((S, M, N) if S > 1 else (M, N)) and ops.is_slab(y) == (S > 1)
    torch.testing.assert_close(ops.slab_reduce(y).double().cpu(), want, atol=2e-2, rtol=2e-2)


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,glu,ms", [(257, 320, 768, False, 1), (515, 320, 768, True, 1), (257, 320, 2048, False, 8)])
@pytest.mark.parametrize("fmt", FORMATS[1:])
def test_linear_tiles_bit_equals_bf16_tiles(cuda, fmt, M, N, K, glu, ms):
    """Same B fragments (the dequantised values are exact in bf16), same MFMA order per accumulator, same epilogue."""
    x515, wt, s, _ = _case(fmt, N, K, glu)
    yq = ops.linear_tiles(x515[:M], wt, max_splits=ms, glu=glu, scale=s)
    y16 = ops.linear_tiles(x515[:M], ops.tile_weight(ops.untile_weight_as(wt, s, glu), glu), max_splits=ms, glu=glu)
    assert ops.is_slab(yq) == (ms > 1) and yq.float().abs().max() > 0 and torch.equal(yq, y16)


@pytest.mark.gpu
def test_tile_gemm_binding_refusals(cuda):
    tg = ops._ext.load().tile_gemm
    x = torch.zeros(300, 512, device=cuda, dtype=torch.bfloat16)
    y = torch.full((300, 128), 7.0, device=cuda, dtype=torch.bfloat16)
    p = torch.full((2, 300, 128), 7.0, device=cuda)
    w = _weight_blocks(128, 512, device=cuda)
    (w16, _), (w8, s8), (w4, s4) = (ops.tile_weight_as(w, f, True) for f in FORMATS)
    w4, s4 = w4.view(torch.uint8), s4.view(torch.uint8)
    for args in [(x, w8, y, None, 1, False, None, 1),           # a quantised format without its scales
                 (x, w16, y, None, 1, False, s8, 0),            # bf16 tiles with scales
                 (x, w8, y, None, 1, False, s8, 2),             # fp8 tiles and scales named mxfp4
                 (x, w4, y, None, 1, False, s4, 1),             # mxfp4 tiles and image named fp8
                 (x[:, :256], w16, y, None, 1, False, None, 0),             # a wrong K
                 (x[:, :384], w16[:, :24].contiguous(), y, None, 1, False, None, 0),  # K % 256 != 0
                 (torch.zeros(300, 513, device=cuda, dtype=x.dtype)[:, :512], w16, y, None, 1, False, None, 0),  # ldx
                 (x, w16, y[:, :64], p, 2, True, None, 0),      # GLU with two splits
                 (x, w16, y, None, 2, False, None, 0)]:         # two splits without slabs
        with pytest.raises(RuntimeError):
            tg(*args)
    torch.cuda.synchronize()
    assert (y == 7.0).all() and (p == 7.0).all(), "a refused call wrote its output"


@pytest.mark.parametrize("fmt", FORMATS)
def test_tile_prefill_model_cpu(fmt, monkeypatch):
    """A 300-token prefill and decode steps of a tiny Llama that lives in its tiles alone: every projection of more
    than stream_max_m rows goes through linear_tiles, nothing is untiled, and the tokens stay within the CPU oracle gap."""
    from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
    from kafka_llm_service_amd.engine.sequence import SamplingParams
    from kafka_llm_service_amd.models.config import get_config
    from kafka_llm_service_amd.models.oracle import dense_logits
    from kafka_llm_service_amd.models.weights import build_model
    from kafka_llm_service_amd.parallel import state as pstate

    for env in ("KAFKA_WEIGHT_DTYPE", "KAFKA_DECODE_GEMM", "KAFKA_TILE_PREFILL"):
        monkeypatch.delenv(env, raising=False)
    monkeypatch.setattr(ops, "STREAM_MAX_M", 128)
    both = LLMEngine(EngineConfig(**_cpu_cfg(weight_dtype=fmt, decode_gemm="stream")))
    eng = LLMEngine(EngineConfig(**_cpu_cfg(weight_dtype=fmt, tile_prefill=True)))
    m = eng.model
    assert m.tile_prefill and not m.tiled_only and m.stream_max_m == 128 and eng.sched.cfg.step_rows_fit == 0
    assert m.lm_head is None and all(lw.qkv is None and lw.o is None and lw.gate_up is None and lw.down is None
                                     for lw in m.layers)
    assert m.weight_bytes() < both.model.weight_bytes()
    assert torch.equal(m.layers[1].down_t.view(torch.uint8), both.model.layers[1].down_t.view(torch.uint8))
    calls, untiled, tiles, untile = [], [], ops.linear_tiles, ops.untile_weight_as
    monkeypatch.setattr(ops, "linear_tiles", lambda x, wt, *a, **k: (
        calls.append((x.shape[0], bool(k.get("glu")), wt.dtype)), tiles(x, wt, *a, **k))[1])
    monkeypatch.setattr(ops, "untile_weight_as", lambda *a, **k: (untiled.append(1), untile(*a, **k))[1])
    monkeypatch.setattr(pstate, "tp_linear_all_reduce", lambda *a, **k: pytest.fail("pipelined seam without a copy"))
    prompts = [torch.randint(0, 5000, (300,), generator=torch.Generator().manual_seed(3)).tolist()]
    outs = eng.generate(prompts, SamplingParams(temperature=0.0, max_tokens=3, ignore_eos=True))
    L = len(m.layers)
    assert len(calls) == 4 * L and not untiled and all(r == 300 and dt == m.layers[0].qkv_t.dtype for r, _, dt in calls)
    assert sum(glu for _, glu, _ in calls) == L  # gate_up with its fused SwiGLU, once per layer
    assert not m._can_pipe(4096, None, m.layers[0].o_t) and both.model._can_pipe(4096, both.model.layers[0].o, None)
    monkeypatch.setattr(ops, "untile_weight_as", untile)
    _assert_greedy_gap(m, prompts, outs, 0.15)
    assert torch.equal(dense_logits(m, prompts[0][:40]), dense_logits(both.model, prompts[0][:40]))
    # a streamed projection the dense tile GEMM does not cover (lm_head N % 64 == 32) is an error, as is the combination
    # with expert_tiles_only
    odd = dataclasses.replace(get_config("tiny-llama"), vocab_size=5024)
    with pytest.raises(ValueError, match="tile_prefill"):
        build_model(odd, "cpu").enable_stream_weights(weight_dtype=fmt, tile_prefill=True)
    with pytest.raises(ValueError, match="tile_prefill"):
        build_model(get_config("tiny-mixtral"), "cpu").enable_stream_weights(tile_prefill=True, expert_tiles_only=True)
    monkeypatch.setenv("KAFKA_TILE_PREFILL", "1")  # the environment turns the mode on for a default config
    assert LLMEngine(EngineConfig(**_cpu_cfg(weight_dtype=fmt))).model.tile_prefill


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["bf16", "mxfp4"])
def test_tile_prefill_engine_gpu(cuda, fmt, monkeypatch):
    """One prompt of more than 256 tokens with nothing decoding (the first step runs the dense tile GEMM), then 8 greedy
    decode steps on the streaming kernel; the bound of the expert-tiles-only engine test."""
    from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
    from kafka_llm_service_amd.engine.sequence import SamplingParams

    for env in ("KAFKA_WEIGHT_DTYPE", "KAFKA_DECODE_GEMM", "KAFKA_TILE_PREFILL"):
        monkeypatch.delenv(env, raising=False)
    rows, tiles = [], ops.linear_tiles
    monkeypatch.setattr(ops, "linear_tiles", lambda x, *a, **k: (rows.append(x.shape[0]), tiles(x, *a, **k))[1])
    e = LLMEngine(EngineConfig(model="small-llama", device=str(cuda), num_kv_blocks=1024, max_model_len=4096,
                               weight_dtype=fmt, tile_prefill=True))
    assert e.model.tile_prefill and e.model.lm_head is None and all(lw.qkv is None for lw in e.model.layers)
    prompts = [torch.randint(0, 5000, (333,), generator=torch.Generator().manual_seed(3)).tolist()]
    outs = e.generate(prompts, SamplingParams(temperature=0.0, max_tokens=9, ignore_eos=True))
    assert len(rows) == 4 * len(e.model.layers) and min(rows) == 333, rows
    _assert_greedy_gap(e.model, prompts, outs, 0.25)
