"""MXFP8 activations on the MXFP4 tiles (csrc/tile_gemm_mx.hip): the quantiser ``ops.mxfp8_quant`` against its CPU
reference bit for bit, ``ops.linear_tiles(..., act="mxfp8")`` on the scaled fp8 x fp4 MFMA against the float64 product
of the same quantised operands, and the ``act_dtype="mxfp8"`` engine mode.

Tolerances are those of tests/test_tile_gemm.py, unchanged: both sides of a GEMM comparison use the same quantised
operands, so only the fp32 accumulation order and the bf16 output rounding differ. Activations carry a power of two per
(row, 32-column block) and the weights one per row and block, so a wrong scale block, scale byte, K order inside a
block or nibble order fails."""
import functools

import pytest
import torch
from test_weight_mxfp4 import _assert_greedy_gap, _close, _cpu_cfg
from test_weight_mxfp4 import _weight as _weight_blocks

from kafka_llm_service_amd import ops
from kafka_llm_service_amd.ops import reference as ref

# (M, N, K, glu, max_splits): the edge set of tests/test_tile_gemm.py. K = 256 ends the ring of three 128-deep stages
# mid-ring (two stages), K = 768 on its boundary (six).
CASES = [(1, 64, 256, False, 1), (255, 320, 768, False, 1), (256, 512, 256, False, 1), (257, 64, 768, False, 1),
         (515, 320, 256, False, 1), (515, 512, 768, False, 8), (257, 320, 2048, False, 8), (1, 512, 2048, False, 8),
         (1, 64, 256, True, 1), (255, 320, 768, True, 1), (257, 512, 256, True, 1), (515, 320, 768, True, 1)]


def _acts(M, K, seed=0):
    """bf16 [M, K]: a seeded normal times a power of two per (row, 32-column block) in 2^-6..2^6; row 0 starts with an
    all-zero block, then blocks whose amax is exactly 448 * 2^-3, the next bf16 above it and the next bf16 below it."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K // 32, 32, generator=g) * torch.exp2(torch.randint(-6, 7, (M, K // 32, 1), generator=g).float())
    x[0, :4] = x[0, :4].clamp(-1, 1)
    x[0, 0] = 0
    x[0, 1, 5], x[0, 2, 9], x[0, 3, 2] = 56.0, -56.25, 55.75
    return x.view(M, K).to(torch.bfloat16)


@pytest.mark.gpu
@pytest.mark.parametrize("M,K,pad", [(1, 256, 0), (37, 768, 8), (257, 2048, 0)])
def test_mxfp8_quant_gpu_equals_reference(cuda, M, K, pad):
    x = _acts(M, K, seed=M)
    xg = torch.zeros(M, K + pad, dtype=torch.bfloat16, device=cuda)[:, :K]  # (pad: a row view with ldx > K)
    xg.copy_(x)
    xq, xe = ops.mxfp8_quant(xg)
    wq, we = ref.mxfp8_quant(x)
    assert xe.dtype == torch.float8_e8m0fnu and we.view(torch.uint8)[0, :4].tolist() == [127, 125, 125, 124]
    assert torch.equal(xe.view(torch.uint8).cpu(), we.view(torch.uint8)) and torch.equal(xq.cpu(), wq)


@functools.lru_cache(maxsize=None)
def _case(N, K, glu):
    """(x [515, K] on the GPU, its dequantised MXFP8 values in float64, tiles, image, the dequantised weight in float64)"""
    dev = torch.device("cuda:0")
    wt, s = ops.tile_weight_as(_weight_blocks(N, K, seed=N + K + glu, device=dev), "mxfp4", glu)
    x = _acts(515, K, seed=K)
    return x.to(dev), ref.mxfp8_dequant(*ref.mxfp8_quant(x)).double(), wt, s, ops.untile_weight_as(wt, s, glu).double().cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,glu,ms", CASES)
def test_linear_tiles_mxfp8_vs_float64(cuda, M, N, K, glu, ms):
    x515, xd, wt, s, deq = _case(N, K, glu)
    S = ops.tile_gemm_plan(M, N, K, 1 if glu else ms)
    assert (S > 1) == (K == 2048)
    y = ops.linear_tiles(x515[:M], wt, max_splits=ms, glu=glu, scale=s, act="mxfp8")
    want = xd[:M] @ deq.t()
    assert y.float().abs().max() > 0
    if glu:
        assert y.dtype == torch.bfloat16 and y.shape == (M, N // 2)
        _close(y, ref.silu_mul(want), atol=0.03, rtol=0.02, msg=f"glu M={M} N={N} K={K}")
        return
    assert y.shape == ((S, M, N) if S > 1 else (M, N)) and ops.is_slab(y) == (S > 1)
    torch.testing.assert_close(ops.slab_reduce(y).double().cpu(), want, atol=2e-2, rtol=2e-2)


@pytest.mark.gpu
def test_mxfp8_refusals(cuda):
    e = ops._ext.load()
    w = _weight_blocks(128, 512, device=cuda)
    (w16, _), (w8, s8), (w4, s4) = (ops.tile_weight_as(w, f, True) for f in ("bf16", "fp8", "mxfp4"))
    x = torch.zeros(300, 512, device=cuda, dtype=torch.bfloat16)
    for wt, sc, name in ((w16, None, "bf16"), (w8, s8, "fp8")):
        with pytest.raises(ValueError, match=name):
            ops.linear_tiles(x, wt, scale=sc, act="mxfp8")
    w4, s4 = w4.view(torch.uint8), s4.view(torch.uint8)
    u8 = dict(device=cuda, dtype=torch.uint8)
    xq, xe = torch.full((300, 512), 7, **u8), torch.full((300, 16), 7, **u8)
    y = torch.full((300, 128), 7.0, device=cuda, dtype=torch.bfloat16)
    p = torch.full((2, 300, 128), 7.0, device=cuda)
    for args in [(x, xq, xe[:, :8].contiguous()),                                   # a wrong xe shape
                 (x[:, :384], xq[:, :384].contiguous(), xe[:, :12].contiguous()),  # K % 256 != 0
                 (torch.zeros(300, 513, device=cuda, dtype=x.dtype)[:, :512], xq, xe)]:  # ldx
        with pytest.raises(RuntimeError):
            e.act_quant_mxfp8(*args)
    for args in [(xq, xe[:, :8].contiguous(), w4, s4, y, None, 1, False),
                 (xq[:, :384], xe[:, :12].contiguous(), w4[:, :6].contiguous(), s4[:, :6].contiguous(), y, None, 1, False),
                 (xq, xe, w4, s4, y[:, :64], p, 2, True),                           # GLU with two splits
                 (torch.zeros(300, 520, **u8)[:, :512], xe, w4, s4, y, None, 1, False)]:  # ldxq % 16 != 0
        with pytest.raises(RuntimeError):
            e.tile_gemm_mx(*args)
    torch.cuda.synchronize()
    assert all((t == 7).all() for t in (xq, xe, y, p)), "a refused call wrote its output"


def _engine(monkeypatch, **kw):
    from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine

    eng = LLMEngine(EngineConfig(**kw))
    calls, tiles = [], ops.linear_tiles
    monkeypatch.setattr(ops, "linear_tiles", lambda x, *a, **k: (calls.append((x.shape[0], k.get("act", "bf16"))),
                                                                 tiles(x, *a, **k))[1])
    return eng, calls


def test_act_mxfp8_engine_cpu(monkeypatch):
    """A 300-token prefill and two decode steps of a tiny Llama in MXFP4 tiles with MXFP8 prefill activations. The CPU
    path contains no kernel: the greedy gap it keeps is the format's (the project's 0.15 holds; measured 0.000)."""
    from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
    from kafka_llm_service_amd.engine.sequence import SamplingParams

    for env in ("KAFKA_WEIGHT_DTYPE", "KAFKA_DECODE_GEMM", "KAFKA_TILE_PREFILL", "KAFKA_ACT_DTYPE"):
        monkeypatch.delenv(env, raising=False)
    monkeypatch.setattr(ops, "STREAM_MAX_M", 128)
    for kw in (dict(weight_dtype="bf16", tile_prefill=True), dict(weight_dtype="fp8", tile_prefill=True),
               dict(weight_dtype="mxfp4")):
        with pytest.raises(ValueError, match="act_dtype"):
            LLMEngine(EngineConfig(**_cpu_cfg(act_dtype="mxfp8", **kw)))
    eng, calls = _engine(monkeypatch, **_cpu_cfg(weight_dtype="mxfp4", tile_prefill=True, act_dtype="mxfp8"))
    assert eng.model.act_dtype == "mxfp8"
    prompts = [torch.randint(0, 5000, (300,), generator=torch.Generator().manual_seed(3)).tolist()]
    outs = eng.generate(prompts, SamplingParams(temperature=0.0, max_tokens=3, ignore_eos=True))
    # every layer's four projections with 300 rows; the lm_head's rows and the decode steps never
    assert [c for c in calls if c[1] == "mxfp8"] == [(300, "mxfp8")] * (4 * len(eng.model.layers))
    assert all(rows < 300 for rows, act in calls if act == "bf16")
    _assert_greedy_gap(eng.model, prompts, outs, 0.15)
    monkeypatch.setenv("KAFKA_ACT_DTYPE", "mxfp8")  # the environment turns the mode on for a default config
    assert LLMEngine(EngineConfig(**_cpu_cfg(weight_dtype="mxfp4", tile_prefill=True))).model.act_dtype == "mxfp8"


@pytest.mark.gpu
def test_act_mxfp8_engine_gpu(cuda, monkeypatch):
    """One 333-token prompt (the first step's projections run the scaled-MFMA kernel), then 8 greedy decode steps on the
    streaming kernel; the bound of test_tile_prefill_engine_gpu."""
    from kafka_llm_service_amd.engine.sequence import SamplingParams

    for env in ("KAFKA_WEIGHT_DTYPE", "KAFKA_DECODE_GEMM", "KAFKA_TILE_PREFILL", "KAFKA_ACT_DTYPE"):
        monkeypatch.delenv(env, raising=False)
    mx, gemm = [], ops._ext.load().tile_gemm_mx
    monkeypatch.setattr(ops._ext.load(), "tile_gemm_mx", lambda xq, *a: (mx.append(xq.shape[0]), gemm(xq, *a))[1])
    e, calls = _engine(monkeypatch, model="small-llama", device=str(cuda), num_kv_blocks=1024, max_model_len=4096,
                       weight_dtype="mxfp4", tile_prefill=True, act_dtype="mxfp8")
    prompts = [torch.randint(0, 5000, (333,), generator=torch.Generator().manual_seed(3)).tolist()]
    outs = e.generate(prompts, SamplingParams(temperature=0.0, max_tokens=9, ignore_eos=True))
    assert mx == [333] * (4 * len(e.model.layers)) and [c for c in calls if c[1] == "mxfp8"] == [(333, "mxfp8")] * len(mx)
    _assert_greedy_gap(e.model, prompts, outs, 0.25)
