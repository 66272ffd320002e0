"""fp8 activations on the fp8 tiles (csrc/tile_gemm_f8.hip): the per-row quantiser ``ops.fp8_act_quant`` against
``reference.fp8_quant`` bit for bit, ``ops.linear_tiles(..., act="fp8")`` on the e4m3 x e4m3 MFMA against the float64
product of the same quantised operands, and the ``act_dtype="fp8"`` engine mode.

Tolerances are those of tests/test_tile_gemm.py, unchanged: both sides of a GEMM comparison use the same quantised
operands, so only the fp32 accumulation order and the bf16 output rounding differ. Activations carry a power of two per
row and the weights one per row (GLU tiles included), so a wrong row exponent, a scale read in natural instead of tile
order or a K order that differs between the operands fails."""
import functools

import pytest
import torch
from test_weight_fp8 import _weight as _weight_rows
from test_weight_mxfp4 import _assert_greedy_gap, _close, _cpu_cfg

from kafka_llm_service_amd import ops
from kafka_llm_service_amd.ops import reference as ref

# (M, N, K, glu, max_splits): the edge set of tests/test_tile_gemm.py. The ring has five 64-deep stages: K = 256 never
# wraps (four stages), K = 768 ends mid-ring (twelve), K = 1280 on the ring's boundary (twenty).
CASES = [(1, 64, 256, False, 1), (255, 320, 768, False, 1), (256, 512, 256, False, 1), (257, 64, 768, False, 1),
         (515, 320, 256, False, 1), (515, 512, 768, False, 8), (257, 320, 2048, False, 8), (1, 512, 2048, False, 8),
         (257, 320, 1280, False, 1), (1, 64, 256, True, 1), (255, 320, 768, True, 1), (257, 512, 256, True, 1),
         (515, 320, 768, True, 1), (257, 64, 1280, True, 1)]
EDGE_EXP = [-2, -2, -3, 0]  # of the rows _acts starts with


def _acts(M, K, seed=0):
    """bf16 [M, K]: a seeded normal times a power of two per row in 2^-6..2^6. The first rows (as many as M has) have an
    amax of exactly 448 * 2^-3, the next bf16 above it and the next bf16 below it; the fourth is all zero."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-6, 7, (M, 1), generator=g).float())
    x[:3] = x[:3].clamp(-1, 1)
    x[3:4] = 0
    for row, (col, v) in enumerate([(5, 56.0), (K - 9, -56.25), (K // 2 + 2, 55.75)][:M]):
        x[row, col] = v
    return x.to(torch.bfloat16)


@pytest.mark.gpu
@pytest.mark.parametrize("M,K,pad", [(1, 256, 0), (37, 768, 8), (257, 2048, 0)])
def test_fp8_act_quant_gpu_equals_reference(cuda, M, K, pad):
    x = _acts(M, K, seed=M)
    xg = torch.zeros(M, K + pad, dtype=torch.bfloat16, device=cuda)[:, :K]  # (pad: a row view with ldx > K)
    xg.copy_(x)
    xq, xe = ops.fp8_act_quant(xg)
    wq, we = ref.fp8_quant(x)
    assert xe.dtype == torch.int32 and xe.shape == (M,) and we[:4].tolist() == EDGE_EXP[:M]
    assert torch.equal(xe.cpu(), we.int()) and torch.equal(ops.fp8_act_order(xq.cpu()), wq)
    cq, ce = ops.fp8_act_quant(x)  # the CPU path describes the same byte order
    assert torch.equal(cq, xq.cpu()) and torch.equal(ce, we)


@functools.lru_cache(maxsize=None)
def _case(N, K, glu):
    """(x [515, K] on the GPU, its dequantised fp8 values in float64, tiles, row scales, the dequantised weight in
    float64)"""
    dev = torch.device("cuda:0")
    wt, s = ops.tile_weight_as(_weight_rows(N, K, seed=N + K + glu, device=dev), "fp8", glu)
    x = _acts(515, K, seed=K)
    xq, xe = ref.fp8_quant(x)
    xd = torch.ldexp(xq.view(torch.float8_e4m3fn).double(), xe[:, None])
    return x.to(dev), xd, wt, s, ops.untile_weight_as(wt, s, glu).double().cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,glu,ms", CASES)
def test_linear_tiles_fp8_vs_float64(cuda, M, N, K, glu, ms):
    x515, xd, wt, s, deq = _case(N, K, glu)
    S = ops.tile_gemm_plan(M, N, K, 1 if glu else ms)
    assert (S > 1) == (K == 2048)
    y = ops.linear_tiles(x515[:M], wt, max_splits=ms, glu=glu, scale=s, act="fp8")
    want = xd[:M] @ deq.t()
    assert y.float().abs().max() > 0
    if glu:
        assert y.dtype == torch.bfloat16 and y.shape == (M, N // 2)
        _close(y, ref.silu_mul(want), atol=0.03, rtol=0.02, msg=f"glu M={M} N={N} K={K}")
        return
    assert y.shape == ((S, M, N) if S > 1 else (M, N)) and ops.is_slab(y) == (S > 1)
    torch.testing.assert_close(ops.slab_reduce(y).double().cpu(), want, atol=2e-2, rtol=2e-2)


@pytest.mark.gpu
def test_fp8_act_refusals(cuda):
    e = ops._ext.load()
    w = _weight_rows(128, 512, device=cuda)
    (w16, _), (w8, s8), (w4, s4) = (ops.tile_weight_as(w, f, True) for f in ("bf16", "fp8", "mxfp4"))
    x = torch.zeros(300, 512, device=cuda, dtype=torch.bfloat16)
    for wt, sc, name in ((w16, None, "bf16"), (w4, s4, "mxfp4")):
        with pytest.raises(ValueError, match=name):
            ops.linear_tiles(x, wt, scale=sc, act="fp8")
    u8 = dict(device=cuda, dtype=torch.uint8)
    xq, xe = torch.full((300, 512), 7, **u8), torch.full((300,), 7, device=cuda, dtype=torch.int32)
    y = torch.full((300, 128), 7.0, device=cuda, dtype=torch.bfloat16)
    p = torch.full((2, 300, 128), 7.0, device=cuda)
    for args in [(x, xq, xe[:299]), (x, xq, xe.float()),                          # a wrong xe length / dtype
                 (x[:, :384], xq[:, :384].contiguous(), xe),                       # K % 256 != 0
                 (torch.zeros(300, 513, device=cuda, dtype=x.dtype)[:, :512], xq, xe)]:  # ldx
        with pytest.raises(RuntimeError):
            e.act_quant_fp8(*args)
    for args in [(xq, xe[:299], w8, s8, y, None, 1, False), (xq, xe.float(), w8, s8, y, None, 1, False),
                 (xq, xe, w8, s8[:64].contiguous(), y, None, 1, False), (xq, xe, w8, s8.double(), y, None, 1, False),
                 (xq[:, :384], xe, w8[:, :12].contiguous(), s8, y, None, 1, False),  # K % 256 != 0
                 (xq, xe, w8, s8, y[:, :64], p, 2, True),                          # GLU with two splits
                 (torch.zeros(300, 520, **u8)[:, :512], xe, w8, s8, y, None, 1, False)]:  # ldxq % 16 != 0
        with pytest.raises(RuntimeError):
            e.tile_gemm_f8(*args)
    torch.cuda.synchronize()
    assert all((t == 7).all() for t in (xq, xe, y, p)), "a refused call wrote its output"


def _engine(monkeypatch, **kw):
    from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine

    eng = LLMEngine(EngineConfig(**kw))
    calls, tiles = [], ops.linear_tiles
    monkeypatch.setattr(ops, "linear_tiles", lambda x, *a, **k: (calls.append((x.shape[0], k.get("act", "bf16"))),
                                                                 tiles(x, *a, **k))[1])
    return eng, calls


ENVS = ("KAFKA_WEIGHT_DTYPE", "KAFKA_DECODE_GEMM", "KAFKA_TILE_PREFILL", "KAFKA_ACT_DTYPE", "KAFKA_EXPERT_TILES_ONLY")


def test_act_fp8_engine_cpu(monkeypatch):
    """A 300-token prefill and two decode steps of a tiny Llama in fp8 tiles with fp8 prefill activations. The CPU path
    contains no kernel: the greedy gap it keeps is the format's (the project's 0.15)."""
    from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
    from kafka_llm_service_amd.engine.sequence import SamplingParams

    for env in ENVS:
        monkeypatch.delenv(env, raising=False)
    monkeypatch.setattr(ops, "STREAM_MAX_M", 128)
    for kw in (dict(weight_dtype="bf16", tile_prefill=True), dict(weight_dtype="mxfp4", tile_prefill=True),
               dict(weight_dtype="fp8"), dict(model="tiny-mixtral", weight_dtype="fp8", expert_tiles_only=True)):
        with pytest.raises(ValueError, match="act_dtype"):
            LLMEngine(EngineConfig(**_cpu_cfg(act_dtype="fp8", **kw)))
    eng, calls = _engine(monkeypatch, **_cpu_cfg(weight_dtype="fp8", tile_prefill=True, act_dtype="fp8"))
    assert eng.model.act_dtype == "fp8"
    prompts = [torch.randint(0, 5000, (300,), generator=torch.Generator().manual_seed(3)).tolist()]
    outs = eng.generate(prompts, SamplingParams(temperature=0.0, max_tokens=3, ignore_eos=True))
    # every layer's four projections with 300 rows; the lm_head's rows and the decode steps never
    assert [c for c in calls if c[1] == "fp8"] == [(300, "fp8")] * (4 * len(eng.model.layers))
    assert all(rows < 300 for rows, act in calls if act == "bf16")
    _assert_greedy_gap(eng.model, prompts, outs, 0.15)
    monkeypatch.setenv("KAFKA_ACT_DTYPE", "fp8")  # the environment turns the mode on for a default config
    assert LLMEngine(EngineConfig(**_cpu_cfg(weight_dtype="fp8", tile_prefill=True))).model.act_dtype == "fp8"


@pytest.mark.gpu
def test_act_fp8_engine_gpu(cuda, monkeypatch):
    """One 333-token prompt (the first step's projections run the e4m3 x e4m3 kernel), then 8 greedy decode steps on the
    streaming kernel; the bound of test_tile_prefill_engine_gpu, against the same mode on the CPU reference path."""
    from kafka_llm_service_amd.engine.sequence import SamplingParams

    for env in ENVS:
        monkeypatch.delenv(env, raising=False)
    f8, gemm = [], ops._ext.load().tile_gemm_f8
    monkeypatch.setattr(ops._ext.load(), "tile_gemm_f8", lambda xq, *a: (f8.append(xq.shape[0]), gemm(xq, *a))[1])
    e, calls = _engine(monkeypatch, model="small-llama", device=str(cuda), num_kv_blocks=1024, max_model_len=4096,
                       weight_dtype="fp8", tile_prefill=True, act_dtype="fp8")
    prompts = [torch.randint(0, 5000, (333,), generator=torch.Generator().manual_seed(3)).tolist()]
    outs = e.generate(prompts, SamplingParams(temperature=0.0, max_tokens=9, ignore_eos=True))
    assert f8 == [333] * (4 * len(e.model.layers)) and [c for c in calls if c[1] == "fp8"] == [(333, "fp8")] * len(f8)
    _assert_greedy_gap(e.model, prompts, outs, 0.25)
