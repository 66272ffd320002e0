"""fp8 / MXFP4 tiles on the skinny MFMA GEMM (csrc/skinny_gemm.hip WF_FP8 / WF_MXFP4, ops.linear_skinny ``scale=``):
bit-equality with the bf16 kernel on the dequantised weight, the float64 product, the binding's checks, the routing."""
import functools

import pytest
import torch

from kafka_llm_service_amd import ops
from kafka_llm_service_amd.ops import reference as ref

FORMATS = ("fp8", "mxfp4")
DEVICES = ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)]
# (N, K, glu, max_splits, splits of the plan): what each shape can break
SHAPES = [(128, 64, False, 1, 1),    # one workgroup, one stage: the ring shorter than its depth
          (128, 320, False, 8, 1),   # five stages: the ring wraps, K no multiple of 128
          (256, 1024, False, 8, 4),  # k0 != 0: tile and scale-image offsets per split, slab epilogue
          (256, 1024, True, 1, 1),   # fused SwiGLU on GLU-interleaved quantised tiles
          (256, 1024, True, 8, 4)]   # gate | up slab column mapping


@functools.lru_cache(maxsize=None)
def _case(fmt, N, K, glu, device="cpu"):
    """(x [256, K] * 0.5, tiles, scale, dequantised weight): w * 0.02, rows times 2^-3..2^3 (distinct fp8 row scales),
    32-column blocks times 2^-2..2^2 (distinct mxfp4 block exponents within a row)."""
    g = torch.Generator().manual_seed(N + K + glu)
    x = (torch.randn(256, K, generator=g) * 0.5).to(torch.bfloat16)
    w = torch.randn(N, K, generator=g) * 0.02 * torch.exp2(torch.randint(-3, 4, (N, 1), generator=g).float())
    w = w.view(N, K // 32, 32) * torch.exp2(torch.randint(-2, 3, (N, K // 32, 1), generator=g).float())
    wt, s = ops.tile_weight_as(w.view(N, K).to(torch.bfloat16).to(device), fmt, glu)
    return x.to(device), wt, s, ops.untile_weight_as(wt, s, glu)


@pytest.mark.parametrize("N,K,glu,ms,S", SHAPES)
@pytest.mark.parametrize("M", [129, 200, 256])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("dev", DEVICES)
def test_skinny_quant_matches_dequantised(request, dev, fmt, M, N, K, glu, ms, S):
    """The kernel (cuda) and its CPU mirror: bit-equal to the call on bf16 tiles of the dequantised weight (same fragments,
    order and splits: a difference is a layout, scale or offset bug) and close to the float64 product."""
    x256, wt, s, deq = _case(fmt, N, K, glu, dev if dev == "cpu" else str(request.getfixturevalue("cuda")))
    assert ops.skinny_plan(M, N, K, ms) == S
    y = ops.linear_skinny(x256[:M], wt, max_splits=ms, glu=glu, scale=s)
    assert torch.equal(y, ops.linear_skinny(x256[:M], ops.tile_weight(deq, glu), max_splits=ms, glu=glu))
    want, got = x256[:M].double() @ deq.double().t(), (y.sum(0) if S > 1 else y)
    if glu:
        want, got = ref.silu_mul(want), (ref.silu_mul(got) if S > 1 else got)
    torch.testing.assert_close(got.double(), want, atol=2e-2, rtol=2e-2)
    with pytest.raises(ValueError):
        ops.linear_skinny(x256[:M], wt, max_splits=ms, glu=glu)  # quantised tiles without their scale


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_skinny_quant_binding_refuses_other_format(cuda, fmt):
    """Both quantised tiles are uint8 [., ., 64, 16]: the binding checks them against the format the caller names."""
    other = FORMATS[fmt == "fp8"]
    (x, wt, s, _), (_, _, so, _) = (_case(f, 128, 320, False, str(cuda)) for f in (fmt, other))
    wt, s, so = (t if t.dtype == torch.float32 else t.view(torch.uint8) for t in (wt, s, so))
    y = torch.empty(200, 128, dtype=torch.bfloat16, device=cuda)
    for scale, name in ((s, other), (so, fmt)):  # under the other format's name; with the other format's scale
        with pytest.raises(RuntimeError):
            ops._ext.load().skinny_gemm(x[:200], wt, y, None, 1, False, scale=scale, fmt=ops.weight_format(name).abi)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("dev", DEVICES)
def test_engine_skinny_quant(request, monkeypatch, dev, fmt):
    """129..256-row steps of a quantised model call linear_skinny with its tiles and scale, within the oracle gap bounds
    and prompts of tests/test_weight_fp8.py (0.15 CPU, 0.25 GPU). CPU, one 150-row prefill: three calls per layer and the
    tokens of SKINNY empty (seed 3: oracle top-2 margins >= 0.03 here; other seeds tie within one bf16 step)."""
    from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
    from kafka_llm_service_amd.engine.sequence import SamplingParams
    from kafka_llm_service_amd.models import llama
    from kafka_llm_service_amd.models.oracle import dense_logits
    gpu = dev != "cpu" and request.getfixturevalue("cuda") is not None
    monkeypatch.delenv("KAFKA_WEIGHT_DTYPE", raising=False)
    monkeypatch.setattr(ops, "STREAM_MAX_M", 128)  # (150 rows would otherwise stream on the CPU: 192-row tile)
    monkeypatch.setattr(llama, "SKINNY", frozenset({"qkv", "o", "down"}))
    g = torch.Generator().manual_seed(11 if gpu else 3)
    pre = torch.randint(0, 5000, (600 if gpu else 100,), generator=g).tolist()
    prompts = [pre + torch.randint(0, 5000, (n,), generator=g).tolist() for n in ((3, 60, 150, 7) if gpu else (50,))]
    greedy = SamplingParams(temperature=0.0, max_tokens=8 if gpu else 6, ignore_eos=True)
    cfg = EngineConfig(model="small-llama" if gpu else "tiny-llama", device=dev, num_kv_blocks=1024,
                       max_model_len=4096, weight_dtype=fmt)
    eng, calls, orig = LLMEngine(cfg), [], ops.linear_skinny
    monkeypatch.setattr(ops, "linear_skinny", lambda x, wt, *a, **k: (
        calls.append((x.shape[0], wt.dtype, k.get("scale") is not None)), orig(x, wt, *a, **k))[1])
    outs = eng.generate(prompts, greedy)
    q = eng.model.layers[0].qkv_t.dtype
    assert q != torch.bfloat16 and calls and all(129 <= m <= 256 and dt == q and scaled for m, dt, scaled in calls)
    for p, o in zip(prompts, outs):
        rows = dense_logits(eng.model, p + o)[len(p) - 1:len(p) - 1 + len(o)].float().cpu()
        gaps = rows.max(-1).values - rows.gather(1, torch.tensor(o)[:, None])[:, 0]
        assert gaps.max().item() < (0.25 if gpu else 0.15), gaps
    if not gpu:
        assert len(calls) % 3 == 0
        monkeypatch.setattr(llama, "SKINNY", frozenset())
        assert LLMEngine(cfg, model=eng.model).generate(prompts, greedy) == outs
