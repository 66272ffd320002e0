"""Expert-tiles-only mode (``enable_stream_weights(expert_tiles_only=True)``, ``EngineConfig.expert_tiles_only``): the MoE
experts live in their wave tiles alone, in any tile format; steps above ``MOE_STREAM_MAX_T`` run the grouped tile GEMM on
them. The GPU bound on greedy tokens is the existing engine MoE tests' (0.25 logits of the dense oracle)."""
import pytest
import torch
from test_weight_mxfp4 import _assert_greedy_gap

from kafka_llm_service_amd import ops

FORMATS = ["bf16", "fp8", "mxfp4"]


@pytest.mark.parametrize("fmt", FORMATS)
def test_expert_tiles_only_model_cpu(fmt, tmp_path):
    from kafka_llm_service_amd.models.config import get_config
    from kafka_llm_service_amd.models.oracle import dense_logits
    from kafka_llm_service_amd.models.weights import build_model, save_safetensors

    cfg = get_config("tiny-mixtral")
    both, only = build_model(cfg, "cpu"), build_model(cfg, "cpu")
    both.enable_stream_weights(weight_dtype=fmt)
    before = only.weight_bytes()
    predicted = only.stream_weight_bytes(fmt, expert_tiles_only=True)
    assert only.enable_stream_weights(weight_dtype=fmt, expert_tiles_only=True) == predicted
    assert only.expert_tiles_only and not both.expert_tiles_only and only.weight_bytes() == before + predicted
    row_major = 0
    for lw, lb in zip(only.layers, both.layers):
        assert lw.w13 is None and lw.w2 is None and lw.w13_t.dtype == lb.w13_t.dtype
        assert torch.equal(lw.w13_t.view(torch.uint8), lb.w13_t.view(torch.uint8))
        row_major += sum(w.numel() * w.element_size() for w in (lb.w13, lb.w2))
    assert only.weight_bytes() == both.weight_bytes() - row_major
    save_safetensors(only, tmp_path / "model.safetensors")
    back = build_model(cfg, "cpu", weights=str(tmp_path))
    for lw, lk in zip(only.layers, back.layers):
        assert torch.equal(lk.w13, ops.untile_experts_as(lw.w13_t, lw.w13_s, True))
        assert torch.equal(lk.w2, ops.untile_experts_as(lw.w2_t, lw.w2_s))
    toks = torch.randint(0, 5000, (40,), generator=torch.Generator().manual_seed(3)).tolist()
    assert torch.equal(dense_logits(only, toks), dense_logits(both, toks))
    with pytest.raises(ValueError):
        build_model(cfg, "cpu").enable_stream_weights(tiled_only=True, weight_dtype=fmt, expert_tiles_only=True)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["mxfp4", "fp8"])
def test_expert_tiles_only_engine_gpu(cuda, fmt, monkeypatch):
    """One prompt of more than MOE_STREAM_MAX_T tokens with nothing decoding (the first step runs the grouped tile GEMM),
    then 8 greedy decode steps on the streaming kernel."""
    from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
    from kafka_llm_service_amd.engine.sequence import SamplingParams
    from kafka_llm_service_amd.models import moe

    monkeypatch.delenv("KAFKA_WEIGHT_DTYPE", raising=False)
    monkeypatch.delenv("KAFKA_EXPERT_TILES_ONLY", raising=False)
    rows, glu = [], ops.grouped_tiles_glu

    def counted(x, *a, **kw):
        rows.append(x.shape[0])
        return glu(x, *a, **kw)

    monkeypatch.setattr(ops, "grouped_tiles_glu", counted)
    e = LLMEngine(EngineConfig(model="tiny-mixtral", device=str(cuda), num_kv_blocks=1024, max_model_len=4096,
                               weight_dtype=fmt, expert_tiles_only=True))
    assert e.model.expert_tiles_only and all(lw.w13 is None and lw.w2 is None for lw in e.model.layers)
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(0, e.model_cfg.vocab_size, (moe.MOE_STREAM_MAX_T + 60,), generator=g).tolist()]
    outs = e.generate(prompts, SamplingParams(temperature=0.0, max_tokens=9, ignore_eos=True))
    assert rows and min(rows) > moe.MOE_STREAM_MAX_T, rows
    _assert_greedy_gap(e.model, prompts, outs, 0.25)
