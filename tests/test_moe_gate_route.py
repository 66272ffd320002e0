"""Fused MoE router (``ops.moe_gate_route``, csrc/moe_router.hip): the gate GEMM, top-k and expert sort of one launch
against the fp64 gate product and ``ref.moe_route``, its re-armed ticket under back-to-back calls and hipGraph replay,
and ``EngineConfig.fused_router``."""
import pytest
import torch
import torch.nn.functional as F
from test_weight_mxfp4 import _assert_greedy_gap

from kafka_llm_service_amd import ops
from kafka_llm_service_amd.ops import reference as ref

# T, d, E, k: tiny-mixtral; a ragged last row tile; 8x7B decode (several K splits); 8x22B width; the E and k limits with
# more than one token per finisher thread and enough row tiles for one K split
SHAPES = [(1, 512, 4, 2), (77, 512, 8, 2), (130, 4096, 8, 2), (640, 6144, 8, 2), (3000, 1024, 16, 4)]
FIELDS = ("topk_w", "topk_e", "perm_tok", "perm_w", "expert_off", "tile_off")


def _exact_inputs(T, d, E, seed):
    """x in {-1, 0, 1} (a quarter non-zero), w in {-1, 0, 1} / 8 (half non-zero): every logit is a multiple of 1/8 and,
    for |8 logit| <= 255, exact in fp32 under any summation order and in bf16."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-1, 2, (T, d), generator=g) * (torch.rand(T, d, generator=g) < 0.375)
    w = torch.randint(-1, 2, (E, d), generator=g) * (torch.rand(E, d, generator=g) < 0.75)
    return x.to(torch.bfloat16), (w.double() / 8).to(torch.bfloat16)


def _exact(x, w):
    exact = x.cpu().double() @ w.cpu().double().t()
    assert float(exact.abs().max()) * 8 <= 255  # a condition on the inputs (nine standard deviations at d = 6144)
    return exact.to(torch.bfloat16)


def _check_routing(r, logits, k):
    """r against ref.moe_route on the (CPU) logits: indices exactly, weights within test_moe_route's 1e-5."""
    want = dict(zip(FIELDS, ref.moe_route(logits, k, ops.GG_BM)))
    for f in FIELDS:
        got = getattr(r, f).cpu()
        if f in ("topk_w", "perm_w"):
            assert (got - want[f]).abs().max().item() <= 1e-5, f
        else:
            assert torch.equal(got, want[f]), f


@pytest.mark.gpu
@pytest.mark.parametrize("T,d,E,k", SHAPES)
def test_gate_route_exact(cuda, T, d, E, k):
    x, w = _exact_inputs(T, d, E, seed=T)
    exact = _exact(x, w)
    xs = torch.zeros(T, d + 8, dtype=torch.bfloat16, device=cuda)[:, :d]  # a row stride that is not d
    xs.copy_(x)
    out = torch.full((T, E), float("nan"), dtype=torch.bfloat16, device=cuda)
    r = ops.moe_gate_route(xs, w.to(cuda), k, logits_out=out)
    assert torch.equal(out.cpu(), exact)
    _check_routing(r, exact, k)


@pytest.mark.gpu
@pytest.mark.parametrize("T,d,E,k", SHAPES)
def test_gate_route_gaussian(cuda, T, d, E, k):
    g = torch.Generator().manual_seed(T)
    x = torch.randn(T, d, generator=g).to(torch.bfloat16)
    w = (torch.randn(E, d, generator=g) * d ** -0.5).to(torch.bfloat16)
    want = x.double() @ w.double().t()
    out = torch.empty(T, E, dtype=torch.bfloat16, device=cuda)
    r = ops.moe_gate_route(x.to(cuda), w.to(cuda), k, logits_out=out)
    out = out.cpu()
    # one bf16 step: half an ulp of rounding plus the fp32 accumulation error, far below it at these depths
    assert bool(((out.double() - want).abs() <= 2.0 ** -7 * want.abs() + 1e-4).all())
    _check_routing(r, out, k)


@pytest.mark.gpu
def test_gate_route_rearm_and_replay(cuda):
    """Two calls of different T back to back on the same workspace, then one captured call replayed twice with X
    rewritten in place: the ticket re-arms itself and no launch needs a memset."""
    d, E, k = 4096, 8, 2
    cases = [_exact_inputs(T, d, E, seed=s) for T, s in ((130, 1), (77, 2), (130, 3), (130, 4))]
    w = cases[0][1].to(cuda)
    for x, _ in cases[:2]:
        out = torch.empty(x.shape[0], E, dtype=torch.bfloat16, device=cuda)
        r = ops.moe_gate_route(x.to(cuda), w, k, logits_out=out)
        assert torch.equal(out.cpu(), _exact(x, w))
        _check_routing(r, _exact(x, w), k)
    xg = torch.zeros(130, d, dtype=torch.bfloat16, device=cuda)
    out = torch.empty(130, E, dtype=torch.bfloat16, device=cuda)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.moe_gate_route(xg, w, k, logits_out=out)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = ops.moe_gate_route(xg, w, k, logits_out=out)
    for x, _ in cases[2:]:
        xg.copy_(x)
        graph.replay()
        assert torch.equal(out.cpu(), _exact(x, w))
        _check_routing(r, _exact(x, w), k)


@pytest.mark.gpu
def test_fused_router_engine_gpu(cuda, monkeypatch):
    """One prompt of several router row tiles with nothing decoding, then 8 greedy decode steps, all routed by the fused
    launch; the bound on greedy tokens is the engine MoE tests' (0.25 logits of the dense oracle)."""
    from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
    from kafka_llm_service_amd.engine.sequence import SamplingParams

    monkeypatch.delenv("KAFKA_FUSED_ROUTER", raising=False)
    rows, fused = [], ops.moe_gate_route

    def counted(x, *a, **kw):
        rows.append(x.shape[0])
        return fused(x, *a, **kw)

    monkeypatch.setattr(ops, "moe_gate_route", counted)
    e = LLMEngine(EngineConfig(model="tiny-mixtral", device=str(cuda), num_kv_blocks=1024, max_model_len=4096,
                               fused_router=True))
    assert e.model.fused_router
    prompts = [torch.randint(0, e.model_cfg.vocab_size, (200,), generator=torch.Generator().manual_seed(3)).tolist()]
    outs = e.generate(prompts, SamplingParams(temperature=0.0, max_tokens=9, ignore_eos=True))
    assert max(rows) > 64 and rows.count(1) >= 8 * e.model_cfg.num_layers, rows
    _assert_greedy_gap(e.model, prompts, outs, 0.25)


@pytest.mark.parametrize("T,d,E,k", [(1, 512, 4, 2), (77, 512, 8, 2), (300, 256, 16, 4)])
def test_gate_route_cpu(T, d, E, k):
    g = torch.Generator().manual_seed(T)
    x = torch.randn(T, d, generator=g).to(torch.bfloat16)
    w = (torch.randn(E, d, generator=g) * d ** -0.5).to(torch.bfloat16)
    out = torch.empty(T, E, dtype=torch.bfloat16)
    r, want = ops.moe_gate_route(x, w, k, logits_out=out), ops.moe_route(F.linear(x, w), k)
    assert torch.equal(out, F.linear(x, w))
    assert all(torch.equal(getattr(r, f), getattr(want, f)) for f in FIELDS) and r.max_tiles == want.max_tiles
    assert ops.moe_gate_route_supported(d, E, k) and not ops.moe_gate_route_supported(d + 32, E, k)
    assert not ops.moe_gate_route_supported(d, 32, k) and not ops.moe_gate_route_supported(d, E, 5)


def test_fused_router_engine_cpu(monkeypatch):
    from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
    from kafka_llm_service_amd.engine.sequence import SamplingParams

    monkeypatch.delenv("KAFKA_FUSED_ROUTER", raising=False)
    calls, fused = [], ops.moe_gate_route
    monkeypatch.setattr(ops, "moe_gate_route", lambda x, *a, **kw: calls.append(x.shape[0]) or fused(x, *a, **kw))
    cfg = dict(model="tiny-mixtral", device="cpu", num_kv_blocks=256, max_model_len=2048)
    prompts = [torch.randint(0, 5000, (40,), generator=torch.Generator().manual_seed(3)).tolist()]
    sp = SamplingParams(temperature=0.0, max_tokens=4, ignore_eos=True)
    plain = LLMEngine(EngineConfig(**cfg))
    want = plain.generate(prompts, sp)
    assert not plain.model.fused_router and not calls
    eng = LLMEngine(EngineConfig(**cfg, fused_router=True))
    assert eng.model.fused_router and eng.generate(prompts, sp) == want and calls
    monkeypatch.setenv("KAFKA_FUSED_ROUTER", "1")
    assert LLMEngine(EngineConfig(**cfg)).cfg.fused_router
    with pytest.raises(ValueError, match="dense"):
        LLMEngine(EngineConfig(**dict(cfg, model="tiny-llama")))
