"""fp8 (OCP e4m3) weights for the decode GEMMs (``weight_dtype="fp8"``): e4m3 wave tiles with one power-of-two scale
per output row, dequantised by v_cvt_scalef32_pk_bf16_fp8 inside the weight-streaming kernel (MFMA stays bf16).

The fp8 model IS the quantised model at every step size: the row-major bf16 copy of every quantised projection holds
the dequantised values (exact in bf16), so prefill (hipBLASLt), decode (the W8 streaming kernel), the CPU reference
path and the dense oracle all compute with the same weights and only the accumulation order differs. Every tolerance
below is therefore the one of the bf16 test it mirrors, unchanged:
  * kernels: atol 0.02 / rtol 0.01 against x @ deq^T in fp32 (tests/test_kernels_gpu.py test_wstream_gemm; GLU
    0.03 / 0.02, test_wstream_glu). W's rows carry random power-of-two factors 2^-3..2^3 so a wrong scale index fails;
  * engine: greedy tokens within 0.15 (CPU) / 0.25 (GPU) logits of the dense oracle (tests/test_kv_fp8.py);
  * composed numerics: the metric and bounds of tests/test_numerics_gpu.py (<= 0.25 std, <= 3x the bf16 forward).
Quantisation itself is checked against the e4m3 bound of tests/test_kv_fp8.py (``_within_fp8``)."""
import functools

import pytest
import torch

from kafka_llm_service_amd import ops
from kafka_llm_service_amd.ops import reference as ref


def _within_fp8(deq, x):
    amax = x.abs().amax(-1, keepdim=True)
    bad = (deq - x).abs() > x.abs() / 16 + amax * 2.0 ** -9 + 1e-12
    assert not bad.any(), f"{int(bad.sum())} elements outside the e4m3 bound"


def _weight(N, K, seed=0, device="cpu"):
    """bf16 [N, K], std 0.05, each row times a random power of two in 2^-3..2^3 (distinct row scales)."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) * 0.05 * torch.exp2(torch.randint(-3, 4, (N, 1), generator=g).float())
    return w.to(torch.bfloat16).to(device)


# ---------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("glu", [False, True])
def test_tile_weight_fp8_roundtrip(glu):
    N, K = 256, 4096
    w = _weight(N, K, seed=1)
    wt8, st = ops.tile_weight_fp8(w, glu=glu)
    assert wt8.dtype == torch.uint8 and wt8.shape == (N // 32, K // 32, 64, 16) and wt8.is_contiguous()
    assert st.dtype == torch.float32 and st.shape == (N,)
    deq = ops.untile_weight_fp8(wt8, st, glu=glu)
    assert deq.dtype == torch.bfloat16 and deq.shape == (N, K)
    q, e = ref.fp8_quant(w)
    exact = q.view(torch.float8_e4m3fn).float() * torch.exp2(e.float())[:, None]
    assert torch.equal(deq.float(), exact)  # element for element, and exact in bf16
    assert torch.equal(exact.to(torch.bfloat16).float(), exact)
    _within_fp8(deq.float(), w.float())
    # scales are the powers of two 2^e in tile order
    order = torch.arange(N).view(N // 32, 32)
    if glu:
        order = order.view(2, N // 64, 32).transpose(0, 1).reshape(N // 32, 32)
    assert torch.equal(st, torch.exp2(e.float())[order.reshape(-1)])
    # lane formula, one (tile, k pair, lane): bytes 0..7 = k-step 2 kb2, bytes 8..15 = k-step 2 kb2 + 1
    nb, kb2, lane = 5, 77, 45
    r, h = lane % 32, lane // 32
    row = int(order[nb, r])
    assert torch.equal(wt8[nb, kb2, lane, :8], q[row, 32 * kb2 + 8 * h: 32 * kb2 + 8 * h + 8])
    assert torch.equal(wt8[nb, kb2, lane, 8:], q[row, 32 * kb2 + 16 + 8 * h: 32 * kb2 + 16 + 8 * h + 8])
    assert float(st[32 * nb + r]) == 2.0 ** int(e[row])


def test_linear_stream_fp8_cpu_equals_dequantised():
    """CPU path: fp8 tiles + scales == the same call on the bf16 tiles of the dequantised weight, slab and one-split."""
    M, N, K = 4, 256, 1024
    g = torch.Generator().manual_seed(2)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    for glu in (False, True):
        w = _weight(N, K, seed=3)
        wt8, st = ops.tile_weight_fp8(w, glu=glu)
        wt = ops.tile_weight(ops.untile_weight_fp8(wt8, st, glu=glu), glu=glu)
        assert ops.stream_plan(M, N, K, 8)[2] > 1 and ops.stream_plan(M, N, K, 1)[2] == 1
        for ms in (1, 8):
            a = ops.linear_stream(x, wt8, max_splits=ms, glu=glu, scale=st)
            b = ops.linear_stream(x, wt, max_splits=ms, glu=glu)
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
            if glu:
                assert torch.equal(ops.linear_glu(x, wt8, max_splits=ms, scale=st), ops.linear_glu(x, wt, max_splits=ms))
    with pytest.raises(ValueError):
        ops.linear_stream(x, wt8)  # uint8 tiles without their scales
    with pytest.raises(ValueError):
        ops.linear_glu(x, wt8)
    with pytest.raises(ValueError):
        ops.linear_stream(x, wt8, nt=False, scale=st)


def _cpu_cfg(**kw):
    cfg = dict(model="tiny-llama", device="cpu", num_kv_blocks=256, max_model_len=2048)
    cfg.update(kw)
    return cfg


def _cpu_prompts():
    g = torch.Generator().manual_seed(3)
    pre = torch.randint(0, 5000, (70,), generator=g).tolist()
    return [pre + torch.randint(0, 5000, (n,), generator=g).tolist() for n in (5, 17, 40)]


def _assert_greedy_gap(model, prompts, outs, bound):
    from kafka_llm_service_amd.models.oracle import dense_logits

    for p, o in zip(prompts, outs):
        lg = dense_logits(model, p + o)
        for i, tok in enumerate(o):
            row = lg[len(p) - 1 + i]
            assert (row.max() - row[tok]).item() < bound, f"token {i}: gap {(row.max() - row[tok]).item():.3f}"


def test_engine_fp8_weights_cpu(monkeypatch):
    from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
    from kafka_llm_service_amd.engine.sequence import SamplingParams
    from kafka_llm_service_amd.models.llama import LayerWeights

    monkeypatch.delenv("KAFKA_WEIGHT_DTYPE", raising=False)
    monkeypatch.delenv("KAFKA_DECODE_GEMM", raising=False)
    eng = LLMEngine(EngineConfig(**_cpu_cfg(weight_dtype="fp8")))
    m = eng.model
    assert m.stream and not m.tiled_only and m.weight_dtype == "fp8"  # auto -> stream on the CPU too
    embed = m.embed.clone()
    for lw in m.layers:
        for name in LayerWeights.STREAMED:
            wt, st = getattr(lw, name + "_t"), getattr(lw, name + "_s")
            assert wt.dtype == torch.uint8 and st.dtype == torch.float32
            glu = name == "gate_up" and bool(lw.glu)
            assert torch.equal(getattr(lw, name), ops.untile_weight_fp8(wt, st, glu=glu))
    assert m.lm_head_t.dtype == torch.uint8
    assert torch.equal(m.lm_head, ops.untile_weight_fp8(m.lm_head_t, m.lm_head_s))
    assert not any(k.endswith("_s") or k.endswith("_t") for k in m.named_tensors())
    prompts = _cpu_prompts()
    sp = SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True)
    outs = eng.generate(prompts, sp)
    assert eng.generate(prompts, sp) == outs  # prefix-cached rerun
    _assert_greedy_gap(m, prompts, outs, 0.15)
    assert torch.equal(m.embed, embed)
    bf16 = LLMEngine(EngineConfig(**_cpu_cfg(decode_gemm="stream")))
    assert bf16.model.weight_dtype == "bf16" and bf16.model.lm_head_t.dtype == torch.bfloat16
    assert m.weight_bytes() < bf16.model.weight_bytes()
    assert m.stream_weight_bytes("fp8") < bf16.model.stream_weight_bytes() * 0.52
    # the environment turns the mode on for a default config
    monkeypatch.setenv("KAFKA_WEIGHT_DTYPE", "fp8")
    env_eng = LLMEngine(EngineConfig(**_cpu_cfg()))
    assert env_eng.model.weight_dtype == "fp8" and env_eng.model.layers[0].qkv_t.dtype == torch.uint8
    assert env_eng.cfg.weight_dtype == "fp8"
    monkeypatch.delenv("KAFKA_WEIGHT_DTYPE")
    with pytest.raises(ValueError):
        LLMEngine(EngineConfig(**_cpu_cfg(weight_dtype="fp8", decode_gemm="blas")))
    with pytest.raises(ValueError):
        LLMEngine(EngineConfig(**_cpu_cfg(weight_dtype="int4")))


def test_engine_fp8_weights_tiled_only_cpu(tmp_path, monkeypatch):
    from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
    from kafka_llm_service_amd.engine.sequence import SamplingParams
    from kafka_llm_service_amd.models.weights import build_model, save_safetensors

    monkeypatch.delenv("KAFKA_WEIGHT_DTYPE", raising=False)
    monkeypatch.delenv("KAFKA_DECODE_GEMM", raising=False)
    eng = LLMEngine(EngineConfig(**_cpu_cfg(weight_dtype="fp8", decode_gemm="stream_only")))
    m = eng.model
    assert m.tiled_only and m.weight_dtype == "fp8"
    lw = m.layers[0]
    assert lw.qkv is None and lw.o is None and lw.gate_up is None and lw.down is None and m.lm_head is None
    assert lw.qkv_t.dtype == torch.uint8 and lw.qkv_s is not None and m.lm_head_s is not None
    calls = []
    orig = ops.untile_weight_fp8

    def counting(*a, **kw):
        calls.append(1)
        return orig(*a, **kw)

    monkeypatch.setattr(ops, "untile_weight_fp8", counting)
    prompts = _cpu_prompts()
    outs = eng.generate(prompts, SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True))
    assert calls, "prefill did not go through the dequantising untile"
    monkeypatch.setattr(ops, "untile_weight_fp8", orig)
    _assert_greedy_gap(m, prompts, outs, 0.15)
    save_safetensors(m, tmp_path / "model.safetensors")
    back = build_model(m.cfg, "cpu", weights=str(tmp_path))
    assert torch.equal(back.lm_head, ops.untile_weight_fp8(m.lm_head_t, m.lm_head_s))
    for i in (0, 1):
        lw = m.layers[i]
        assert torch.equal(back.layers[i].qkv, ops.untile_weight_fp8(lw.qkv_t, lw.qkv_s))
        assert torch.equal(back.layers[i].gate_up, ops.untile_weight_fp8(lw.gate_up_t, lw.gate_up_s, glu=bool(lw.glu)))
        assert torch.equal(back.layers[i].down, ops.untile_weight_fp8(lw.down_t, lw.down_s))
    assert torch.equal(back.embed, m.embed)


def test_server_config_weight_dtype(monkeypatch):
    from kafka_llm_service_amd.server import __main__ as main_mod
    from kafka_llm_service_amd.server.state import ServerConfig

    for env in main_mod.FLAGS.values():
        monkeypatch.delenv(env, raising=False)
    assert main_mod.FLAGS["weight_dtype"] == "KAFKA_WEIGHT_DTYPE"
    assert "weight_dtype" not in ServerConfig.from_env().engine_kwargs
    monkeypatch.setenv("KAFKA_WEIGHT_DTYPE", "fp8")
    assert ServerConfig.from_env().engine_kwargs["weight_dtype"] == "fp8"


# ---------------------------------------------------------------------------------------------------------------- GPU
def _close(a, b, atol, msg="", rtol=0.01):
    """|a - b| <= atol + rtol * max|b| (tests/test_kernels_gpu.py)"""
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs().max().item()
    tol = atol + rtol * b.abs().max().item()
    assert err <= tol, f"{msg}: max err {err} > {tol}"


@functools.lru_cache(maxsize=None)
def _gpu_case(N, K, glu):
    """(fp8 tiles, scales, dequantised fp32 weight, x of 256 rows) on the GPU, built once per shape."""
    dev = torch.device("cuda:0")
    w = _weight(N, K, seed=N + K, device=dev)
    wt8, st = ops.tile_weight_fp8(w, glu=glu)
    deq = ops.untile_weight_fp8(wt8, st, glu=glu)
    _within_fp8(deq.float(), w.float())
    g = torch.Generator().manual_seed(11)
    x = torch.randn(256, K, generator=g).to(torch.bfloat16).to(dev)
    return wt8, st, deq.float(), x


@pytest.mark.gpu
@pytest.mark.parametrize("N,K", [(96, 256), (160, 768), (1280, 1024), (256, 1536), (6144, 4096)])
@pytest.mark.parametrize("M", [1, 33, 64, 96, 97, 128, 160, 192, 200, 256])
def test_wstream_gemm_fp8(cuda, M, N, K):
    """W8 streaming kernel (bf16 direct and split-K slabs) vs the fp32 product with the dequantised weight: every row
    tile count, 1..8 chunks, inactive tail waves, unpinned plans, KW = 2, splits up to 8."""
    wt8, st, deq, x256 = _gpu_case(N, K, False)
    x = x256[:M]
    ref_y = x.float() @ deq.t()
    for ms in (1, 8):
        plan = ops.stream_plan(M, N, K, ms)
        if plan is None:
            assert K not in (1024, 4096)
            pytest.skip(f"no stream plan for M={M} N={N} K={K}")
        y = ops.linear_stream(x, wt8, max_splits=ms, scale=st)
        if plan[2] == 1:
            assert y.dtype == torch.bfloat16 and y.shape == (M, N)
        else:
            assert ops.is_slab(y) and y.shape == (plan[2], M, N)
        _close(ops.slab_reduce(y), ref_y, atol=0.02, rtol=0.01, msg=f"wstream fp8 M={M} N={N} K={K} ms={ms}")
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("N,K", [(2048, 1024), (7168, 2048)])
@pytest.mark.parametrize("M", [1, 64, 100, 168])
def test_wstream_glu_fp8(cuda, M, N, K):
    wt8, st, deq, x256 = _gpu_case(N, K, True)
    x = x256[:M]
    y_ref = x.float() @ deq.t()
    a = ops.linear_glu(x, wt8, scale=st)
    _close(a, ref.silu_mul(y_ref.cpu()), atol=0.03, rtol=0.02, msg=f"glu fp8 M={M} N={N} K={K}")
    for ms in (1, 8):
        y = ops.linear_stream(x, wt8, max_splits=ms, glu=True, scale=st)
        if ops.is_slab(y):
            _close(ops.slab_reduce(y), y_ref, atol=0.02, rtol=0.01, msg=f"glu fp8 slab M={M} N={N} ms={ms}")
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("graphs,kv", [(False, "bf16"), (True, "bf16"), (False, "fp8")],
                         ids=["eager", "graphs", "eager-kvfp8"])
def test_engine_fp8_weights_gpu_greedy_agreement(cuda, graphs, kv, monkeypatch):
    from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
    from kafka_llm_service_amd.engine.sequence import SamplingParams

    monkeypatch.delenv("KAFKA_WEIGHT_DTYPE", raising=False)
    eng = LLMEngine(EngineConfig(model="small-llama", device=str(cuda), num_kv_blocks=1024, max_model_len=4096,
                                 weight_dtype="fp8", kv_dtype=kv, use_graphs=graphs))
    m = eng.model
    assert m.weight_dtype == "fp8" and m.layers[0].qkv_t.dtype == torch.uint8 and m.lm_head_t.dtype == torch.uint8
    assert torch.equal(m.layers[0].qkv, ops.untile_weight_fp8(m.layers[0].qkv_t, m.layers[0].qkv_s))
    g = torch.Generator().manual_seed(11)
    pre = torch.randint(0, 5000, (600,), generator=g).tolist()  # long enough for the cascade pass
    prompts = [pre + torch.randint(0, 5000, (n,), generator=g).tolist() for n in (3, 60, 150, 7)]
    outs = eng.generate(prompts, SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True))
    _assert_greedy_gap(m, prompts, outs, 0.25)


@pytest.mark.gpu
def test_engine_fp8_weights_logits_bounded_by_fp32_forward(cuda, monkeypatch):
    """The composed-numerics metric of tests/test_numerics_gpu.py on the fp8-weight engine: engine logits vs the fp32
    forward on the SAME (dequantised) weights, next to the bf16 PyTorch forward's own error; that file's bounds."""
    from test_numerics_gpu import _check, composed_errors

    from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine

    monkeypatch.delenv("KAFKA_WEIGHT_DTYPE", raising=False)
    eng = LLMEngine(EngineConfig(model="small-llama", device="cuda:0", num_kv_blocks=2048, max_model_len=4096,
                                 cascade_min_prefix=64, weight_dtype="fp8"))
    assert eng.model.layers[0].down_t.dtype == torch.uint8
    g = torch.Generator().manual_seed(11)
    cold = [torch.randint(0, 50000, (n,), generator=g).tolist() for n in (37, 150, 300)]
    _check(composed_errors(eng, cold), "fp8 weights cold")
    prefix = torch.randint(0, 50000, (400,), generator=g).tolist()
    warm = [prefix + torch.randint(0, 50000, (n,), generator=g).tolist() for n in (3, 40, 90, 7)]
    rows = composed_errors(eng, warm, warm_prefix=prefix)
    assert max(st["cascade_prefix"] for st in eng.runner.recent_stats) > 0, "the cascade did not run"
    _check(rows, "fp8 weights prefix-cached + cascade")
