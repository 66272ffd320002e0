"""MXFP4 (OCP Microscaling: e2m1 elements, 32-column blocks along K, one e8m0 exponent per block) weights for the
decode GEMMs (``weight_dtype="mxfp4"``), dequantised by v_cvt_scalef32_pk_bf16_fp4 inside the weight-streaming kernel
(MFMA stays bf16).

As with fp8 weights the mxfp4 model IS the quantised model at every step size: the row-major bf16 copy of every
quantised projection holds the dequantised values e2m1 * 2^e (exact in bf16), so prefill (hipBLASLt), decode (the W4
streaming kernel), the CPU reference path and the dense oracle all compute with the same weights and only the
accumulation order differs. Every tolerance below is therefore the one of the bf16 / fp8 test it mirrors, unchanged:
  * kernels: atol 0.02 / rtol 0.01 against x @ deq^T in fp32 (tests/test_kernels_gpu.py test_wstream_gemm; GLU
    0.03 / 0.02, test_wstream_glu);
  * engine: greedy tokens within 0.15 (CPU) / 0.25 (GPU) logits of the dense oracle (tests/test_weight_fp8.py);
  * composed numerics: the metric and bounds of tests/test_numerics_gpu.py.
Weights carry a random power of two per row (2^-3..2^3) AND per 32-column block (2^-2..2^2), so a wrong row index or a
wrong block-scale index fails. Quantisation itself is checked against the bound of the OCP rule
(e = floor(log2 amax) - 2: grid step <= |w| / 2 below the clip, clip of at most amax / 4 above 6 * 2^e):
|deq - w| <= |w| / 4 + amax_block / 8."""
import functools

import pytest
import torch

from kafka_llm_service_amd import ops
from kafka_llm_service_amd.ops import reference as ref

F4, E8 = torch.float4_e2m1fn_x2, torch.float8_e8m0fnu


def _weight(N, K, seed=0, device="cpu"):
    """bf16 [N, K], std 0.05, times a random power of two per row (2^-3..2^3) and per 32-column block (2^-2..2^2)."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) * 0.05 * torch.exp2(torch.randint(-3, 4, (N, 1), generator=g).float())
    w = w.view(N, K // 32, 32) * torch.exp2(torch.randint(-2, 3, (N, K // 32, 1), generator=g).float())
    return w.view(N, K).to(torch.bfloat16).to(device)


def _within_mxfp4(deq, w):
    N, K = w.shape
    amax = w.view(N, K // 32, 32).abs().amax(-1, keepdim=True).expand(N, K // 32, 32).reshape(N, K)
    bad = (deq - w).abs() > w.abs() / 4 + amax / 8 + 1e-12
    assert not bad.any(), f"{int(bad.sum())} elements outside the mxfp4 bound"


def _u8(t):
    return t.view(torch.uint8)


# ---------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("glu", [False, True])
def test_tile_weight_mxfp4_roundtrip(glu):
    N, K = 256, 4096
    w = _weight(N, K, seed=1)
    codes, e = ops.mxfp4_quant(w)
    assert codes.dtype == torch.uint8 and codes.shape == (N, K // 2)
    assert e.dtype == torch.uint8 and e.shape == (N, K // 32) and 7 <= int(e.min()) and int(e.max()) <= 247
    wt4, se = ops.tile_weight_mxfp4(w, glu=glu)
    assert wt4.dtype == F4 and wt4.shape == (N // 32, K // 64, 64, 16) and wt4.is_contiguous()
    assert se.dtype == E8 and se.shape == (N // 32, K // 64, 32, 2) and se.is_contiguous()
    assert ops.is_mxfp4_weight(wt4) and not ops.is_fp8_weight(wt4) and ops.tiled_dims(wt4) == (N, K)
    deq = ops.untile_weight_mxfp4(wt4, se, glu=glu)
    assert deq.dtype == torch.bfloat16 and deq.shape == (N, K)
    # codes * 2^e, spelled out: low nibble = even column, sign + 3 bits on the e2m1 grid, e8m0 bias 127
    grid = torch.tensor([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6])
    c = torch.stack((codes & 15, codes >> 4), -1).reshape(N, K).long()
    exact = (grid[c].view(N, K // 32, 32) * torch.exp2(e.float() - 127)[..., None]).view(N, K)
    assert torch.equal(deq.float(), exact)  # element for element, and exact in bf16
    assert torch.equal(exact.to(torch.bfloat16).float(), exact)
    _within_mxfp4(deq.float(), w.float())
    # the OCP shared exponent, block by block
    amax = w.float().view(N, K // 32, 32).abs().amax(-1)
    assert torch.equal(e.long(), (torch.floor(torch.log2(amax)) - 2 + 127).long())
    # lane formula, one (tile, kb4, lane): bytes 4j..4j+3 = columns 64 kb4 + 16 j + 8 h : +8 of the lane's row
    order = torch.arange(N).view(N // 32, 32)
    if glu:
        order = order.view(2, N // 64, 32).transpose(0, 1).reshape(N // 32, 32)
    nb, kb4, lane = 5, 41, 45
    r, h = lane % 32, lane // 32
    row = int(order[nb, r])
    for j in range(4):
        col = 64 * kb4 + 16 * j + 8 * h
        assert torch.equal(_u8(wt4)[nb, kb4, lane, 4 * j:4 * j + 4], codes[row, col // 2:col // 2 + 4])
    # its two scale bytes: the blocks of columns 64 kb4 : +32 and 64 kb4 + 32 : +32
    assert _u8(se)[nb, kb4, r].tolist() == e[row, 2 * kb4:2 * kb4 + 2].tolist()


def test_mxfp4_quant_rule_edges():
    """All-zero blocks get e = 127, ties round to even, values beyond 6 * 2^e saturate, the exponent clamps."""
    w = torch.zeros(1, 128)
    w[0, 32:40] = torch.tensor([4.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, -0.25])  # amax 4 -> e = 0: ties on the grid
    w[0, 64:66] = torch.tensor([7.5, -7.0])  # amax 7.5 -> e = 0: both clip to +-6
    w[0, 96] = 2.0 ** -126                    # floor(log2) - 2 + 127 = -1: clamped to 7
    codes, e = ops.mxfp4_quant(w.to(torch.bfloat16))
    assert e[0].tolist() == [127, 127, 127, 7]
    deq = ref.mxfp4_dequant(codes, e)[0]
    assert deq[:32].abs().sum() == 0
    assert deq[32:40].tolist() == [4.0, 0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 0.0]
    assert deq[64:66].tolist() == [6.0, -6.0]
    assert float(deq[96]) == 0.0  # 2^-126 / 2^-120 is below half the smallest grid step


def test_linear_stream_mxfp4_cpu_equals_dequantised():
    """CPU path: mxfp4 tiles + scale image == the same call on the bf16 tiles of the dequantised weight."""
    M, N, K = 4, 256, 1024
    g = torch.Generator().manual_seed(2)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    for glu in (False, True):
        w = _weight(N, K, seed=3)
        wt4, se = ops.tile_weight_mxfp4(w, glu=glu)
        wt = ops.tile_weight(ops.untile_weight_mxfp4(wt4, se, glu=glu), glu=glu)
        assert ops.stream_plan(M, N, K, 8)[2] > 1 and ops.stream_plan(M, N, K, 1)[2] == 1
        for ms in (1, 8):
            a = ops.linear_stream(x, wt4, max_splits=ms, glu=glu, scale=se)
            b = ops.linear_stream(x, wt, max_splits=ms, glu=glu)
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
            if glu:
                assert torch.equal(ops.linear_glu(x, wt4, max_splits=ms, scale=se), ops.linear_glu(x, wt, max_splits=ms))
    with pytest.raises(ValueError):
        ops.linear_stream(x, wt4)  # no scale image
    with pytest.raises(ValueError):
        ops.linear_glu(x, wt4)
    with pytest.raises(ValueError):
        ops.linear_stream(x, wt4, scale=_u8(se))  # not the e8m0 image
    with pytest.raises(ValueError):
        ops.linear_stream(x, wt4, scale=torch.ones(N))  # fp8-style row scales
    with pytest.raises(ValueError):
        ops.linear_stream(x, wt4, scale=se[:, :-1])  # shape does not match the tiles
    with pytest.raises(ValueError):
        ops.linear_stream(x, wt4, nt=False, scale=se)
    with pytest.raises(ValueError):
        ops.linear_stream(x[:, :512], wt4, scale=se)  # K mismatch
    # kernels that read bf16 tiles refuse the mxfp4 ones instead of misreading them
    with pytest.raises(ValueError):
        ops.linear_skinny(torch.zeros(160, K, dtype=torch.bfloat16), wt4)
    with pytest.raises(ValueError):
        ops.linear_glu_rs(x, wt4, None, 1e-5)
    with pytest.raises(ValueError):
        ops.linear_res(x, wt4, None, None, None, None)
    with pytest.raises(ValueError):
        ops.linear_qkv_rope(x, wt4, None, 1e-5, None, None, None, None, None, None, 1, 1)


def test_tile_weight_mxfp4_k_shard_is_a_slice():
    """Blocks run along K: the tiles of a K slice cut on 64-column boundaries are that slice of the full images (a
    row-parallel TP shard quantises to the matching part of the unsharded model)."""
    N, K = 64, 1024
    w = _weight(N, K, seed=5)
    wt4, se = ops.tile_weight_mxfp4(w)
    k0, k1 = 192, 704  # multiples of 64, not of 128
    st4, ss = ops.tile_weight_mxfp4(w[:, k0:k1].contiguous())
    assert torch.equal(_u8(st4), _u8(wt4)[:, k0 // 64:k1 // 64])
    assert torch.equal(_u8(ss), _u8(se)[:, k0 // 64:k1 // 64])
    assert torch.equal(ops.untile_weight_mxfp4(st4, ss), ops.untile_weight_mxfp4(wt4, se)[:, k0:k1])


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


def test_engine_mxfp4_weights_cpu(monkeypatch):
    from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
    from kafka_llm_service_amd.engine.sequence import SamplingParams
    from kafka_llm_service_amd.models.llama import LayerWeights

    monkeypatch.delenv("KAFKA_WEIGHT_DTYPE", raising=False)
    monkeypatch.delenv("KAFKA_DECODE_GEMM", raising=False)
    eng = LLMEngine(EngineConfig(**_cpu_cfg(weight_dtype="mxfp4")))
    m = eng.model
    assert m.stream and not m.tiled_only and m.weight_dtype == "mxfp4"  # auto -> stream on the CPU too
    embed = m.embed.clone()
    for lw in m.layers:
        for name in LayerWeights.STREAMED:
            wt, st = getattr(lw, name + "_t"), getattr(lw, name + "_s")
            assert wt.dtype == F4 and st.dtype == E8
            glu = name == "gate_up" and bool(lw.glu)
            assert torch.equal(getattr(lw, name), ops.untile_weight_mxfp4(wt, st, glu=glu))
    assert m.lm_head_t.dtype == F4 and m.lm_head_s.dtype == E8
    assert torch.equal(m.lm_head, ops.untile_weight_mxfp4(m.lm_head_t, m.lm_head_s))
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
    assert m.stream_weight_bytes("mxfp4") < bf16.model.stream_weight_bytes() * 0.27  # 4.25 / 16 bits
    # the environment turns the mode on for a default config
    monkeypatch.setenv("KAFKA_WEIGHT_DTYPE", "mxfp4")
    env_eng = LLMEngine(EngineConfig(**_cpu_cfg()))
    assert env_eng.model.weight_dtype == "mxfp4" and env_eng.model.layers[0].qkv_t.dtype == F4
    assert env_eng.cfg.weight_dtype == "mxfp4"
    monkeypatch.delenv("KAFKA_WEIGHT_DTYPE")
    with pytest.raises(ValueError):
        LLMEngine(EngineConfig(**_cpu_cfg(weight_dtype="mxfp4", decode_gemm="blas")))
    with pytest.raises(ValueError):
        LLMEngine(EngineConfig(**_cpu_cfg(weight_dtype="int4")))


def test_engine_mxfp4_weights_tiled_only_cpu(tmp_path, monkeypatch):
    from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
    from kafka_llm_service_amd.engine.sequence import SamplingParams
    from kafka_llm_service_amd.models.weights import build_model, save_safetensors

    monkeypatch.delenv("KAFKA_WEIGHT_DTYPE", raising=False)
    monkeypatch.delenv("KAFKA_DECODE_GEMM", raising=False)
    eng = LLMEngine(EngineConfig(**_cpu_cfg(weight_dtype="mxfp4", decode_gemm="stream_only")))
    m = eng.model
    assert m.tiled_only and m.weight_dtype == "mxfp4"
    lw = m.layers[0]
    assert lw.qkv is None and lw.o is None and lw.gate_up is None and lw.down is None and m.lm_head is None
    assert lw.qkv_t.dtype == F4 and lw.qkv_s.dtype == E8 and m.lm_head_s is not None
    calls = []
    orig = ops.untile_weight_mxfp4

    def counting(*a, **kw):
        calls.append(1)
        return orig(*a, **kw)

    monkeypatch.setattr(ops, "untile_weight_mxfp4", counting)
    prompts = _cpu_prompts()
    outs = eng.generate(prompts, SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True))
    assert calls, "prefill did not go through the dequantising untile"
    monkeypatch.setattr(ops, "untile_weight_mxfp4", orig)
    _assert_greedy_gap(m, prompts, outs, 0.15)
    save_safetensors(m, tmp_path / "model.safetensors")
    back = build_model(m.cfg, "cpu", weights=str(tmp_path))
    assert torch.equal(back.lm_head, ops.untile_weight_mxfp4(m.lm_head_t, m.lm_head_s))
    for i in (0, 1):
        lw = m.layers[i]
        assert torch.equal(back.layers[i].qkv, ops.untile_weight_mxfp4(lw.qkv_t, lw.qkv_s))
        assert torch.equal(back.layers[i].gate_up, ops.untile_weight_mxfp4(lw.gate_up_t, lw.gate_up_s, glu=bool(lw.glu)))
        assert torch.equal(back.layers[i].down, ops.untile_weight_mxfp4(lw.down_t, lw.down_s))
    assert torch.equal(back.embed, m.embed)


# ---------------------------------------------------------------------------------------------------------------- GPU
def _close(a, b, atol, msg="", rtol=0.01):
    """|a - b| <= atol + rtol * max|b| (tests/test_kernels_gpu.py)"""
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs().max().item()
    tol = atol + rtol * b.abs().max().item()
    assert err <= tol, f"{msg}: max err {err} > {tol}"


@functools.lru_cache(maxsize=None)
def _gpu_case(N, K, glu):
    """(mxfp4 tiles, scale image, dequantised fp32 weight, x of 256 rows) on the GPU, built once per shape."""
    dev = torch.device("cuda:0")
    w = _weight(N, K, seed=N + K, device=dev)
    wt4, se = ops.tile_weight_mxfp4(w, glu=glu)
    deq = ops.untile_weight_mxfp4(wt4, se, glu=glu)
    _within_mxfp4(deq.float(), w.float())
    g = torch.Generator().manual_seed(11)
    x = torch.randn(256, K, generator=g).to(torch.bfloat16).to(dev)
    return wt4, se, deq.float(), x


@pytest.mark.gpu
@pytest.mark.parametrize("N,K", [(96, 256), (160, 768), (1280, 1024), (256, 1536), (6144, 4096)])
@pytest.mark.parametrize("M", [1, 33, 64, 96, 97, 128, 160, 192, 200, 256])
def test_wstream_gemm_mxfp4(cuda, M, N, K):
    """W4 streaming kernel (bf16 direct and split-K slabs) vs the fp32 product with the dequantised weight: every row
    tile count, 1..8 chunks, inactive tail waves, unpinned plans, KW = 2, splits up to 8. The nibble order (low nibble =
    element 0 of the conversion's byte) and both scale indices are settled here: any other order misses the bound."""
    wt4, se, deq, x256 = _gpu_case(N, K, False)
    x = x256[:M]
    ref_y = x.float() @ deq.t()
    for ms in (1, 8):
        plan = ops.stream_plan(M, N, K, ms)
        if plan is None:
            assert K not in (1024, 4096)
            pytest.skip(f"no stream plan for M={M} N={N} K={K}")
        y = ops.linear_stream(x, wt4, max_splits=ms, scale=se)
        if plan[2] == 1:
            assert y.dtype == torch.bfloat16 and y.shape == (M, N)
        else:
            assert ops.is_slab(y) and y.shape == (plan[2], M, N)
        _close(ops.slab_reduce(y), ref_y, atol=0.02, rtol=0.01, msg=f"wstream mxfp4 M={M} N={N} K={K} ms={ms}")
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("N,K", [(2048, 1024), (7168, 2048)])
@pytest.mark.parametrize("M", [1, 64, 100, 168])
def test_wstream_glu_mxfp4(cuda, M, N, K):
    wt4, se, deq, x256 = _gpu_case(N, K, True)
    x = x256[:M]
    y_ref = x.float() @ deq.t()
    a = ops.linear_glu(x, wt4, scale=se)
    _close(a, ref.silu_mul(y_ref.cpu()), atol=0.03, rtol=0.02, msg=f"glu mxfp4 M={M} N={N} K={K}")
    for ms in (1, 8):
        y = ops.linear_stream(x, wt4, max_splits=ms, glu=True, scale=se)
        if ops.is_slab(y):
            _close(ops.slab_reduce(y), y_ref, atol=0.02, rtol=0.01, msg=f"glu mxfp4 slab M={M} N={N} ms={ms}")
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("graphs,kv", [(False, "bf16"), (True, "bf16"), (False, "fp8")],
                         ids=["eager", "graphs", "eager-kvfp8"])
def test_engine_mxfp4_weights_gpu_greedy_agreement(cuda, graphs, kv, monkeypatch):
    from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
    from kafka_llm_service_amd.engine.sequence import SamplingParams

    monkeypatch.delenv("KAFKA_WEIGHT_DTYPE", raising=False)
    eng = LLMEngine(EngineConfig(model="small-llama", device=str(cuda), num_kv_blocks=1024, max_model_len=4096,
                                 weight_dtype="mxfp4", kv_dtype=kv, use_graphs=graphs))
    m = eng.model
    assert m.weight_dtype == "mxfp4" and m.layers[0].qkv_t.dtype == F4 and m.lm_head_t.dtype == F4
    assert torch.equal(m.layers[0].qkv, ops.untile_weight_mxfp4(m.layers[0].qkv_t, m.layers[0].qkv_s))
    g = torch.Generator().manual_seed(11)
    pre = torch.randint(0, 5000, (600,), generator=g).tolist()  # long enough for the cascade pass
    prompts = [pre + torch.randint(0, 5000, (n,), generator=g).tolist() for n in (3, 60, 150, 7)]
    outs = eng.generate(prompts, SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True))
    _assert_greedy_gap(m, prompts, outs, 0.25)


@pytest.mark.gpu
def test_engine_mxfp4_weights_logits_bounded_by_fp32_forward(cuda, monkeypatch):
    """The composed-numerics metric of tests/test_numerics_gpu.py on the mxfp4-weight engine: engine logits vs the fp32
    forward on the SAME (dequantised) weights, next to the bf16 PyTorch forward's own error; that file's bounds."""
    from test_numerics_gpu import _check, composed_errors

    from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine

    monkeypatch.delenv("KAFKA_WEIGHT_DTYPE", raising=False)
    eng = LLMEngine(EngineConfig(model="small-llama", device="cuda:0", num_kv_blocks=2048, max_model_len=4096,
                                 cascade_min_prefix=64, weight_dtype="mxfp4"))
    assert eng.model.layers[0].down_t.dtype == F4
    g = torch.Generator().manual_seed(11)
    cold = [torch.randint(0, 50000, (n,), generator=g).tolist() for n in (37, 150, 300)]
    _check(composed_errors(eng, cold), "mxfp4 weights cold")
    prefix = torch.randint(0, 50000, (400,), generator=g).tolist()
    warm = [prefix + torch.randint(0, 50000, (n,), generator=g).tolist() for n in (3, 40, 90, 7)]
    rows = composed_errors(eng, warm, warm_prefix=prefix)
    assert max(st["cascade_prefix"] for st in eng.runner.recent_stats) > 0, "the cascade did not run"
    _check(rows, "mxfp4 weights prefix-cached + cascade")
