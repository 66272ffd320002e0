"""Plain-PyTorch fp32 reference implementations of every HIP kernel.

They define the numerics the CDNA4 kernels are tested against, and they are the CPU execution path used by the
unit tests (no GPU in CI). They use exactly the same tensor layouts as the kernels, including the paged KV layout
  K page: [num_blocks, Hkv, 16, D] holding D/8 chunk planes [D/8][16 keys][8] (k_planes / k_natural below)
  V page: [num_blocks, Hkv, D, 16]  (V^T, key offset o at vt_pos(o)).
or, for the fp8 cache (kv_dtype="fp8", ops/csrc/rope_kv.hip), uint8 pages
  K page: [num_blocks, Hkv, 16 * D + 32]: e4m3 units [D/32 j][2 h][16 keys][2 s][8 e] holding d = 32j + 16s + 8h + e,
          then int8 exponents: K of key o at 16D + o, V of key o at 16D + 16 + vt_pos(o) (value = e4m3 * 2^e)
  V page: [num_blocks, Hkv, D * 16]: e4m3 V^T [D][16], key o at vt_pos(o).
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

PAGE = 16
LOG2E = 1.4426950408889634


def vt_pos(o: torch.Tensor | int):
    """Position of key offset ``o`` inside a V^T page (swap bits 2 and 3)."""
    if isinstance(o, int):
        return (o & ~15) | (o & 3) | ((o & 4) << 1) | ((o & 8) >> 1)
    return (o & ~15) | (o & 3) | ((o & 4) << 1) | ((o & 8) >> 1)


_VT_PERM = torch.tensor([vt_pos(o) for o in range(PAGE)], dtype=torch.long)


FP8_MAX = 448.0
FP8_EXP_MIN, FP8_EXP_MAX = -100, 100


def is_fp8_cache(k_cache: torch.Tensor) -> bool:
    return k_cache.dtype == torch.uint8


def cache_head_dim(k_cache: torch.Tensor, v_cache: torch.Tensor) -> int:
    return v_cache.shape[-1] // PAGE if is_fp8_cache(k_cache) else k_cache.shape[-1]


def kv_cache_shapes(num_blocks: int, hkv: int, D: int, kv_dtype: str = "bf16"):
    """(K shape, V shape, torch dtype) of one layer's paged cache."""
    if kv_dtype == "fp8":
        return (num_blocks, hkv, PAGE * D + 32), (num_blocks, hkv, D * PAGE), torch.uint8
    if kv_dtype != "bf16":
        raise ValueError(f"kv_dtype must be bf16 or fp8, not {kv_dtype!r}")
    return (num_blocks, hkv, PAGE, D), (num_blocks, hkv, D, PAGE), torch.bfloat16


def kv_page_bytes(hkv: int, D: int, kv_dtype: str = "bf16") -> int:
    """Bytes of K + V for one 16-token page of one layer."""
    return hkv * (2 * PAGE * D + 32) if kv_dtype == "fp8" else hkv * 2 * PAGE * D * 2


def fp8_quant(x: torch.Tensor):
    """Per-vector e4m3 quantization over the last dim: (bytes uint8 [..., D], exponent int [...]) with
    x ~= e4m3(bytes) * 2^e and e = frexp exponent of amax / 448 (the kernel's rule, rope_kv.hip)."""
    x = x.float()
    amax = x.abs().amax(-1)
    _, e = torch.frexp(amax / FP8_MAX)
    e = torch.where(amax > 0, e, torch.zeros_like(e)).clamp(FP8_EXP_MIN, FP8_EXP_MAX)
    y = torch.ldexp(x, -e[..., None].float()).clamp(-FP8_MAX, FP8_MAX)
    return y.to(torch.float8_e4m3fn).view(torch.uint8), e


def tile_weight_fp8(w: torch.Tensor, glu: bool = False):
    """Row-major weight [N, K] -> (wt8 uint8 [N/32, K/32, 64, 16], st fp32 [N]): every row quantised over its whole K
    by ``fp8_quant`` (e4m3 bytes, one power-of-two scale 2^e per row) and laid out for the fp8 weight-streaming GEMM
    (csrc/wstream_gemm.hip W8): lane l = (r = l % 32, h = l // 32) of tile (nb, kb2) holds W[32 nb + r,
    32 kb2 + 8 h : +8] in bytes 0..7 (MFMA k-step 2 kb2) and W[32 nb + r, 32 kb2 + 16 + 8 h : +8] in bytes 8..15
    (k-step 2 kb2 + 1). ``st`` is in tile order: st[32 nb + r] scales the row of lane r of tile nb. ``glu``
    interleaves the 32-row tiles gate_0, up_0, gate_1, ... as ``tile_weight`` does."""
    N, K = w.shape
    if N % 32 or K % 32 or (glu and N % 64):
        raise ValueError(f"tile_weight_fp8: N={N} K={K} must be multiples of 32 (N of 64 with glu)")
    q, e = fp8_quant(w)
    t = q.reshape(N // 32, 32, K // 32, 2, 2, 8).permute(0, 2, 4, 1, 3, 5)
    s = torch.exp2(e.float()).reshape(N // 32, 32)
    if glu:
        t = t.reshape(2, N // 64, K // 32, 2, 32, 2, 8).transpose(0, 1)
        s = s.reshape(2, N // 64, 32).transpose(0, 1)
    return t.contiguous().view(N // 32, K // 32, 64, 16), s.contiguous().view(N)


def untile_weight_fp8(wt8: torch.Tensor, st: torch.Tensor, glu: bool = False) -> torch.Tensor:
    """The dequantised row-major weight e4m3 * 2^e of fp8 tiles: bf16 [N, K], exact (3 mantissa bits, and the
    exponents fp8_quant picks for bf16 inputs stay in bf16's range)."""
    nb, kb = wt8.shape[0], wt8.shape[1]
    st = st.view(nb, 32)
    if glu:
        wt8 = wt8.view(nb // 2, 2, kb, 64, 16).transpose(0, 1).reshape(nb, kb, 64, 16)
        st = st.view(nb // 2, 2, 32).transpose(0, 1).reshape(nb, 32)
    q = wt8.reshape(nb, kb, 2, 32, 2, 8).permute(0, 3, 1, 4, 2, 5).reshape(nb * 32, kb * 32)
    w = q.contiguous().view(torch.float8_e4m3fn).float() * st.reshape(nb * 32, 1)
    return w.to(torch.bfloat16)


def tile_experts_fp8(w: torch.Tensor, glu: bool = False):
    """Expert weights [E, N, K] -> (wt8 uint8 [E, N/32, K/32, 64, 16], st fp32 [E, N]): ``tile_weight_fp8`` per expert
    (every row of every expert quantised over its whole K, scales in tile order, ``glu`` the gate / up tile interleave
    of ``tile_experts``), for the grouped fp8 streaming kernel (csrc/wstream_gemm.hip, W8 grouped variant)."""
    E, N, K = w.shape
    wt8 = torch.empty(E, N // 32, K // 32, 64, 16, dtype=torch.uint8, device=w.device)
    st = torch.empty(E, N, dtype=torch.float32, device=w.device)
    for e in range(E):
        t, s = tile_weight_fp8(w[e], glu)
        wt8[e].copy_(t)
        st[e].copy_(s)
    return wt8, st


def untile_experts_fp8(wt8: torch.Tensor, st: torch.Tensor, glu: bool = False) -> torch.Tensor:
    """The dequantised row-major experts of fp8 expert tiles: bf16 [E, N, K], exact (``untile_weight_fp8``)."""
    E = wt8.shape[0]
    out = torch.empty(E, wt8.shape[1] * 32, wt8.shape[2] * 32, dtype=torch.bfloat16, device=wt8.device)
    for e in range(E):
        out[e].copy_(untile_weight_fp8(wt8[e], st[e], glu))
    return out


# MXFP4 (OCP Microscaling): 32-element blocks along K, e2m1 elements (sign + 3 bits on the grid below), one e8m0
# exponent (bias 127) per block.
MXFP4_BLOCK = 32
MXFP4_EXP_MIN, MXFP4_EXP_MAX = 7, 247  # biased: the scale uint32(e) << 23 is a normal fp32, e2m1 * 2^e a normal bf16
_E2M1_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
# magnitude code of the doubled grid value 0, 1, 2, 3, 4, 6, 8, 12
_E2M1_CODE_OF_2V = torch.tensor([0, 1, 2, 3, 4, 0, 5, 0, 6, 0, 0, 0, 7], dtype=torch.uint8)
_E2M1_VALUE = torch.tensor(_E2M1_GRID + tuple(-v for v in _E2M1_GRID), dtype=torch.float32)


def mxfp4_quant(w: torch.Tensor):
    """bf16 [N, K] (K % 64 == 0) -> (codes uint8 [N, K/2], e uint8 [N, K/32]): per 32-column block the OCP shared
    exponent e = floor(log2(amax)) - 2 (biased by 127, clamped to [7, 247]; 127 for an all-zero block) and the
    elements w / 2^e rounded to nearest-even on the e2m1 grid 0, .5, 1, 1.5, 2, 3, 4, 6, saturated to +-6. Two codes
    per byte, the even column in the LOW nibble (the order v_cvt_scalef32_pk_bf16_fp4 delivers a byte's elements)."""
    N, K = w.shape
    if K % 64:
        raise ValueError(f"mxfp4_quant: K={K} must be a multiple of 64")
    x = w.float().reshape(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
    amax = x.abs().amax(-1)
    _, ex = torch.frexp(amax)  # amax = m * 2^ex, m in [0.5, 1): floor(log2(amax)) = ex - 1
    e = torch.where(amax > 0, ex - 3 + 127, torch.full_like(ex, 127)).clamp(MXFP4_EXP_MIN, MXFP4_EXP_MAX)
    y = torch.ldexp(x, (127 - e)[..., None])
    a = y.abs().clamp(max=6.0)
    # nearest-even per binade: steps of .5 below 2, of 1 below 4, of 2 up to 6 (torch.round is half-to-even, and the
    # even multiple of the step is the code with an even mantissa bit)
    v = torch.where(a < 2.0, torch.round(a * 2.0) * 0.5, torch.where(a < 4.0, torch.round(a), torch.round(a * 0.5) * 2.0))
    mag = _E2M1_CODE_OF_2V.to(w.device)[(v * 2.0).long()]
    code = (mag | (((y < 0) & (mag > 0)).to(torch.uint8) << 3)).reshape(N, K // 2, 2)
    return code[..., 0] | (code[..., 1] << 4), e.to(torch.uint8)


def mxfp4_dequant(codes: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """(codes uint8 [N, K/2], e uint8 [N, K/32]) of ``mxfp4_quant`` -> the values e2m1 * 2^(e - 127), fp32 [N, K]
    (each one exact in bf16)."""
    N = codes.shape[0]
    c = torch.stack((codes & 15, codes >> 4), dim=-1).reshape(N, -1).long()
    v = _E2M1_VALUE.to(codes.device)[c].reshape(N, -1, MXFP4_BLOCK)
    return torch.ldexp(v, (e.int() - 127)[..., None]).reshape(N, -1)


def _glu_tiles(t: torch.Tensor, inverse: bool = False) -> torch.Tensor:
    """Tile rows [N/32, ...] between natural order and the gate_0, up_0, gate_1, ... interleave of ``tile_weight``."""
    nb = t.shape[0]
    a, b = (nb // 2, 2) if inverse else (2, nb // 2)
    return t.reshape(a, b, *t.shape[1:]).transpose(0, 1).reshape(t.shape)


def tile_weight_mxfp4(w: torch.Tensor, glu: bool = False):
    """Row-major weight [N, K] -> (wt4 float4_e2m1fn_x2 [N/32, K/64, 64, 16], se float8_e8m0fnu [N/32, K/64, 32, 2]):
    ``mxfp4_quant`` laid out for the MXFP4 weight-streaming GEMM (csrc/wstream_gemm.hip W4). Lane l = (r = l % 32,
    h = l // 32) of tile (nb, kb4) holds in bytes 4j..4j+3 (j = 0..3) the eight columns 64 kb4 + 16 j + 8 h : +8 of row
    32 nb + r — the B fragment of MFMA k-step 4 kb4 + j — so one 16-B load carries four k-steps. se[nb, kb4, r] are the
    two block exponents of row 32 nb + r for columns 64 kb4 : +32 and 64 kb4 + 32 : +32 (dwords 0, 1 and 2, 3 of that
    lane's vector): one 64-B run per (tile, kb4), independent of the kernel's plan, and a K slice on a 64-column
    boundary is a slice of both images. ``glu`` interleaves the 32-row tiles gate_0, up_0, gate_1, ... as
    ``tile_weight`` does (rows of both images in that tile order)."""
    N, K = w.shape
    if N % 32 or K % 64 or (glu and N % 64):
        raise ValueError(f"tile_weight_mxfp4: N={N} must be a multiple of 32 (64 with glu), K={K} of 64")
    codes, e = mxfp4_quant(w)
    # bytes of a row's 64-column tile: [j][h][4], byte (j, h, b) = columns 16 j + 8 h + 2 b, + 1
    t = codes.reshape(N // 32, 32, K // 64, 4, 2, 4).permute(0, 2, 4, 1, 3, 5)
    s = e.reshape(N // 32, 32, K // 64, 2).permute(0, 2, 1, 3)
    if glu:
        t, s = _glu_tiles(t), _glu_tiles(s)
    return (t.contiguous().view(N // 32, K // 64, 64, 16).view(torch.float4_e2m1fn_x2),
            s.contiguous().view(torch.float8_e8m0fnu))


def untile_weight_mxfp4(wt4: torch.Tensor, se: torch.Tensor, glu: bool = False) -> torch.Tensor:
    """The dequantised row-major weight e2m1 * 2^e of MXFP4 tiles: bf16 [N, K], exact (1 mantissa bit, normal
    exponents) and element for element ``mxfp4_dequant(*mxfp4_quant(w))``."""
    nb, kb = wt4.shape[0], wt4.shape[1]
    t, s = wt4.view(torch.uint8), se.view(torch.uint8)
    if glu:
        t, s = _glu_tiles(t, inverse=True), _glu_tiles(s, inverse=True)
    codes = t.reshape(nb, kb, 2, 32, 4, 4).permute(0, 3, 1, 4, 2, 5).reshape(nb * 32, kb * 32)
    e = s.permute(0, 2, 1, 3).reshape(nb * 32, kb * 2)
    return mxfp4_dequant(codes, e).to(torch.bfloat16)


def fp8_dequant_pages(k_pages: torch.Tensor, v_pages: torch.Tensor):
    """fp8 pages (K [n, Hkv, 16D + 32], V [n, Hkv, 16D] uint8) -> fp32 K [n, Hkv, 16, D] and V [n, Hkv, D, 16]
    (V in natural key order)."""
    n, hkv = k_pages.shape[:2]
    D = v_pages.shape[-1] // PAGE
    data = k_pages[..., :PAGE * D].contiguous().view(torch.float8_e4m3fn).float()
    k = data.view(n, hkv, D // 32, 2, PAGE, 2, 8).permute(0, 1, 4, 2, 5, 3, 6).reshape(n, hkv, PAGE, D)
    ke = k_pages[..., PAGE * D:PAGE * D + PAGE].contiguous().view(torch.int8).float()
    ve = k_pages[..., PAGE * D + PAGE:PAGE * D + 2 * PAGE].contiguous().view(torch.int8).float()
    k = k * torch.exp2(ke)[..., None]
    v = v_pages.contiguous().view(torch.float8_e4m3fn).float().view(n, hkv, D, PAGE) * torch.exp2(ve)[:, :, None, :]
    return k, v[..., _VT_PERM.to(v.device)]


def fp8_pack_pages(k: torch.Tensor, v: torch.Tensor):
    """Natural-order K, V [n, Hkv, 16, D] -> fp8 pages (K [n, Hkv, 16D + 32], V [n, Hkv, 16D] uint8), every
    (key, head) vector quantized on its own (the layout rope_kv_write produces)."""
    n, hkv, _, D = k.shape
    kq, ke = fp8_quant(k)
    vq, ve = fp8_quant(v)
    kp = torch.zeros(n, hkv, PAGE * D + 2 * PAGE, dtype=torch.uint8, device=k.device)
    kp[..., :PAGE * D] = kq.view(n, hkv, PAGE, D // 32, 2, 2, 8).permute(0, 1, 3, 5, 2, 4, 6).reshape(n, hkv, -1)
    kp[..., PAGE * D:PAGE * D + PAGE] = ke.to(torch.int8).view(torch.uint8)
    perm = _VT_PERM.to(k.device)
    kp[..., PAGE * D + PAGE + perm] = ve.to(torch.int8).view(torch.uint8)
    vt = torch.zeros(n, hkv, D, PAGE, dtype=torch.uint8, device=k.device)
    vt[..., perm] = vq.transpose(2, 3)
    return kp, vt.reshape(n, hkv, D * PAGE)


def k_planes(k_cache: torch.Tensor) -> torch.Tensor:
    """View of a K cache [nb, Hkv, 16, D] as its chunk planes [nb, Hkv, D/8, 16 keys, 8] (the memory layout)."""
    nb, hkv, _, D = k_cache.shape
    return k_cache.view(nb, hkv, D // 8, PAGE, 8)


def k_natural(k_pages: torch.Tensor) -> torch.Tensor:
    """K pages [n, Hkv, 16, D] as stored -> [n, Hkv, 16 keys, D] in natural (key, d) order."""
    n, hkv, _, D = k_pages.shape
    return k_pages.reshape(n, hkv, D // 8, PAGE, 8).permute(0, 1, 3, 2, 4).reshape(n, hkv, PAGE, D)


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    xf = x.float()
    r = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (xf * r * w.float()).to(x.dtype)


def fused_add_rmsnorm(x: torch.Tensor, residual: torch.Tensor, w: torch.Tensor, eps: float):
    s = (x.float() + residual.float()).to(residual.dtype)
    return rmsnorm(s, w, eps), s


def silu_mul(x: torch.Tensor) -> torch.Tensor:
    F = x.shape[-1] // 2
    g, u = x[..., :F].float(), x[..., F:].float()
    return (torch.nn.functional.silu(g) * u).to(x.dtype)


def rope_kv_write(qkv, positions, cos_sin, q_out, k_cache, v_cache, slot_mapping, Hq: int, Hkv: int) -> None:
    T = qkv.shape[0]
    D = cache_head_dim(k_cache, v_cache)
    half = D // 2
    x = qkv.float().view(T, Hq + 2 * Hkv, D)
    cs = cos_sin[positions.long()].float()  # [T, D]
    cos, sin = cs[:, None, :half], cs[:, None, half:]
    qk = x[:, : Hq + Hkv]
    x1, x2 = qk[..., :half], qk[..., half:]
    rot32 = torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)
    rot = rot32.to(qkv.dtype)
    q_out.copy_(rot[:, :Hq])
    if slot_mapping is None:
        return
    if is_fp8_cache(k_cache):
        kq, ke = fp8_quant(rot32[:, Hq:])
        vq, ve = fp8_quant(x[:, Hq + Hkv:])
        kd = kq.view(T, Hkv, D // 32, 2, 2, 8).permute(0, 1, 2, 4, 3, 5)  # (j, s, h, e) -> (j, h, s, e)
        for t in range(T):
            s = int(slot_mapping[t])
            if s < 0:
                continue
            blk, off = divmod(s, PAGE)
            k_cache[blk, :, :PAGE * D].view(Hkv, D // 32, 2, PAGE, 2, 8)[:, :, :, off] = kd[t]
            k_cache[blk, :, PAGE * D + off] = ke[t].to(torch.int8).view(torch.uint8)
            k_cache[blk, :, PAGE * D + PAGE + vt_pos(off)] = ve[t].to(torch.int8).view(torch.uint8)
            v_cache[blk].view(Hkv, D, PAGE)[:, :, vt_pos(off)] = vq[t]
        return
    k = rot[:, Hq:]
    v = x[:, Hq + Hkv:].to(qkv.dtype)
    for t in range(T):
        s = int(slot_mapping[t])
        if s < 0:
            continue
        blk, off = divmod(s, PAGE)
        k_planes(k_cache)[blk, :, :, off, :] = k[t].reshape(Hkv, D // 8, 8)
        v_cache[blk, :, :, vt_pos(off)] = v[t]


def gather_kv(k_cache, v_cache, block_table, length: int):
    """Materialise [length, Hkv, D] K and V for one sequence from the paged caches (fp32)."""
    nb = (length + PAGE - 1) // PAGE
    ids = block_table[:nb].long()
    if is_fp8_cache(k_cache):
        k, v = fp8_dequant_pages(k_cache[ids], v_cache[ids])
    else:
        k = k_natural(k_cache[ids].float())  # [nb, Hkv, 16, D]
        v = v_cache[ids].float()  # [nb, Hkv, D, 16]
        v = v[..., _VT_PERM.to(v.device)]  # undo the page permutation -> [nb, Hkv, D, 16] natural key order
    k = k.permute(0, 2, 1, 3).reshape(nb * PAGE, k.shape[1], k.shape[3])[:length]
    v = v.permute(0, 3, 1, 2).reshape(nb * PAGE, v.shape[1], v.shape[2])[:length]
    return k, v


def _attend(q, k, v, mask, scale):
    """q [M, G, D], k/v [N, D] (one kv head), mask [M, N] bool -> (o [M, G, D], lse2 [M, G])."""
    s = torch.einsum("mgd,nd->mgn", q, k) * scale
    s = s.masked_fill(~mask[:, None, :], float("-inf"))
    m = s.amax(-1, keepdim=True)
    m_use = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    p = torch.exp(s - m_use)
    l = p.sum(-1, keepdim=True)
    o = torch.einsum("mgn,nd->mgd", p, v) / torch.where(l > 0, l, torch.ones_like(l))
    lse = torch.where(l[..., 0] > 0, (m_use[..., 0] + torch.log(l[..., 0])) * LOG2E,
                      torch.full_like(l[..., 0], float("-inf")))
    return o, lse


def attn_decode_full(q, k_cache, v_cache, block_tables, seq_lens, scale, kv_start=None):
    """Reference single-token paged attention over keys [kv_start, seq_len). q [B, Hq, D] -> (o fp32, lse2)."""
    B, Hq, D = q.shape
    Hkv = k_cache.shape[1]
    G = Hq // Hkv
    out = torch.zeros(B, Hq, D, dtype=torch.float32, device=q.device)
    lse = torch.full((B, Hq), float("-inf"), dtype=torch.float32, device=q.device)
    for b in range(B):
        L = int(seq_lens[b])
        s0 = int(kv_start[b]) if kv_start is not None else 0
        if L <= s0:
            continue
        k, v = gather_kv(k_cache, v_cache, block_tables[b], L)
        for h in range(Hkv):
            qh = q[b, h * G:(h + 1) * G].float()[None]
            mask = torch.zeros(1, L, dtype=torch.bool, device=q.device)
            mask[:, s0:L] = True
            o, l2 = _attend(qh, k[:, h], v[:, h], mask, scale)
            out[b, h * G:(h + 1) * G] = o[0]
            lse[b, h * G:(h + 1) * G] = l2[0]
    return out, lse


def attn_decode_items(q, k_cache, v_cache, block_tables, items, out_part, lse_part, scale, out=None,
                      pre_part=None):
    """Reference for the work-item decode kernel (ops/csrc/attention.hip attn_decode_kernel). ``pre_part`` (bf16,
    out_part's shape): the cascade's prefix partials (slots < npre) are read from it instead of out_part."""
    B, Hq, D = q.shape
    Hkv = k_cache.shape[1]
    G = Hq // Hkv
    S_total = out_part.shape[2]
    lp = lse_part.view(out_part.shape[0], Hq, S_total)
    nparts, npres = {}, {}
    for b, lo, hi, split, nsplit, npre in (it[:6] for it in items.tolist()):
        if not (0 <= b < B and 0 <= split < nsplit and npre >= 0 and npre + nsplit <= S_total):
            continue  # padding / malformed item: dropped, as by the kernel
        nparts[b] = npre + nsplit
        npres[b] = npre
        o = torch.zeros(Hq, D, dtype=torch.float32, device=q.device)
        l2 = torch.full((Hq,), float("-inf"), dtype=torch.float32, device=q.device)
        if hi > lo:
            k, v = gather_kv(k_cache, v_cache, block_tables[b], hi)
            mask = torch.zeros(1, hi, dtype=torch.bool, device=q.device)
            mask[:, lo:hi] = True
            for h in range(Hkv):
                oh, lh = _attend(q[b, h * G:(h + 1) * G].float()[None], k[:, h], v[:, h], mask, scale)
                o[h * G:(h + 1) * G] = oh[0]
                l2[h * G:(h + 1) * G] = lh[0]
        out_part[b, :, npre + split] = o
        lp[b, :, npre + split] = l2
    if out is not None:
        for b, n in nparts.items():
            parts = out_part[b:b + 1, :, :n].clone()
            if pre_part is not None:
                parts[:, :, :npres[b]] = pre_part[b:b + 1, :, :npres[b]].float()
            attn_merge(parts.contiguous(), lp[b:b + 1, :, :n].contiguous(), out[b:b + 1])


def attn_prefill_items(items, q, k_cache, v_cache, block_tables, q_limit, scale, out=None, out_part=None,
                       lse_part=None, alt_part=None, alt_lse=None, alt_tok_off=0):
    """Reference for the work-item prefill / cascade kernel (see ops/csrc/attention.hip, attn_tile.hip); items with
    field 6 set write their partial to alt_part / alt_lse at row token - alt_tok_off."""
    T, Hq, D = q.shape
    Hkv = k_cache.shape[1]
    G = Hq // Hkv
    for it in items.tolist():
        q_start, q_count, bt_row, lo, hi, split = it[:6]
        if q_count <= 0:
            continue
        toks = torch.arange(q_start, q_start + q_count, device=q.device)
        lim = q_limit[toks].long()
        kmax = int(min(hi, int(lim.max()) + 1))
        if kmax <= lo:
            o = torch.zeros(q_count, Hq, D, device=q.device)
            l2 = torch.full((q_count, Hq), float("-inf"), device=q.device)
        else:
            k, v = gather_kv(k_cache, v_cache, block_tables[bt_row], kmax)
            pos = torch.arange(kmax, device=q.device)
            mask = (pos[None] >= lo) & (pos[None] < hi) & (pos[None] <= lim[:, None])
            o = torch.zeros(q_count, Hq, D, device=q.device)
            l2 = torch.zeros(q_count, Hq, device=q.device)
            for h in range(Hkv):
                oh, lh = _attend(q[toks, h * G:(h + 1) * G].float(), k[:, h], v[:, h], mask, scale)
                o[:, h * G:(h + 1) * G] = oh
                l2[:, h * G:(h + 1) * G] = lh
        if split < 0:
            out[toks] = o.to(out.dtype)
        elif it[6] and alt_part is not None:
            rows = toks - alt_tok_off
            alt_part[rows, :, split] = o.to(alt_part.dtype)
            alt_lse.view(alt_part.shape[0], Hq, alt_part.shape[2])[rows, :, split] = l2
        else:
            out_part[toks, :, split] = o.to(out_part.dtype)
            lse_part.view(out_part.shape[0], Hq, out_part.shape[2])[toks, :, split] = l2


def attn_merge(part, lse, out, lse_out=None, pre=None, npre=0):
    rows = out.shape[0]
    p = part[:rows].float()
    if pre is not None and npre:  # bf16 prefix partials in slots [0, npre)
        p = p.clone()
        p[:, :, :npre] = pre[:rows, :, :npre].float()
    l = lse.view(part.shape[0], part.shape[1], part.shape[2])[:rows]
    M = l.amax(-1, keepdim=True)
    Mu = torch.where(torch.isinf(M), torch.zeros_like(M), M)
    f = torch.exp2(l - Mu)
    L = f.sum(-1, keepdim=True)
    pz = torch.where(f[..., None] > 0, p, torch.zeros_like(p))  # unwritten slots (lse -inf) may hold anything
    o = (f[..., None] * pz).sum(2) / torch.where(L > 0, L, torch.ones_like(L))
    out.copy_(o.to(out.dtype))
    if lse_out is not None:
        lse_out.view(rows, -1).copy_(torch.where(L[..., 0] > 0, Mu[..., 0] + torch.log2(L[..., 0]),
                                                 torch.full_like(L[..., 0], float("-inf"))))


LOGIT_BIAS_MAX = 300  # entries of one bias_tab row (csrc/kafka_abi.h): ids at [0, n), fp32 bits at [LOGIT_BIAS_MAX, ..)
COUNT_SEEN_PROMPT = 1 << 30  # flag of a prompt token in a count word (csrc/kafka_abi.h); the count is the bits below


def process_logits(logits, proc, mask_tab, counts, bias_tab=None, rep_tab=None):
    """The sampler's per-row logits processing (csrc/sampling.hip RowProc) in fp32: penalties from the row's token
    counts, then the row's sparse logit bias — ``(y - freq * c - (c > 0 ? pres : 0)) + b``, one fp32 add after the
    penalty arithmetic — then the grammar bitmask (-inf where a bit is 0, whatever the bias). Returns (processed fp32
    logits, forced ids or -1).

    ``rep_tab`` (fp32 [slots, 2] = (r, inv_r), inv_r = float32(1) / float32(r) from the host; None or r == 1: off) is
    the repetition penalty: ``y = x`` unless the row's count word of the token is non-zero (a prompt token carries
    COUNT_SEEN_PROMPT, a generated one its count), then ``y = x * inv_r`` for ``x > 0`` and ``y = x * r`` otherwise —
    one fp32 multiply rounded on its own, never a division, so ``y`` is within one fp32 ulp of ``x / r``. ``c`` is the
    generated count, the word without the flag. Forced rows ignore it."""
    B, V = logits.shape
    x = logits.float().clone()
    forced = torch.full((B,), -1, dtype=torch.long)
    pr = proc[:B].cpu()
    for b in range(B):
        mode, arg, slot = int(pr[b, 0]), int(pr[b, 1]), int(pr[b, 2])
        pres, freq = pr[b, 3:5].clone().view(torch.float32).tolist()
        if mode == 2:
            forced[b] = arg
            continue
        if slot >= 0:
            word = counts[slot, :V].to(x.device)
            if rep_tab is not None and float(rep_tab[slot, 0]) != 1.0:
                r, inv_r = (rep_tab[slot, j].to(device=x.device, dtype=torch.float32) for j in (0, 1))
                x[b] = torch.where(word != 0, torch.where(x[b] > 0, x[b] * inv_r, x[b] * r), x[b])
            c = (word & (COUNT_SEEN_PROMPT - 1)).float()
            x[b] -= freq * c + pres * (c > 0).float()
        nb = min(int(pr[b, 6]), LOGIT_BIAS_MAX)  # (the kernel's clamp)
        if nb > 0:
            if bias_tab is None:
                raise ValueError("process_logits: a proc row carries logit-bias entries but no bias_tab was given")
            row = bias_tab[int(pr[b, 5])].cpu()
            ids = row[:nb].long().to(x.device)
            x[b, ids] += row[LOGIT_BIAS_MAX:LOGIT_BIAS_MAX + nb].clone().view(torch.float32).to(x.device)
        if mode == 1:
            words = mask_tab[arg].to(torch.int64) & 0xFFFFFFFF
            bits = (words[:, None] >> torch.arange(32)) & 1
            keep = bits.reshape(-1)[:V].bool().to(x.device)
            x[b].masked_fill_(~keep, float("-inf"))
    return x, forced


def sample(logits, temperature=None, top_p=None, top_k=None, seeds=None, step=None, out=None, proc=None,
           mask_tab=None, counts=None, bias_tab=None, rep_tab=None):
    """CPU sampler with the same semantics (not the same random stream) as the HIP kernel: the sort-based definition
    of top-k / top-p and the CPU engine path. ``proc[:, 7]`` (the fp32 bits of ln(min_p), 0 = off) adds the min_p
    set ``x / T >= max(x / T) + ln(min_p)`` with the kernel's fp32 threshold, intersected with the other two; greedy
    and forced rows ignore it. ``rep_tab``: the repetition penalty of ``process_logits`` (one fp32 multiply by the
    host's reciprocal, within one fp32 ulp of x / r) over the row's seen tokens. ``sample_replay`` below reproduces
    the kernel's own stream and decisions draw by draw."""
    B, V = logits.shape
    forced = None
    if proc is not None:
        x, forced = process_logits(logits, proc, mask_tab, counts, bias_tab, rep_tab)
    else:
        x = logits.float()
    res = torch.empty(B, dtype=torch.long, device=logits.device)
    for b in range(B):
        if forced is not None and int(forced[b]) >= 0:
            res[b] = int(forced[b])
            continue
        t = float(temperature[b]) if temperature is not None else 0.0
        if not t > 0:
            res[b] = int(torch.argmax(x[b]))
            continue
        z = x[b] / t
        p = torch.softmax(z, -1)
        tp = float(top_p[b]) if top_p is not None else 1.0
        tk = int(top_k[b]) if top_k is not None else 0
        order = torch.argsort(p, descending=True)
        ps = p[order]
        keep = torch.ones(V, dtype=torch.bool, device=p.device)
        if tk > 0:
            keep[tk:] = False
        if tp < 1.0:
            above = torch.cumsum(ps, 0) - ps
            keep &= above < tp
        if proc is not None and int(proc[b, 7]) != 0:  # min_p: xv >= max + ln(min_p), the kernel's fp32 threshold
            lmp = proc[b, 7:8].cpu().clone().view(torch.float32)[0]
            xv = x[b] * (torch.tensor(1.0) / torch.tensor(t, dtype=torch.float32)).to(x.device)
            keep &= (xv >= xv.max() + lmp.to(x.device))[order]
        ps = torch.where(keep, ps, torch.zeros_like(ps))
        gen = torch.Generator(device="cpu")
        seed = int(seeds[b]) if seeds is not None else 0x1234
        stepv = int(step[0]) if step is not None else 0
        gen.manual_seed((seed * 1000003 + stepv) & 0x7FFFFFFFFFFFFFFF)
        idx = torch.multinomial(ps.cpu() / ps.sum().cpu(), 1, generator=gen)
        res[b] = order[idx.to(order.device)]
    if proc is not None and counts is not None:
        for b in range(B):
            slot = int(proc[b, 2])
            if slot >= 0:
                counts[slot, int(res[b])] += 1
    if out is not None:
        out[:B].copy_(res)
        return out
    return res


# ---- sample_replay: the sampler kernel's algorithm with the kernel's own random stream -------------------------------
# The noise of csrc/sampling.hip is a pure integer function of (seed, step, round, index) (mix64 / uniform01 of
# csrc/common.h, lowbias32 / gumbel_fast of csrc/sampling.hip) and its uniform u = (h + 1) * 2^-24 is exact in fp32, so
# the stream is reproduced bit for bit with wrapping numpy integers. x / T is formed in fp32 exactly as the kernel forms
# it (its exact ties are the replay's exact ties); everything after that (Gumbel noise, scores, max, z, mass) is float64.
# Where the float64 decision is closer than a band to going the other way the row is flagged ``ambiguous``: the kernel's
# fp32 arithmetic may legitimately decide it either way. The bands come from fp32 arithmetic, not from a kernel run:
#   score band on x / T + g: scores stay below ~64 in magnitude, so one fp32 ulp is at most 3.8e-6; 1e-4 is ~25 ulps for
#     the two native logarithms and the add;
#   mass band on mass / z: fp32 sums of 1024 partial sums and the native exp on arguments up to ~50 in magnitude are of
#     the order of 1e-5 relative.
SAMPLE_SCORE_BAND = 1e-4
SAMPLE_MASS_BAND = 1e-4
SAMPLE_MAX_ROUNDS = 32                                           # the launcher's max_rounds
_U_CLAMP = float(np.float32(1.0) - np.float32(2.0 ** -24))      # the kernel's 0.99999994f: only u == 1 is clamped
_NO_IDX = 0x7FFFFFFF                                             # ArgMax's "nothing yet" index
_STREAM_MUL = np.uint64(0x632BE59BD9B4E019)


class SampleReplay(NamedTuple):
    tokens: torch.Tensor     # int64 [B]
    ambiguous: torch.Tensor  # bool [B]: some decision of the row lies within a band (the kernel may differ there)
    rounds: torch.Tensor     # int64 [B]: draws of the rejection loop (0 for greedy / plain / forced rows)
    fell_back: torch.Tensor  # bool [B]: the loop ended without an accepted draw (token = argmax)
    plain: torch.Tensor      # bool [B]: drawn from the plain-temperature stream (gumbel_fast), not the filtered one
    rescans: torch.Tensor    # int64 [B]: slices of a min_p-only row whose own winner fell below the row's threshold


def _mix64(z: np.ndarray) -> np.ndarray:
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _lowbias32(x: np.ndarray) -> np.ndarray:
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7FEB352D)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846CA68B)
    return x ^ (x >> np.uint32(16))


def _gumbel(h24: np.ndarray) -> np.ndarray:
    """Gumbel noise of the 24-bit integers h: u = (h + 1) * 2^-24 in (0, 1], exact in fp32 and in float64."""
    u = np.minimum((h24.astype(np.float64) + 1.0) * 2.0 ** -24, _U_CLAMP)
    return -np.log(-np.log(u))


def _first_max(s: np.ndarray):
    """Per row (max, index) the way the kernel's ``better`` reduces from (-inf, 0x7fffffff): NaN never wins and the
    lowest index wins among equals; a row with nothing to compare keeps (-inf, 0x7fffffff)."""
    R = s.shape[0]
    if s.shape[1] == 0:
        return np.full(R, -np.inf), np.full(R, _NO_IDX, dtype=np.int64)
    ok = ~np.isnan(s)
    m = np.where(ok, s, -np.inf).max(1)
    hit = ok & (s == m[:, None])
    return m, np.where(hit.any(1), hit.argmax(1), _NO_IDX).astype(np.int64)


def _min_p_threshold(xv, lmp):
    """Per row the fp32 threshold max(xv) + lmp (one fp32 add; fmaxf drops a NaN) — -inf where lmp is NaN (no min_p)."""
    mx = np.where(np.isnan(xv), np.float32(-np.inf), xv).max(1) if xv.shape[1] else np.full(xv.shape[0], -np.inf)
    thr = mx.astype(np.float32) + np.where(np.isnan(lmp), np.float32(0), lmp).astype(np.float32)
    return np.where(np.isnan(lmp), np.float32(-np.inf), thr).astype(np.float32)


def _replay_plain(xv, greedy, seeds, steps, nsplit, lmp=None):
    """Greedy / plain-temperature rows: argmax of x (greedy) or x / T + gumbel_fast over ``nsplit`` slices of the row
    and the reduction of the slices' winners, as the split workgroups do. ``lmp`` (fp32 [R], NaN = none): ln(min_p) of
    a min_p row — its slices draw over {xv >= slice max + lmp}, and the last workgroup keeps a slice's winner if it
    passes the row's threshold, drops a slice whose maximum does not, and rescans a slice whose winner fell below it
    (sample_min_p_split); the same draw over the row's kept set must give the same token.
    -> (token, ambiguous, rescans)."""
    R, V = xv.shape
    key = _mix64(seeds ^ _mix64((steps << np.uint64(8)) * _STREAM_MUL))
    idx = np.arange(V, dtype=np.uint32)[None, :]
    h = _lowbias32(_lowbias32(idx + key.astype(np.uint32)[:, None]) ^ (key >> np.uint64(32)).astype(np.uint32)[:, None])
    s = xv.astype(np.float64)
    s = np.where(greedy[:, None], s, s + _gumbel(h >> np.uint32(8)))
    on = np.zeros(R, dtype=bool) if lmp is None else (~np.isnan(lmp) & ~greedy)
    lmp = np.where(on, lmp, np.float32(np.nan)).astype(np.float32) if on.any() else None
    nvec = V >> 3
    per = -(-nvec // nsplit)
    vals = np.full((R, nsplit), -np.inf)
    ids = np.full((R, nsplit), _NO_IDX, dtype=np.int64)
    ms = np.full((R, nsplit), -np.inf, dtype=np.float32)  # min_p rows: the slices' maxima
    slices = []
    for sp in range(nsplit):
        v0 = sp * per
        v1 = min(nvec, v0 + per)
        cols = np.r_[v0 * 8:max(v0, v1) * 8, (nvec * 8 if sp == nsplit - 1 else V):V]  # the last split owns the tail
        slices.append(cols)
        sc = s[:, cols]
        if lmp is not None and cols.size:
            xs = xv[:, cols]
            ms[:, sp] = np.where(np.isnan(xs), np.float32(-np.inf), xs).max(1)  # (fmaxf drops a NaN)
            thr_s = ms[:, sp] + lmp  # one fp32 add (NaN in the other rows, which keep every score)
            sc = np.where(on[:, None] & ~(xs >= thr_s[:, None]), np.nan, sc)
        vals[:, sp], i = _first_max(sc)
        if cols.size:
            ids[:, sp] = np.where(i != _NO_IDX, cols[np.minimum(i, cols.size - 1)], _NO_IDX)
    r = np.arange(R)
    rescans = np.zeros(R, dtype=np.int64)
    kept = s
    if lmp is not None:  # the last workgroup of a min_p row
        thr = ms.max(1) + lmp  # fp32
        for sp, cols in enumerate(slices):
            w = ids[:, sp]
            has = on & (ms[:, sp] >= thr) & (w != _NO_IDX)
            redo = has & ~(xv[r, np.minimum(w, V - 1)] >= thr)
            none = on & ~has
            vals[none, sp], ids[none, sp] = np.nan, _NO_IDX
            if redo.any():
                rescans[redo] += 1
                q = np.nonzero(redo)[0]
                sub = xv[np.ix_(q, cols)]
                vals[q, sp], i = _first_max(np.where(sub >= thr[q, None], s[np.ix_(q, cols)], np.nan))
                ids[q, sp] = np.where(i != _NO_IDX, cols[np.minimum(i, cols.size - 1)], _NO_IDX)
        kept = np.where(on[:, None] & ~(xv >= thr[:, None]), np.nan, s)
    dead = np.isnan(vals)  # (a min_p slice that contributes nothing; a plain slice's value is never NaN)
    vm = np.where(dead, -np.inf, vals)
    m = vm.max(1)
    tok = np.where((vm == m[:, None]) & ~dead, ids, _NO_IDX).min(1)
    if lmp is not None:  # the split draw is the draw over the row's kept set
        whole = _first_max(kept)[1]
        assert (tok[on] == whole[on]).all(), "min_p replay: the sliced draw and the draw over the kept set differ"
    tok = np.where((tok >= 0) & (tok < V), tok, 0)  # emit_token: an index outside the vocabulary becomes 0
    # greedy compares the fp32 values themselves (exact, lowest index among equals): never ambiguous
    rest = kept.copy()
    rest[r, tok] = -np.inf
    amb = ~greedy & (kept[r, tok] - _first_max(rest)[0] < SAMPLE_SCORE_BAND)
    return tok, amb, rescans


def _replay_filtered(x, xv, tp, tk, seeds, steps, lmp=None):
    """top-k / top-p rows: the rejection loop round by round. x: the processed fp32 logits (the fallback's argmax),
    xv = x / T in fp32; ``lmp`` (fp32 [R], NaN = none): a candidate also passes xv >= max + ln(min_p), compared in
    fp32 as the kernel compares it (no band). -> (token, ambiguous, rounds, fell_back)."""
    R, V = xv.shape
    thr = _min_p_threshold(xv, np.full(R, np.nan, dtype=np.float32) if lmp is None else lmp)
    xd = xv.astype(np.float64)
    e = np.exp(xd - _first_max(xd)[0][:, None])
    z = e.sum(1)
    pivot = np.full(R, -np.inf, dtype=np.float32)
    tok = np.full(R, -1, dtype=np.int64)
    rounds = np.zeros(R, dtype=np.int64)
    amb = np.zeros(R, dtype=bool)
    base = steps << np.uint64(8)
    live = np.arange(R)
    for rnd in range(SAMPLE_MAX_ROUNDS):
        # strict: tokens tied with the pivot are out (thr is -inf without min_p, and a NaN fails the first test already)
        cand = (xv[live] > pivot[live, None]) & (xv[live] >= thr[live, None])
        n = cand.sum(1)
        live, cand, n = live[n > 0], cand[n > 0], n[n > 0]  # nothing above the pivot ends the loop (fallback)
        if live.size == 0:
            break
        rounds[live] += 1
        r, c = np.nonzero(cand)  # row-major: one contiguous segment per live row
        rows = live[r]
        stream = (base[rows] ^ np.uint64(rnd)) * _STREAM_MUL + c.astype(np.uint64)
        s = xd[rows, c] + _gumbel(_mix64(seeds[rows] ^ _mix64(stream)) >> np.uint64(40))
        start = np.cumsum(n) - n
        best = np.maximum.reduceat(s, start)
        ci = np.minimum.reduceat(np.where(s == best[r], c, V), start)  # lowest index among equal scores
        second = np.maximum.reduceat(np.where(c == ci[r], -np.inf, s), start)
        xc = xv[live, ci]
        above = xv[live] > xc[:, None]  # strict: tokens tied with the candidate count toward neither k nor the mass
        cnt = above.sum(1)
        mass = np.where(above, e[live], 0.0).sum(1) / z[live]
        ok = (mass < tp[live]) & ((tk[live] <= 0) | (cnt < tk[live]))
        amb[live] |= (best - second < SAMPLE_SCORE_BAND) | (np.abs(mass - tp[live]) < SAMPLE_MASS_BAND)
        tok[live[ok]] = ci[ok]
        pivot[live[~ok]] = xc[~ok]
        live = live[~ok]
    fell = tok < 0
    if fell.any():  # argmax of the processed logits (not divided by T), lowest index among equals
        i = _first_max(x[fell].astype(np.float64))[1]
        tok[fell] = np.where((i >= 0) & (i < V), i, 0)
    return tok, amb, rounds, fell


def sample_replay(logits, temperature=None, top_p=None, top_k=None, seeds=None, step=None, out=None, proc=None,
                  mask_tab=None, counts=None, nsplit: int = 1, bias_tab=None, rep_tab=None) -> SampleReplay:
    """CPU replay of csrc/sampling.hip with the kernel's own random stream: the arguments of ``ops.sample`` plus
    ``nsplit`` (the workgroups a greedy / plain-temperature row is split over; it must not change the result). Every
    row whose ``ambiguous`` flag is clear has exactly one right token and the kernel must return it. Logits are finite
    or -inf. ``step`` holds one value as for the kernel, or (replay only) one per row. ``counts`` is bumped with every
    token like the kernel bumps it. min_p (``proc[:, 7]``) is a threshold max + ln(min_p) formed and compared in fp32
    exactly as the kernel does, so it adds no ambiguity band; ``rescans`` counts, per min_p-only row, the slices the
    kernel's last workgroup reads again. ``rep_tab``: the repetition penalty, formed by ``process_logits`` in one fp32
    multiply by the host's reciprocal as the kernel forms it (within one fp32 ulp of x / r): no band either."""
    B, V = logits.shape
    assert 1 <= nsplit <= 64
    forced = None
    if proc is not None:
        x, forced = process_logits(logits, proc, mask_tab, counts, bias_tab, rep_tab)
    else:
        x = logits.float()
    x = x.cpu().contiguous().numpy()

    def arg(t, dtype, default):
        if t is None:
            return np.full(B, default, dtype=dtype)
        return np.ascontiguousarray(t.detach().cpu().numpy()[:B].astype(dtype, copy=False))

    temp = arg(temperature, np.float32, 0.0)
    tp = arg(top_p, np.float32, 1.0).astype(np.float64)
    tk = arg(top_k, np.int64, 0)
    sd = arg(seeds, np.int64, 0x1234).view(np.uint64)  # int64 reinterpreted: negative seeds are legal
    st = np.zeros(1, dtype=np.int64) if step is None else step.detach().cpu().numpy().astype(np.int64).reshape(-1)
    st = np.ascontiguousarray(np.broadcast_to(st if st.size == B else st[:1], (B,))).view(np.uint64)
    tokens = np.zeros(B, dtype=np.int64)
    amb = np.zeros(B, dtype=bool)
    rounds = np.zeros(B, dtype=np.int64)
    fell = np.zeros(B, dtype=bool)
    rescans = np.zeros(B, dtype=np.int64)
    lmp = None  # proc[7]: the fp32 bits of ln(min_p), 0 = none (NaN here)
    if proc is not None:
        bits = np.ascontiguousarray(proc[:B, 7].detach().cpu().numpy().astype(np.int32))
        if bits.any():
            lmp = np.where(bits != 0, bits.view(np.float32), np.float32(np.nan)).astype(np.float32)
    with np.errstate(all="ignore"):
        greedy = ~(temp > 0)
        inv_t = np.where(greedy, np.float32(1.0), np.float32(1.0) / temp).astype(np.float32)
        is_forced = forced.numpy() >= 0 if forced is not None else np.zeros(B, dtype=bool)
        filtered = ~greedy & ((tp < 1.0) | ((tk > 0) & (tk < V))) & ~is_forced
        plain = ~filtered & ~is_forced
        tokens[is_forced] = forced.numpy()[is_forced] if forced is not None else 0
        tokens[is_forced & ((tokens < 0) | (tokens >= V))] = 0
        chunk = max(1, (1 << 22) // max(V, 1))  # rows per pass: bounds the float64 temporaries
        for sel, filt in ((np.nonzero(plain)[0], False), (np.nonzero(filtered)[0], True)):
            for i in range(0, sel.size, chunk):
                rows = sel[i:i + chunk]
                xv = x[rows] * inv_t[rows, None]  # fp32 product, as the kernel forms it
                lm = None if lmp is None else lmp[rows]
                if filt:
                    tokens[rows], amb[rows], rounds[rows], fell[rows] = _replay_filtered(x[rows], xv, tp[rows], tk[rows],
                                                                                        sd[rows], st[rows], lm)
                else:
                    tokens[rows], amb[rows], rescans[rows] = _replay_plain(xv, greedy[rows], sd[rows], st[rows], nsplit,
                                                                           lm)
    res = torch.from_numpy(tokens)
    if proc is not None and counts is not None:
        for b in range(B):
            slot = int(proc[b, 2])
            if slot >= 0:
                counts[slot, int(res[b])] += 1
    if out is not None:
        out[:B].copy_(res)
    return SampleReplay(res, torch.from_numpy(amb), torch.from_numpy(rounds), torch.from_numpy(fell),
                        torch.from_numpy(plain & ~greedy), torch.from_numpy(rescans))


def token_logprobs(logits, tokens, rows=None, k: int = 0):
    """fp32 reference of csrc/logprobs.hip: for each scored row r (``rows``, default every row) of the RAW logits,
    (log softmax at tokens[row], the k largest log-probabilities, their ids) as (tok_lp [R] f32, top_lp [R, k] f32,
    top_id [R, k] i32). The k largest are the first k of a STABLE descending sort — (value descending, index
    ascending), the kernel's tie rule; ``torch.topk`` leaves the order of ties unspecified. Slots past the row's
    length hold -inf / -1; a NaN entry counts as -inf."""
    x = logits.float()
    x = torch.where(x != x, torch.full_like(x, float("-inf")), x)
    V = x.shape[1]
    if rows is None:
        idx = torch.arange(x.shape[0], device=x.device)
    else:
        idx = torch.as_tensor(rows, device=x.device).long().reshape(-1)
    xs = x[idx]
    R = xs.shape[0]
    lse = torch.logsumexp(xs, -1)
    tok = torch.as_tensor(tokens, device=x.device).long()[idx]
    tok_lp = xs.gather(1, tok[:, None])[:, 0] - lse
    top_lp = torch.full((R, k), float("-inf"), dtype=torch.float32, device=x.device)
    top_id = torch.full((R, k), -1, dtype=torch.int32, device=x.device)
    n = min(k, V)
    if n and R:
        vals, ids = torch.sort(xs, dim=-1, descending=True, stable=True)
        top_lp[:, :n] = vals[:, :n] - lse[:, None]
        top_id[:, :n] = ids[:, :n].to(torch.int32)
    return tok_lp, top_lp, top_id


def rope_cos_sin(max_pos: int, head_dim: int, theta: float, scaling: dict | None = None,
                 device="cpu") -> torch.Tensor:
    """[max_pos, D] fp32 table: cos of the D/2 frequencies then sin (rotate-half / NeoX convention).

    ``scaling`` follows the HF ``rope_scaling`` dict: ``{"rope_type": "llama3", "factor", "low_freq_factor",
    "high_freq_factor", "original_max_position_embeddings"}`` or ``{"rope_type": "linear", "factor"}``.
    """
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim))
    if scaling:
        kind = scaling.get("rope_type", scaling.get("type"))
        if kind == "llama3":
            factor = scaling["factor"]
            lf, hf = scaling["low_freq_factor"], scaling["high_freq_factor"]
            old = scaling["original_max_position_embeddings"]
            low_wl, high_wl = old / lf, old / hf
            wl = 2 * math.pi / inv
            smooth = (old / wl - lf) / (hf - lf)
            scaled = torch.where(wl > low_wl, inv / factor, inv)
            mid = (wl <= low_wl) & (wl >= high_wl)
            inv = torch.where(mid, (1 - smooth) * inv / factor + smooth * inv, scaled)
        elif kind == "linear":
            inv = inv / scaling["factor"]
    t = torch.arange(max_pos, dtype=torch.float64)
    f = torch.outer(t, inv)
    return torch.cat([f.cos(), f.sin()], dim=-1).float().to(device)


def moe_route(logits: torch.Tensor, k: int, bm: int = 64):
    """fp32 reference of csrc/moe.hip moe_route: (topk_w, topk_e, perm_tok, perm_w, expert_off, tile_off)."""
    T, E = logits.shape
    p = torch.softmax(logits.float(), dim=-1)
    # descending by probability, lowest expert index first on ties (the kernel's order)
    order = torch.argsort(-p + torch.arange(E, device=p.device) * 1e-12, dim=-1, stable=True)[:, :k]
    w = torch.gather(p, 1, order)
    w = w / w.sum(-1, keepdim=True)
    te = order.to(torch.int32)
    flat = te.reshape(-1).long()
    perm = torch.argsort(flat, stable=True)
    counts = torch.bincount(flat, minlength=E)
    eo = torch.zeros(E + 1, dtype=torch.int32, device=p.device)
    eo[1:] = torch.cumsum(counts, 0)
    to = torch.zeros(E + 1, dtype=torch.int32, device=p.device)
    to[1:] = torch.cumsum((counts + bm - 1) // bm, 0)
    return w.float(), te, (perm // k).to(torch.int32), w.reshape(-1)[perm].float(), eo, to


def grouped_gemm(x, w, perm_tok, perm_w, expert_off, e_lo, gather, y, out):
    e_n = w.shape[0]
    eo = expert_off.tolist()
    for j in range(e_n):
        a, b = eo[e_lo + j], eo[e_lo + j + 1]
        if a == b:
            continue
        rows = x[perm_tok[a:b].long()] if gather else x[a:b]
        yy = rows.float() @ w[j].float().t()
        if out is not None:
            out.index_add_(0, perm_tok[a:b].long(), yy * perm_w[a:b, None])
        else:
            y[a:b] = yy.to(y.dtype)


# ---- expert-parallel all-to-all (csrc/moe.hip ep_*): CPU references of the same image layout -------------------
def _ep_meta(img: torch.Tensor, q: int, C: int) -> torch.Tensor:
    """int32 view of destination block q's metadata rows: [count, 0, 0, 0, expert of slot 0 .. C-1, ...]."""
    return img[q, C:].reshape(-1).view(torch.int32)


def ep_dispatch(x, topk_e, lo, n_own, El, C, img, slot_map):
    ep = img.shape[0]
    k = topk_e.shape[1]
    te = topk_e[lo:lo + n_own].reshape(-1).long()
    counts = [0] * ep
    for i, e in enumerate(te.tolist()):
        q = e // El
        pos = counts[q]
        counts[q] += 1
        slot_map[i] = q * img.shape[1] + pos
        _ep_meta(img, q, C)[4 + pos] = e - q * El
        img[q, pos] = x[lo + i // k]
    for q in range(ep):
        m = _ep_meta(img, q, C)
        m[0:4] = torch.tensor([counts[q], 0, 0, 0], dtype=torch.int32)
        m[4 + counts[q]:4 + C] = -1


def ep_recv_route(img, C, El, bm):
    ep, rows = img.shape[0], img.shape[1]
    ents = []  # (expert, row) of every valid slot, in (source, slot) order
    for p in range(ep):
        m = _ep_meta(img, p, C)
        n = int(m[0])
        for s in range(n):
            ents.append((int(m[4 + s]), p * rows + s))
    S = ep * C
    perm_tok = torch.zeros(S, dtype=torch.int32)
    perm_w = torch.zeros(S, dtype=torch.float32)
    eo = torch.zeros(El + 1, dtype=torch.int32)
    to = torch.zeros(El + 1, dtype=torch.int32)
    pos = 0
    for e in range(El):
        seg = [r for ex, r in ents if ex == e]
        perm_tok[pos:pos + len(seg)] = torch.tensor(seg, dtype=torch.int32)
        perm_w[pos:pos + len(seg)] = 1.0
        pos += len(seg)
        eo[e + 1] = pos
        to[e + 1] = to[e] + (len(seg) + bm - 1) // bm
    return perm_tok, perm_w, eo, to


def ep_combine(back, slot_map, topk_w, lo, n_own, out):
    k = topk_w.shape[1]
    for i in range(n_own):
        acc = torch.zeros(back.shape[-1], dtype=torch.float32)
        for j in range(k):
            acc += float(topk_w[lo + i, j]) * back[int(slot_map[i * k + j])].float()
        out[i] = acc.to(out.dtype)


# ---- JSON mode: the byte walk of engine/json_mode.py's automaton, token masks and state advance -------------------
# A state is (state id, depth, stack bits). These three functions are the definition csrc/json_mask.hip is held to,
# bit for bit: all of it is integer work, so there is no tolerance anywhere.
def json_walk(state, data: bytes):
    """The state after reading ``data`` from ``state``; (DEAD, depth, stack) as soon as a byte is rejected (depth and
    stack as they stood). DONE and DEAD accept no byte."""
    from kafka_llm_service_amd.engine import json_mode as jm

    s, d, stk = (int(v) for v in state)
    for b in data:
        if s == jm.DEAD:
            break
        e = int(jm.TRANS[s, b])
        op, nxt = e >> 6, e & 63
        if nxt == jm.DEAD:
            s = jm.DEAD
        elif op == 0:
            s = nxt
        elif op == jm.OP_OPEN:
            if d >= jm.JSON_MAX_DEPTH:
                s = jm.DEAD
            else:
                if b == 0x7B:
                    stk |= 1 << d
                d += 1
                s = nxt
        else:
            top = (stk >> (d - 1)) & 1 if d > 0 else -1
            if op == jm.OP_COMMA:
                s = jm.DEAD if top < 0 else (jm.EXPECT_KEY if top else jm.EXPECT_VALUE)
            elif top != (1 if b == 0x7D else 0):
                s = jm.DEAD
            else:
                d -= 1
                stk &= ~(1 << d)
                s = jm.DONE if d == 0 else nxt
    return s, d, stk


def json_advance_ref(state, token: int, table):
    """The row's state after ``token`` (``table``: engine/json_mode.JsonTable). In DONE every id — the EOS the mask
    allows, a forced id — leaves the state at DONE; elsewhere an id without bytes or outside the table is a rejected
    byte."""
    from kafka_llm_service_amd.engine import json_mode as jm

    s, d, stk = (int(v) for v in state)
    if s == jm.DONE:
        return s, d, stk
    token = int(token)
    if not 0 <= token < table.V or table.lens[token] == 0:
        return jm.DEAD, d, stk
    return json_walk((s, d, stk), table.bytes_of(token))


def json_mask_ref(state, table) -> np.ndarray:
    """uint32 [ceil(V / 32)]: bit i (bit ``i % 32`` of word ``i // 32``) is set iff token i is allowed in ``state`` —
    in DONE: iff it is one of the table's EOS ids; elsewhere: iff it has at least one byte and every byte is accepted
    in sequence from ``state``. All tokens are walked together, one byte position at a time."""
    from kafka_llm_service_amd.engine import json_mode as jm

    V = table.V
    s0, d0, k0 = (int(v) for v in state)
    keep = np.zeros(table.W * 32, dtype=bool)
    if s0 == jm.DONE:
        keep[table.eos_ids] = True
    elif s0 != jm.DEAD:
        s = np.full(V, s0, dtype=np.int64)
        d = np.full(V, d0, dtype=np.int64)
        stk = np.full(V, k0, dtype=np.int64)
        off = table.tok_off[:-1].astype(np.int64)
        live = np.flatnonzero(table.lens > 0)
        trans = jm.TRANS.astype(np.int64)
        for j in range(int(table.lens.max())):
            live = live[(table.lens[live] > j) & (s[live] != jm.DEAD)]
            if not live.size:
                break
            b = table.tok_bytes[off[live] + j].astype(np.int64)
            e = trans[s[live], b]
            op, nxt = e >> 6, e & 63
            dl, kl = d[live], stk[live]
            top = np.where(dl > 0, (kl >> np.maximum(dl - 1, 0)) & 1, -1)
            opening, closing, comma = op == jm.OP_OPEN, op == jm.OP_CLOSE, op == jm.OP_COMMA
            dead = (nxt == jm.DEAD) | (opening & (dl >= jm.JSON_MAX_DEPTH)) | (comma & (top < 0)) \
                | (closing & (top != (b == 0x7D)))
            nd = dl + opening - closing
            nk = np.where(opening & (b == 0x7B), kl | (1 << np.minimum(dl, 31)), kl)
            nk = np.where(closing, kl & ~(1 << np.maximum(dl - 1, 0)), nk)
            ns = np.where(comma, np.where(top == 1, jm.EXPECT_KEY, jm.EXPECT_VALUE), nxt)
            ns = np.where(closing & (nd == 0), jm.DONE, ns)
            s[live] = np.where(dead, jm.DEAD, ns)
            d[live] = np.where(dead, dl, nd)
            stk[live] = np.where(dead, kl, nk)
        keep[:V] = (table.lens > 0) & (s != jm.DEAD)
    return np.packbits(keep, bitorder="little").view("<u4")


# ---- structured outputs: the walk of a compiled schema automaton (engine/json_schema.py), token masks and advance ------
# A state is one integer: START 0, DONE 1, DEAD 0xFFFF; ``dfa`` holds ``cls`` uint8 [256] and ``trans`` uint16 [S, C].
# csrc/json_schema.hip is held to these three functions bit for bit.
def schema_walk(state: int, data: bytes, dfa) -> int:
    """The state after reading ``data`` from ``state``: ``s = trans[s, cls[b]]`` per byte, DEAD as soon as a byte is
    rejected. DONE has no outgoing edge; a state at or above S that is not DONE walks as DEAD."""
    from kafka_llm_service_amd.engine import json_schema as js

    s = int(state)
    if s >= dfa.S:
        s = js.DEAD
    for b in data:
        if s == js.DEAD:
            break
        s = int(dfa.trans[s, dfa.cls[b]])
    return s


def schema_advance_ref(state: int, token: int, dfa, table) -> int:
    """The row's state after ``token`` (``table``: engine/json_mode.JsonTable): DONE stays DONE whatever the id;
    elsewhere an id without bytes or outside the vocabulary gives DEAD."""
    from kafka_llm_service_amd.engine import json_schema as js

    s, token = int(state), int(token)
    if s == js.DONE:
        return s
    if s >= dfa.S or not 0 <= token < table.V or table.lens[token] == 0:
        return js.DEAD
    return schema_walk(s, table.bytes_of(token), dfa)


def schema_mask_ref(state: int, dfa, table) -> np.ndarray:
    """uint32 [ceil(V / 32)], the bit layout and the rules of ``json_mask_ref``: in DONE the table's EOS ids; elsewhere
    the ids with at least one byte whose bytes are all accepted in sequence from ``state``."""
    from kafka_llm_service_amd.engine import json_schema as js

    V, s0 = table.V, int(state)
    keep = np.zeros(table.W * 32, dtype=bool)
    if s0 == js.DONE:
        keep[table.eos_ids] = True
    elif s0 < dfa.S:
        s = np.full(V, s0, dtype=np.int64)
        off = table.tok_off[:-1].astype(np.int64)
        live = np.flatnonzero(table.lens > 0)
        trans, cls = dfa.trans.astype(np.int64), dfa.cls.astype(np.int64)
        for j in range(int(table.lens.max())):
            live = live[(table.lens[live] > j) & (s[live] != js.DEAD)]
            if not live.size:
                break
            s[live] = trans[s[live], cls[table.tok_bytes[off[live] + j]]]
        keep[:V] = (table.lens > 0) & (s != js.DEAD)
    return np.packbits(keep, bitorder="little").view("<u4")


# ---- automaton tool grammar: the envelope around a call body's automaton (engine/tool_automaton.py) ------------------
# A record is (state, phase, 0, table + 1); ``open`` and ``close`` are the special tokens (no bytes) that begin and end
# a call. csrc/tool_grammar.hip is held to these two functions bit for bit.
def tool_mask_ref(record, open: int, close: int, dfa, table) -> np.ndarray:
    """bool [V]: the ids a tool row may draw. FREE and TEXT: every id; OPEN: ``open``; BODY before DONE: the ids with
    bytes whose walk from the state stays alive (``schema_walk``; a state at or above S that is not DONE allows none);
    BODY in DONE, and CLOSED: ``close``."""
    from kafka_llm_service_amd.engine import json_schema as js
    from kafka_llm_service_amd.engine import tool_automaton as ta

    s, phase = int(record[0]) & 0xFFFFFFFF, int(record[1])
    V = table.V
    if not 0 <= phase < ta.TOOL_PHASES or not (0 <= open < V and 0 <= close < V):
        raise ValueError("tool_mask_ref: a phase outside 0..4, or an envelope token outside the vocabulary")
    keep = np.zeros(V, dtype=bool)
    if phase in (ta.TOOL_FREE, ta.TOOL_TEXT):
        keep[:] = True
    elif phase == ta.TOOL_OPEN:
        keep[open] = True
    elif phase == ta.TOOL_CLOSED or s == js.DONE:
        keep[close] = True
    elif s < dfa.S:
        # schema_walk over every id with bytes, in schema_mask_ref's vectorised form (s != DONE: no EOS branch there)
        bits = np.unpackbits(schema_mask_ref(s, dfa, table).view(np.uint8), bitorder="little")
        keep[:] = bits[:V].astype(bool)
    return keep


def tool_mask_words(record, open: int, close: int, dfa, table) -> np.ndarray:
    """``tool_mask_ref`` as the mask row's uint32 [ceil(V / 32)] words (bit j of word w is id 32 w + j)."""
    keep = np.zeros(table.W * 32, dtype=bool)
    keep[:table.V] = tool_mask_ref(record, open, close, dfa, table)
    return np.packbits(keep, bitorder="little").view("<u4")


def tool_advance_ref(record, token: int, open: int, close: int, dfa, table) -> np.ndarray:
    """The record after the drawn ``token`` (int32 [4]; word 3 as it was). FREE: ``open`` -> (START, BODY), else TEXT;
    OPEN: ``open`` -> (START, BODY), else DEAD; BODY before DONE: the schema walk (DEAD for an id without bytes or
    outside the vocabulary); BODY in DONE: ``close`` -> CLOSED, else DEAD; TEXT and CLOSED stay."""
    from kafka_llm_service_amd.engine import json_schema as js
    from kafka_llm_service_amd.engine import tool_automaton as ta

    s, phase, token = int(record[0]) & 0xFFFFFFFF, int(record[1]), int(token)
    if not 0 <= phase < ta.TOOL_PHASES:
        raise ValueError("tool_advance_ref: a phase outside 0..4")
    if phase == ta.TOOL_FREE:
        s, phase = (js.START, ta.TOOL_BODY) if token == open else (s, ta.TOOL_TEXT)
    elif phase == ta.TOOL_OPEN:
        s, phase = (js.START, ta.TOOL_BODY) if token == open else (js.DEAD, phase)
    elif phase == ta.TOOL_BODY:
        if s == js.DONE:
            s, phase = (s, ta.TOOL_CLOSED) if token == close else (js.DEAD, phase)
        elif s >= dfa.S or not 0 <= token < table.V or table.lens[token] == 0:
            s = js.DEAD
        else:
            s = schema_walk(s, table.bytes_of(token), dfa)
    return np.array([s, phase, int(record[2]), int(record[3])], dtype=np.int64).astype(np.int32)
