"""Tile attention v3 (ops/csrc/attn_tile.h) on fp8 KV pages, against the key-exact constructions and bounds of
test_attn_keys_gpu.py (dequantised e4m3 * 2^e is exact in bf16, so the bounds are the bf16 kernel's). The census
signatures' amax differs from token to token, so a V exponent paired with the wrong key moves a sum; the needle
worlds' 1x and 1.5x keys have different K exponents, so a wrong key exponent moves the winner."""
import pytest
import torch

from kafka_llm_service_amd import ops

import test_attn_keys_gpu as keys
from test_attn_keys_gpu import BIG, CPU, D, HEADS, SCALE, census_check


def needle_check(out, ref_out, vp, what=""):
    """keys.needle_check with its bf16 ulp taken of the whole output, V[p] + leak, not of V[p] alone:
    |out - V[p]| <= 2^-8 |V[p]| + (1 + 2^-8) leak. An e4m3 V[p] has exact zeros; there the unmended bound is the leak
    itself, which a bf16 output cannot meet once the leak rounds away from zero (measured on the 32/8 parity-1 world,
    token 63, d 22, V[p] = -0.0: reference -3.7163e-11, kernel -3.7289e-11 = the next bf16 value, 4 of 4608 probes).
    The leak is <= 1e-3, so the bound moves by < 4e-6."""
    ref_out, vp = ref_out.double(), vp.double()
    keys.needle_check(out, vp + (ref_out - vp) * (1 + 2.0 ** -8), vp, what)


@pytest.mark.gpu
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_census_prefill_fp8_tile(cuda, Hq, Hkv):
    """Unaligned key chunks (0,45) (45,300) (300,BIG), causal limits per token, fp32 partials + lse."""
    keys._census_prefill(cuda, Hq, Hkv, True, 3)


@pytest.mark.gpu
def test_census_staged_pages_limit_fp8_tile(cuda):
    keys.test_census_prefill_staged_pages_limit(cuda, 3, True)


@pytest.mark.gpu
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_needle_prefill_causal_fp8_tile(cuda, Hq, Hkv):
    """The final-bf16 ``out`` path, both parities."""
    for flip in (0, 1):
        w = keys._prefill_needle_world(Hkv, True, flip)
        q, vp = keys._prefill_probes(w, Hq)
        o_ref = keys._prefill_needle_run(w, q, CPU, 3, torch.float32)
        out = keys._prefill_needle_run(w, q, cuda, 3, torch.bfloat16)
        needle_check(out, o_ref, vp, f"prefill needle fp8 tile parity {flip}")


@pytest.mark.gpu
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_needle_decode_bf16_prefix_partials_fp8_tile(cuda, Hq, Hkv):
    """bf16 prefix partials (sc1 stores) written by the fp8 tile kernel, folded by the fp8 decode kernel's fused merge;
    three launches."""
    w = keys._decode_needle_world(Hkv, True)
    for launch in range(3):
        q, vp = keys._decode_probes(w, Hq, launch)
        o_ref = keys._decode_needle_run(w, q, CPU, True, 3, torch.float32)
        out = keys._decode_needle_run(w, q, cuda, True, 3, torch.bfloat16)
        needle_check(out, o_ref, vp, f"decode needle bf16-pre fp8 tile launch {launch}")


# Alt partials: sequences 0..2 of the census world are plain items (fp32 out_part, row = token), sequence 3 (40 tokens
# on 700 keys of context; at G = 8 two tiles of 32 and 8 tokens) is flagged alt and writes alt_part / alt_lse at row
# token - ALT_OFF. Key ranges (0, 45) and (45, BIG): a range edge inside the first 64-key tile, keys on both sides of it.
ALT_RANGES = [(0, 45), (45, BIG)]
ALT_OFF = sum(keys.NEW[:3])


def _alt_census(dev, Hq, Hkv):
    w = keys._census_world(tuple(c + n for c, n in zip(keys.CTX, keys.NEW)), Hkv, True, seed=3)
    items, lim, entries = keys._prefill_items(Hq // Hkv, 3, ALT_RANGES)
    items[items[:, 0] >= ALT_OFF, 6] = 1
    T, S = sum(keys.NEW), len(ALT_RANGES)
    q = torch.zeros(T, Hq, D, dtype=torch.bfloat16, device=dev)
    part = torch.full((ALT_OFF, Hq, S, D), float("nan"), device=dev)
    lse = torch.full((ALT_OFF, Hq, S), float("nan"), device=dev)
    apart = torch.full((T - ALT_OFF, Hq, S, D), float("nan"), device=dev)
    alse = torch.full((T - ALT_OFF, Hq, S), float("nan"), device=dev)
    ops.attn_prefill(items.to(dev), q, w.k.to(dev), w.v.to(dev), w.bt.to(dev), lim.to(dev), SCALE, out_part=part,
                     lse_part=lse, variant=3, alt_part=apart, alt_lse=alse, alt_tok_off=ALT_OFF)
    census_check(w, part, lse, [e for e in entries if e[0] < ALT_OFF], "fp8 tile, plain items")
    census_check(w, apart, alse, [(e[0] - ALT_OFF,) + e[1:] for e in entries if e[0] >= ALT_OFF], "fp8 tile, alt items")


@pytest.mark.gpu
def test_census_alt_partials_fp8_tile(cuda):
    _alt_census(cuda, 8, 1)


def test_fp8_tile_constructions_pass_on_the_reference():
    """Every construction above holds on the reference (the CPU path of ``ops``), and the new needle cases meet the
    leak condition their tolerance rests on."""
    keys._census_prefill(CPU, 8, 1, True, 3)
    keys._census_prefill(CPU, 4, 2, True, 3)
    _alt_census(CPU, 8, 2)
    for Hq, Hkv in HEADS:
        w = keys._decode_needle_world(Hkv, True)
        cases = [(keys._decode_probes(w, Hq, n), lambda q: keys._decode_needle_run(w, q, CPU, True, 3, torch.float32))
                 for n in range(3)]
        for wp in (keys._prefill_needle_world(Hkv, True, flip) for flip in (0, 1)):
            cases.append((keys._prefill_probes(wp, Hq),
                          lambda q, wp=wp: keys._prefill_needle_run(wp, q, CPU, 3, torch.float32)))
        for (q, vp), run in cases:
            o_ref = run(q)
            assert (o_ref - vp).abs().amax().item() <= 1e-3, f"{Hq}/{Hkv}: reference leak"
            needle_check(o_ref, o_ref, vp)
