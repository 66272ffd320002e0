"""``min_p`` inside the sampler kernel (ops/csrc/sampling.hip) against ``ops.reference.sample_replay``, token for
token: a min_p row with top-k / top-p adds one test to the rejection loop's candidates; a row with min_p alone stays on
the split path (sample_min_p_split: slice maximum, slice draw, and in the last workgroup the row threshold, with a
rescan of a slice whose winner fell below it). Every row the replay does not flag ``ambiguous`` has exactly one right
token; the threshold itself adds no ambiguity (one fp32 add of the host's logarithm, compared in fp32 on both sides).
The logits follow the sampler suite's recipe (randn * 3 clamped to +-14, T in {0.9, 1.3}); penalties and biases are
multiples of 1/8, so the processed bf16 rows are exact in fp32 with or without an fma."""
import math

import numpy as np
import pytest
import torch
from test_min_p import min_p_proc, staircase_rows

from kafka_llm_service_amd import ops
from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
from kafka_llm_service_amd.engine.logits_proc import LogitsProcessor
from kafka_llm_service_amd.engine.sequence import SamplingParams, Sequence
from kafka_llm_service_amd.ops import reference as ref

AMBIGUOUS_CAP = 0.02  # of a test's rows (the sampler suite's cap); asserted on the replay before the kernel runs
# (name, min_p, top_p, top_k, greedy)
MODES = (("min_p 0.05", 0.05, 1.0, 0, False), ("min_p 0.3", 0.3, 1.0, 0, False), ("min_p 1.0", 1.0, 1.0, 0, False),
         ("min_p 0.1 top_p 0.9", 0.1, 0.9, 0, False), ("min_p 0.1 top_k 40", 0.1, 1.0, 40, False),
         ("greedy min_p 0.3", 0.3, 1.0, 0, True))


def _capped(rep, what):
    B = rep.tokens.numel()
    msg = (f"{what}: rows {B}, ambiguous {int(rep.ambiguous.sum())}, max rounds {int(rep.rounds.max())}, "
           f"fallback rows {int(rep.fell_back.sum())}, rescanning rows {int((rep.rescans > 0).sum())}")
    assert int(rep.ambiguous.sum()) <= AMBIGUOUS_CAP * B, msg
    return msg


def _same(tok, rep, msg):
    tok = tok.cpu()
    bad = torch.nonzero((tok != rep.tokens) & ~rep.ambiguous).flatten().tolist()
    assert not bad, f"{msg}; rows {bad[:8]} differ: kernel {tok[bad[:8]].tolist()} replay {rep.tokens[bad[:8]].tolist()}"
    print(msg)


def _ws(dev, B, nsplit):
    return torch.zeros(65536 + 2 * B * nsplit, dtype=torch.int32, device=dev)


def _logits(B, V, seed, dtype):
    return (torch.randn(B, V, generator=torch.Generator().manual_seed(seed)) * 3).clamp(-14, 14).to(dtype)


def _temps(B):
    return torch.tensor([0.9, 1.3] * ((B + 1) // 2))[:B]


def _tables(dev, V, rows, B, **kw):
    lp = LogitsProcessor(dev, V, **kw)
    proc, upd = lp.build(rows, B)
    up = torch.from_numpy if str(dev) == "cpu" else (lambda a: torch.from_numpy(a).to(dev))
    lp.apply(upd, up)
    return lp, torch.from_numpy(proc).to(dev)


def _threshold(xp: torch.Tensor, temp: torch.Tensor, min_p: float) -> tuple[np.ndarray, np.ndarray]:
    """(xv, thr) of processed fp32 rows as the kernel forms them: xv = x * (1 / T), thr = max + float32(ln min_p)."""
    xv = xp.numpy() * (np.float32(1) / temp.numpy().astype(np.float32))[:, None]
    return xv, xv.max(1) + np.float32(math.log(min_p))


# ---- ragged and small vocabularies ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("V", [9, 40, 1031, 16389])
def test_min_p_ragged_vocab_matches_replay(cuda, V):
    """B = 60 rows, bf16 and fp32 with a padded stride whose padding holds the largest finite value (a read past V
    would be the maximum and move the threshold), one workgroup and 8 splits; min_p alone, with top_p, with top_k, and
    on greedy rows, which ignore it."""
    from kafka_llm_service_amd.ops._ext import ext

    B = 60
    step = torch.tensor([3], dtype=torch.long)
    seeds = torch.arange(B, dtype=torch.long) * 13 + 1
    for dtype in (torch.bfloat16, torch.float32):
        x = _logits(B, V, 31 + V, dtype)
        buf = torch.full((B, (V + 7) // 8 * 8 + 8), torch.finfo(dtype).max, dtype=dtype, device=cuda)
        buf[:, :V] = x.to(cuda)
        xg = buf[:, :V]
        for name, mp, p, k, greedy in MODES:
            temp = torch.zeros(B) if greedy else _temps(B)
            tp = torch.full((B,), p) if p < 1 else None
            tk = torch.full((B,), k, dtype=torch.int32) if k else None
            rows = [(i, Sequence(f"r{i}", [1], SamplingParams(min_p=mp)), None) for i in range(B)]
            lp_c, pd_c = _tables("cpu", V, rows, B, max_slots=8, mask_rows=2, bias_rows=2)
            rep = ref.sample_replay(x, temp, tp, tk, seeds, step, proc=pd_c, mask_tab=lp_c.tables()[0], nsplit=8)
            msg = _capped(rep, f"V {V} {dtype} {name}")
            xv, thr = _threshold(x.float(), torch.ones(B) if greedy else temp, mp)
            if greedy:
                assert torch.equal(rep.tokens, x.float().argmax(-1)) and not bool(rep.ambiguous.any())
            else:
                assert bool(rep.plain.all()) == (tp is None and not (k and k < V))
                assert (xv[np.arange(B), rep.tokens.numpy()] >= thr).all()
                # (the draws are not decided: some rows take another token than the maximum)
                assert mp == 1.0 or int((rep.tokens != x.float().argmax(-1)).sum()) >= B // 10, msg
            lp, proc = _tables(cuda, V, rows, B, max_slots=8, mask_rows=2, bias_rows=2)
            for nsplit in (1, 8):
                out = torch.full((B,), -1, dtype=torch.long, device=cuda)
                ext().sample(xg, temp.to(cuda), None if tp is None else tp.to(cuda), None if tk is None else tk.to(cuda),
                             seeds.to(cuda), step.to(cuda), out, _ws(cuda, B, nsplit), nsplit, proc, lp.tables()[0],
                             None, lp.bias_table())
                _same(out, rep, f"{msg}, nsplit {nsplit}")
                if not greedy:  # ambiguous rows included: the threshold is exact
                    assert (xv[np.arange(B), out.cpu().numpy()] >= thr).all(), msg


# ---- the rescan branch ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_min_p_staircase_rescan_matches_replay(cuda):
    """Rows whose slice winners fall below the row threshold (test_min_p.staircase_rows): at 8 and at 3 splits the last
    workgroup rescans a slice in at least half the rows — asserted on the replay before the kernel runs — and the
    kernel returns the replay's token at 1, 3 and 8 splits, never one below the threshold."""
    from kafka_llm_service_amd.ops._ext import ext

    x, temp = staircase_rows()
    B, V = x.shape
    seeds = torch.arange(B, dtype=torch.long) * 13 + 1
    step = torch.tensor([2], dtype=torch.long)
    proc = min_p_proc(B, 0.05)
    reps = {}
    for ns in (1, 3, 8):
        reps[ns] = ref.sample_replay(x, temp, seeds=seeds, step=step, proc=proc, nsplit=ns)
        msg = _capped(reps[ns], f"staircase nsplit {ns}")
        assert ns == 1 or int((reps[ns].rescans > 0).sum()) >= B // 2, msg
        assert torch.equal(reps[ns].tokens, reps[1].tokens)
    xv, thr = _threshold(x, temp, 0.05)
    buf = torch.zeros(B, (V + 7) // 8 * 8, device=cuda)  # (the kernel wants a row stride of 8 k)
    buf[:, :V] = x.to(cuda)
    mt = torch.zeros(1, (V + 31) // 32, dtype=torch.int32, device=cuda)
    for ns in (1, 3, 8):
        for launch in range(2):  # (twice: the tickets re-arm)
            out = torch.full((B,), -1, dtype=torch.long, device=cuda)
            ext().sample(buf[:, :V], temp.to(cuda), None, None, seeds.to(cuda), step.to(cuda), out, _ws(cuda, B, ns), ns,
                         proc.to(cuda), mt, None, None)
            _same(out, reps[ns], f"staircase nsplit {ns} launch {launch}")
            assert (xv[np.arange(B), out.cpu().numpy()] >= thr).all()


# ---- combined with the other processing -------------------------------------------------------------------------------
def processed_case():
    """32 rows of 16,389 bf16 logits, min_p = 0.05 in all of them; the kind of a row is i % 4: 0 a grammar mask that
    removes the raw maximum (the threshold follows the masked maximum), 1 presence / frequency penalties, 2 a +100
    logit_bias (its token is then the maximum and the only one kept), 3 a forced token. Rows 16.. add top_p = 0.9."""
    B, V = 32, 16389
    x = _logits(B, V, 41, torch.bfloat16)
    g = torch.Generator().manual_seed(3)
    rows, top, biased = [], x.float().argmax(-1).tolist(), {}
    for i in range(B):
        kind = i % 4
        kw, spec = dict(min_p=0.05), None
        if kind == 0:
            peak = set(torch.nonzero(x[i] == x[i].max()).flatten().tolist())  # (a bf16 maximum may occur twice)
            spec = [t for t in range(V) if t not in peak and t % 3 != i % 3]
        elif kind == 1:
            kw.update(presence_penalty=0.5, frequency_penalty=1.5)
        elif kind == 2:
            biased[i] = int(torch.randint(0, V, (1,), generator=g))
            kw.update(logit_bias={biased[i]: 100.0})
        else:
            spec = [int(torch.randint(0, V, (1,), generator=g))]
        rows.append((i, Sequence(f"p{i}", [1], SamplingParams(**kw)), spec))
    topp = torch.tensor([1.0] * 16 + [0.9] * 16)
    return x, rows, top, biased, topp


@pytest.mark.gpu
def test_min_p_with_mask_penalties_bias_and_forced_rows(cuda):
    """Three successive steps with the count table carried along (the second and third see penalties): tokens and
    counts equal the replay's after each, and every penalised row's counts grew by exactly one per step."""
    x, rows, top, biased, topp = processed_case()
    B, V = x.shape
    lp_c, pd_c = _tables("cpu", V, rows, B, max_slots=16, mask_rows=16, bias_rows=16)
    lp_g, pd_g = _tables(cuda, V, rows, B, max_slots=16, mask_rows=16, bias_rows=16)
    assert torch.equal(pd_c, pd_g.cpu()) and (pd_c[:, 7] == int(np.float32(math.log(0.05)).view(np.int32))).all()
    (mt_c, cnt_c), (mt_g, cnt_g) = lp_c.tables(), lp_g.tables()
    temp = _temps(B)
    seeds = torch.arange(B, dtype=torch.long) * 13 + 1
    buf = torch.full((B, (V + 7) // 8 * 8), torch.finfo(x.dtype).max, dtype=x.dtype, device=cuda)
    buf[:, :V] = x.to(cuda)  # (the kernel wants a row stride of 8 k; the padding would be the maximum if it were read)
    xg = buf[:, :V]
    for stepv in range(3):
        step = torch.tensor([stepv], dtype=torch.long)
        xp, _ = ref.process_logits(x, pd_c, mt_c, cnt_c, lp_c.bias_table())  # (before the replay bumps the counts)
        rep = ref.sample_replay(x, temp, topp, None, seeds, step, proc=pd_c, mask_tab=mt_c, counts=cnt_c, nsplit=8,
                                bias_tab=lp_c.bias_table())
        msg = _capped(rep, f"processed step {stepv}")
        assert not bool(rep.ambiguous.any()), msg  # the count tables can only be compared when no row may differ
        assert torch.equal(rep.plain, torch.tensor([i < 16 and i % 4 != 3 for i in range(B)]))
        tok = ops.sample(xg, temp.to(cuda), topp.to(cuda), None, seeds.to(cuda), step.to(cuda), proc=pd_g,
                         mask_tab=mt_g, counts=cnt_g, bias_tab=lp_g.bias_table())
        _same(tok, rep, msg)
        tok = tok.cpu()
        assert torch.equal(cnt_g.cpu(), cnt_c), f"counts after {msg}"
        assert int(cnt_c.sum()) == (stepv + 1) * (B // 4), msg  # one bump per penalised row and step
        assert torch.equal(tok[3::4], pd_c[3::4, 1].long())  # forced rows: untouched
        assert all(int(tok[i]) == t for i, t in biased.items())  # the +100 token is the maximum: kept alone
        xv, thr = _threshold(xp, temp, 0.05)
        free = [i for i in range(B) if i % 4 != 3]
        assert (xv[free, tok[free].numpy()] >= thr[free]).all()
        for i in range(0, B, 4):  # the masked rows: never the raw maximum, and a threshold below the raw one
            assert int(tok[i]) != top[i] and int(tok[i]) % 3 != i % 3
            assert thr[i] < float(x[i, top[i]]) * float(np.float32(1) / np.float32(temp[i])) + np.float32(math.log(0.05))
    assert int(cnt_c.max()) >= 1


# ---- the full vocabulary ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_min_p_full_vocab_matches_replay(cuda):
    B, V = 64, 128256
    x = _logits(B, V, 31, torch.bfloat16)
    temp = torch.full((B,), 0.7)
    seeds = torch.arange(B, dtype=torch.long) * 1000003 - 17
    proc = min_p_proc(B, 0.05)
    mt = torch.zeros(1, (V + 31) // 32, dtype=torch.int32, device=cuda)
    xg, pg = x.to(cuda), proc.to(cuda)
    xv, thr = _threshold(x.float(), temp, 0.05)
    for stepv in (0, 5):
        step = torch.tensor([stepv], dtype=torch.long)
        rep = ref.sample_replay(x, temp, seeds=seeds, step=step, proc=proc, nsplit=8)
        msg = _capped(rep, f"full vocabulary step {stepv}")
        assert bool(rep.plain.all()) and len(set(rep.tokens.tolist())) > B // 2
        tok = ops.sample(xg, temp.to(cuda), seeds=seeds.to(cuda), step=step.to(cuda), proc=pg, mask_tab=mt)
        _same(tok, rep, msg)
        assert (xv[np.arange(B), tok.cpu().numpy()] >= thr).all()


# ---- rows without min_p in the same batch -----------------------------------------------------------------------------
@pytest.mark.gpu
def test_rows_without_min_p_are_unchanged(cuda):
    """Greedy, plain-temperature and top_p rows next to min_p rows: they give the tokens they give when the min_p rows
    are plain rows (proc[7] = 0)."""
    B, V = 32, 128256
    x = _logits(B, V, 37, torch.bfloat16).to(cuda)
    temp = torch.tensor([0.0, 0.9, 1.3, 0.9] * (B // 4))
    topp = torch.tensor([1.0, 1.0, 1.0, 0.9] * (B // 4))
    seeds = torch.arange(B, dtype=torch.long) * 13 + 1
    step = torch.tensor([4], dtype=torch.long)
    with_mp = min_p_proc(B, [0.05 if (i // 4) % 2 else 0.0 for i in range(B)])
    mt = torch.zeros(1, (V + 31) // 32, dtype=torch.int32, device=cuda)
    args = (x, temp.to(cuda), topp.to(cuda), None, seeds.to(cuda), step.to(cuda))
    a = ops.sample(*args, proc=with_mp.to(cuda), mask_tab=mt).cpu()
    b = ops.sample(*args, proc=min_p_proc(B, 0.0).to(cuda), mask_tab=mt).cpu()
    old = with_mp[:, 7] == 0
    assert int(old.sum()) == B // 2 and torch.equal(a[old], b[old])
    stoch = ~old & (temp > 0)
    assert int((a[stoch] != b[stoch]).sum()) >= 1  # (min_p did cut somewhere: the batches are not the same launch)
    assert torch.equal(a[~old & (temp == 0)], b[~old & (temp == 0)])  # greedy rows ignore it


# ---- engine -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_engine_min_p_one_is_greedy_eager_and_graphed(cuda):
    """min_p = 1 keeps the maximum alone, so the row is the greedy row — unless the maximum occurs twice, which bf16
    logits over 128k entries do now and then (greedy takes the first, min_p = 1 draws among the equals). The prompt
    is therefore the first of a fixed list whose greedy run has a unique maximum at all 16 steps."""
    cfg = dict(model="tiny-llama", device="cuda:0", num_kv_blocks=512, max_model_len=2048)
    kw = dict(max_tokens=16, ignore_eos=True)
    sps = [SamplingParams(temperature=1.5, seed=5, min_p=1.0, **kw), SamplingParams(temperature=1.5, seed=6, **kw)]
    eager = model = None
    for pseed in range(21, 33):
        g = torch.Generator().manual_seed(pseed)
        prompts = [torch.randint(0, 5000, (n,), generator=g).tolist() for n in (17, 23)]
        eager = LLMEngine(EngineConfig(**cfg), model=model)
        model = eager.model
        eager.runner.fixed_decode_items = True  # the graph engine's decode split, so both sum in the same order
        margins, orig = [], eager.runner.sample_device

        def spy(logits, sp, margins=margins, orig=orig):
            top = logits[0].float().topk(2).values
            margins.append(float(top[0] - top[1]))
            return orig(logits, sp)

        eager.runner.sample_device = spy
        # (the same batch: the greedy row next to the same unconstrained one)
        greedy = eager.generate(prompts, [SamplingParams(temperature=0.0, **kw), sps[1]])[0]
        eager.runner.sample_device = orig
        print(f"prompt seed {pseed}: smallest top-1 / top-2 margin of the greedy row {min(margins)}")
        if min(margins) > 0:
            break
    else:
        pytest.fail("no prompt of the list has a tie-free greedy run")
    outs = LLMEngine(EngineConfig(**cfg), model=eager.model)
    outs.runner.fixed_decode_items = True
    got = outs.generate(prompts, sps)
    assert got[0] == greedy and len(greedy) == 16 and got[1] != got[0]
    graphed = LLMEngine(EngineConfig(**cfg, use_graphs=True), model=eager.model)
    got_g = graphed.generate(prompts, sps)
    st = graphed.runner.graphs.stats
    assert not graphed.runner.graphs.disabled, "hipGraph capture failed (see log)"
    assert st["replays"] > 0 and got_g[0] == greedy and got_g == got
