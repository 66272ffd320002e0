"""``repetition_penalty`` inside the sampler kernel (ops/csrc/sampling.hip) against ``ops.reference.sample_replay``,
token for token on every row the replay does not flag ``ambiguous``: the replay runs on the CPU first, the ambiguity
cap is asserted on it, then the kernel runs. A seen token (a non-zero word of the row's count-table slot: the prompt
flag COUNT_SEEN_PROMPT, a generated count, or both) has its logit multiplied by 1 / r if positive and by r otherwise,
one fp32 multiply rounded on its own, before the additive penalties, the bias and the mask. With r in {2, 0.5} every
product of a bf16 logit is exact; with r = 1.3 the kernel's ``__fmul_rn`` and the replay's fp32 product are the same
rounding, so the comparison stays exact there too."""
import numpy as np
import pytest
import torch
from test_min_p_gpu import _capped, _logits, _same, _tables, _temps, _ws
from test_numerics_gpu import K_STD, RATIO
from test_repetition_penalty import FLAG, hand_loop, penalise

from kafka_llm_service_amd import ops
from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
from kafka_llm_service_amd.engine.logits_proc import rep_factors
from kafka_llm_service_amd.engine.sequence import SamplingParams, Sequence
from kafka_llm_service_amd.models.oracle import dense_logits
from kafka_llm_service_amd.ops import reference as ref

# (name, top_p, top_k, min_p, greedy)
MODES = (("greedy", 1.0, 0, 0.0, True), ("temperature", 1.0, 0, 0.0, False), ("top_p 0.9", 0.9, 0, 0.0, False),
         ("top_k 40", 1.0, 40, 0.0, False), ("min_p 0.1", 1.0, 0, 0.1, False))


def seen_tables(B, V, r, seed):
    """One slot per row: a random third of the vocabulary is seen — half of it as prompt flags, half as generated
    counts 1..3 — and every slot's factor is r. -> (proc [B, 8], counts [B, cnt_ld], rep_tab [B, 2], seen bool [B, V])."""
    g = torch.Generator().manual_seed(seed)
    counts = torch.zeros(B, (V + 7) // 8 * 8, dtype=torch.int32)
    n = max(2, V // 3)
    for b in range(B):
        ids = torch.randperm(V, generator=g)[:n]
        counts[b, ids[:n // 2]] = FLAG
        counts[b, ids[n // 2:]] = torch.randint(1, 4, (n - n // 2,), generator=g).int()
    proc = torch.zeros(B, 8, dtype=torch.int32)
    proc[:, 2] = torch.arange(B, dtype=torch.int32)
    rep_tab = torch.from_numpy(rep_factors(r))[None].repeat(B, 1).contiguous()
    return proc, counts, rep_tab, counts[:, :V] != 0


def ragged_case(cuda, V, dtype, r, seed):
    """B = 60 rows in a padded-stride buffer whose padding holds the dtype's maximum (a read past V would win); every
    mode at one workgroup and at 8 splits against the replay; the emitted token's count grows by one, flags stay."""
    from kafka_llm_service_amd.engine.logits_proc import min_p_bits
    from kafka_llm_service_amd.ops._ext import ext

    B = 60
    step = torch.tensor([3], dtype=torch.long)
    seeds = torch.arange(B, dtype=torch.long) * 13 + 1
    x = _logits(B, V, seed, dtype)
    buf = torch.full((B, (V + 7) // 8 * 8 + 8), torch.finfo(dtype).max, dtype=dtype, device=cuda)
    buf[:, :V] = x.to(cuda)
    xg = buf[:, :V]
    proc, counts, rep_tab, seen = seen_tables(B, V, r, seed + 1)
    mt = torch.zeros(1, (V + 31) // 32, dtype=torch.int32)
    y = penalise(x.float().numpy(), seen.numpy(), r)
    assert (y != x.float().numpy()).sum() >= B * (V // 3) * 0.9  # (the seen logits do change; zeros are rare)
    rep_g, mt_g = rep_tab.to(cuda), mt.to(cuda)
    for name, p, k, mp, greedy in MODES:
        temp = torch.zeros(B) if greedy else _temps(B)
        tp = torch.full((B,), p) if p < 1 else None
        tk = torch.full((B,), k, dtype=torch.int32) if k else None
        pr = proc.clone()
        pr[:, 7] = min_p_bits(mp)
        cnt_c = counts.clone()
        rep = ref.sample_replay(x, temp, tp, tk, seeds, step, proc=pr, mask_tab=mt, counts=cnt_c, nsplit=8,
                                rep_tab=rep_tab)
        msg = _capped(rep, f"V {V} {dtype} r {r} {name}")
        off = ref.sample_replay(x, temp, tp, tk, seeds, step, proc=pr, mask_tab=mt, counts=counts.clone(), nsplit=8)
        if V >= 40:  # the penalty decides some rows: the replay without the table draws other tokens
            assert int((off.tokens != rep.tokens).sum()) >= (B // 10 if r in (2.0, 0.5) else 1), msg
        if greedy:
            assert torch.equal(rep.tokens, torch.from_numpy(y.argmax(-1))) and not bool(rep.ambiguous.any())
        for nsplit in (1, 8):
            out = torch.full((B,), -1, dtype=torch.long, device=cuda)
            cnt_g = counts.clone().to(cuda)
            ext().sample(xg, temp.to(cuda), None if tp is None else tp.to(cuda), None if tk is None else tk.to(cuda),
                         seeds.to(cuda), step.to(cuda), out, _ws(cuda, B, nsplit), nsplit, pr.to(cuda), mt_g, cnt_g,
                         None, rep_g)
            _same(out, rep, f"{msg}, nsplit {nsplit}")
            want = counts.clone()
            want[torch.arange(B), out.cpu()] += 1
            assert torch.equal(cnt_g.cpu(), want), msg
            if not bool(rep.ambiguous.any()):
                assert torch.equal(want, cnt_c)


# ---- 1. ragged vocabularies, exact factors ----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("r", [2.0, 0.5])
@pytest.mark.parametrize("V", [9, 40, 1031, 16389])
def test_ragged_vocab_matches_replay(cuda, V, r):
    for dtype in (torch.bfloat16, torch.float32):
        ragged_case(cuda, V, dtype, r, 31 + V)


# ---- 2. a general factor ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("V", [1031, 16389])
def test_general_factor_matches_replay(cuda, V):
    """r = 1.3: the products round. The kernel forms each in one fp32 multiply (``__fmul_rn``: no fma with the
    subtraction behind it), as the replay does."""
    for dtype in (torch.bfloat16, torch.float32):
        ragged_case(cuda, V, dtype, 1.3, 57 + V)


# ---- 3. combined with everything --------------------------------------------------------------------------------------
def combined_rows(V, B, g, with_rep):
    """Kind of row i is i % 8: 0 repetition + presence / frequency, 1 repetition + logit_bias, 2 repetition under a
    grammar mask, 3 a forced row (with the penalty, which it ignores), 4 untouched, 5 presence / frequency alone, 6
    repetition alone, 7 frequency alone under a mask. ``with_rep`` False: the same batch without the feature."""
    rows = []
    for i in range(B):
        kind = i % 8
        prompt = torch.randint(0, V, (V // 6,), generator=g).tolist()
        bias_tok, forced, rest = (int(torch.randint(0, V, (1,), generator=g)) for _ in range(3))
        kw, spec = {}, None
        if kind in (0, 1, 2, 3, 6) and with_rep:
            kw["repetition_penalty"] = 2.0 if i % 16 < 8 else 0.5
        if kind == 0:
            kw.update(presence_penalty=0.5, frequency_penalty=1.5)
        elif kind == 1:
            kw.update(logit_bias={bias_tok: 2.5, prompt[0]: -1.25})
        elif kind in (2, 7):
            spec = [t for t in range(V) if t % 3 != rest % 3]
            if kind == 7:
                kw.update(frequency_penalty=0.75)
        elif kind == 3:
            spec = [forced]
        elif kind == 5:
            kw.update(presence_penalty=0.25, frequency_penalty=0.5)
        if kind != 4:
            rows.append((i, Sequence(f"c{i}", prompt, SamplingParams(**kw)), spec))
    return rows


@pytest.mark.gpu
def test_combined_with_penalties_bias_mask_and_forced_rows(cuda):
    """Three successive steps with the tables carried along (steps two and three see generated counts beside the
    prompt flags): tokens and count tables equal the replay's, each slotted row's word at its token grew by one and no
    flag moved; the rows without repetition give the tokens of a batch in which no row has the feature."""
    B, V = 32, 16389
    x = _logits(B, V, 43, torch.bfloat16)
    rows = combined_rows(V, B, torch.Generator().manual_seed(5), True)
    plain_rows = combined_rows(V, B, torch.Generator().manual_seed(5), False)
    kw = dict(max_slots=32, mask_rows=16, bias_rows=16)
    lp_c, pd_c = _tables("cpu", V, rows, B, **kw)
    lp_g, pd_g = _tables(cuda, V, rows, B, **kw)
    lp_p, pd_p = _tables(cuda, V, plain_rows, B, **kw)
    assert torch.equal(pd_c, pd_g.cpu()) and pd_c.shape == (B, 8)
    (mt_c, cnt_c), (mt_g, cnt_g), (mt_p, cnt_p) = lp_c.tables(), lp_g.tables(), lp_p.tables()
    assert torch.equal(cnt_c, cnt_g.cpu()) and torch.equal(lp_c.rep_table(), lp_g.rep_table().cpu())
    flags = cnt_c & FLAG
    rep_rows = [i for i, s, _ in rows if s.params.repetition_penalty != 1]
    assert len(rep_rows) == 20 and int((flags != 0).sum()) > 20 * (V // 8) and not bool((cnt_p.cpu() & FLAG).any())
    assert set(lp_c.rep_table()[pd_c[rep_rows, 2].long(), 0].tolist()) == {2.0, 0.5}
    old = [i for i in range(B) if i not in rep_rows]  # untouched rows and penalty rows without repetition
    temp = _temps(B)
    temp[::16] = 0.0  # (two greedy repetition rows)
    topp = torch.tensor([1.0] * 16 + [0.9] * 16)
    seeds = torch.arange(B, dtype=torch.long) * 13 + 1
    buf = torch.full((B, (V + 7) // 8 * 8), torch.finfo(x.dtype).max, dtype=x.dtype, device=cuda)
    buf[:, :V] = x.to(cuda)
    xg = buf[:, :V]
    slots = pd_c[:, 2].long()
    slotted = torch.nonzero(slots >= 0).flatten()
    changed = 0
    for stepv in range(3):
        step = torch.tensor([stepv], dtype=torch.long)
        before = cnt_c.clone()
        xp, _ = ref.process_logits(x, pd_c, mt_c, cnt_c, lp_c.bias_table(), lp_c.rep_table())
        x0, _ = ref.process_logits(x, pd_c, mt_c, cnt_c, lp_c.bias_table())
        changed += int((xp[rep_rows] != x0[rep_rows]).sum())
        rep = ref.sample_replay(x, temp, topp, None, seeds, step, proc=pd_c, mask_tab=mt_c, counts=cnt_c, nsplit=8,
                                bias_tab=lp_c.bias_table(), rep_tab=lp_c.rep_table())
        msg = _capped(rep, f"combined step {stepv}")
        assert not bool(rep.ambiguous.any()), msg  # the count tables can only be compared when no row may differ
        tok = ops.sample(xg, temp.to(cuda), topp.to(cuda), None, seeds.to(cuda), step.to(cuda), proc=pd_g,
                         mask_tab=mt_g, counts=cnt_g, bias_tab=lp_g.bias_table(), rep_tab=lp_g.rep_table())
        _same(tok, rep, msg)
        tok = tok.cpu()
        assert torch.equal(cnt_g.cpu(), cnt_c), f"counts after {msg}"
        grew = cnt_c - before
        want = torch.zeros_like(grew)
        want[slots[slotted], tok[slotted]] = 1
        assert torch.equal(grew, want) and torch.equal(cnt_c & FLAG, flags), msg  # one bump per slotted row, flags stay
        assert torch.equal(tok[3::8], pd_c[3::8, 1].long())  # forced rows: their token, whatever the penalty
        for i, _, spec in rows:  # masked rows stay inside their mask
            assert i % 8 not in (2, 7) or int(tok[i]) in set(spec)
        # the same batch without the feature, with an all-ones table and with none: the rows without repetition give
        # the same tokens in all three
        no_tab = ops.sample(xg, temp.to(cuda), topp.to(cuda), None, seeds.to(cuda), step.to(cuda), proc=pd_p,
                            mask_tab=mt_p, counts=cnt_p.clone(), bias_tab=lp_p.bias_table()).cpu()
        plain = ops.sample(xg, temp.to(cuda), topp.to(cuda), None, seeds.to(cuda), step.to(cuda), proc=pd_p,
                           mask_tab=mt_p, counts=cnt_p, bias_tab=lp_p.bias_table(), rep_tab=lp_p.rep_table()).cpu()
        assert torch.equal(plain, no_tab) and torch.equal(plain[old], tok[old]), msg
        free = [i for i in rep_rows if i % 8 != 3]
        assert int((plain[free] != tok[free]).sum()) >= 1  # (and the penalty did decide some of its own rows)
    assert changed > 20 * (V // 8)


# ---- 4. the decisive probe --------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_decisive_probe(cuda, dtype):
    """Greedy rows whose answer is the penalty's doing. Positive rows: the maximum 8.0 is seen, the runner-up 5.0 is
    not — r = 2 halves the maximum below it, r = 1 leaves it. Negative rows: the seen maximum -2.0 against the unseen
    -3.0 — r = 2 doubles it to -4.0. The two tokens sit in different splits of the 8, or one of them in the ragged tail
    (V = 16389: 8 slices of 2,048 and a tail of 5); a token is seen through the flag, a count, or both."""
    from kafka_llm_service_amd.ops._ext import ext

    V = 16389
    places = [(100, 16386), (16387, 5000), (2047, 2048), (16388, 16384), (9000, 3), (14336, 16385)]  # (seen, unseen)
    words = [FLAG, 1, FLAG + 2]
    cases = []  # (r, seen token, unseen token, positive, word)
    for j, (s, u) in enumerate(places):
        for r in (2.0, 1.0):
            for positive in (True, False):
                cases.append((r, s, u, positive, words[j % 3]))
    B = len(cases)
    x = torch.full((B, V), -10.0)
    counts = torch.zeros(B, (V + 7) // 8 * 8, dtype=torch.int32)
    rep_tab = torch.ones(B, 2)
    want = []
    g = torch.Generator().manual_seed(9)
    for b, (r, s, u, positive, word) in enumerate(cases):
        x[b, s], x[b, u] = (8.0, 5.0) if positive else (-2.0, -3.0)
        other = torch.randperm(V, generator=g)[:200]
        other = other[(other != s) & (other != u)]
        counts[b, other] = FLAG  # seen background tokens at -10: they only sink further
        counts[b, s] = word
        rep_tab[b] = torch.from_numpy(rep_factors(r))
        want.append(u if r == 2.0 else s)
    proc = torch.zeros(B, 8, dtype=torch.int32)
    proc[:, 2] = torch.arange(B, dtype=torch.int32)
    mt = torch.zeros(1, (V + 31) // 32, dtype=torch.int32)
    x = x.to(dtype)
    rep = ref.sample_replay(x, None, proc=proc, mask_tab=mt, counts=counts.clone(), nsplit=8, rep_tab=rep_tab)
    assert rep.tokens.tolist() == want and not bool(rep.ambiguous.any())
    buf = torch.full((B, (V + 7) // 8 * 8 + 8), torch.finfo(dtype).max, dtype=dtype, device=cuda)
    buf[:, :V] = x.to(cuda)
    for nsplit in (1, 8):
        out = torch.full((B,), -1, dtype=torch.long, device=cuda)
        ext().sample(buf[:, :V], None, None, None, None, None, out, _ws(cuda, B, nsplit), nsplit, proc.to(cuda),
                     mt.to(cuda), counts.clone().to(cuda), None, rep_tab.to(cuda))
        assert out.tolist() == want, nsplit
    # the public op (8 splits at this size); without the table nothing is multiplied: every row returns its maximum
    tok = ops.sample(buf[:, :V], proc=proc.to(cuda), mask_tab=mt.to(cuda), counts=counts.clone().to(cuda),
                     rep_tab=rep_tab.to(cuda))
    assert tok.tolist() == want
    tok = ops.sample(buf[:, :V], proc=proc.to(cuda), mask_tab=mt.to(cuda), counts=counts.clone().to(cuda))
    assert tok.tolist() == [s for _, s, _, _, _ in cases]


# ---- 5. the engine ----------------------------------------------------------------------------------------------------
def decided(model, prompt, out, r):
    """Per token of an engine run ``out``: (the fp32 oracle's penalised argmax given the prompt and the run's own
    earlier tokens, whether that argmax is decided against the engine's bf16 error, whether the raw argmax is another
    token). tests/test_numerics_gpu.py bounds the engine's error on a row by min(K_STD, RATIO * b + 0.02) standard
    deviations of the fp32 row, b the bf16 forward's own error on it. The penalty multiplies a logit's error by at most
    1 when the two best penalised logits are positive (factors 1 and 1 / r, r > 1) and by r otherwise, and two logits
    off by that much in opposite directions keep their order when they lie more than twice as far apart. As long as
    the run follows the oracle this is the hand loop of tests/test_repetition_penalty.py token for token."""
    f32 = dense_logits(model, prompt + out, fp32=True).float().cpu().numpy()
    b16 = dense_logits(model, prompt + out).float().cpu().numpy()
    res, figures = [], []
    for i in range(len(out)):
        row = f32[len(prompt) - 1 + i]
        sd = float(row.std())
        seen = np.zeros(row.size, dtype=bool)
        seen[prompt + out[:i]] = True
        y = penalise(row, seen, r)
        top = np.sort(y)[-2:]
        b = float(np.abs(b16[len(prompt) - 1 + i] - row).max()) / sd
        bound = 2 * min(K_STD, RATIO * b + 0.02) * sd * (1.0 if top[0] > 0 else max(r, 1 / r))
        figures.append((round(float(top[1] - top[0]), 3), round(bound, 3)))
        res.append((int(np.argmax(y)), bool(top[1] - top[0] > bound), int(np.argmax(row)) != int(np.argmax(y))))
    print(f"penalised fp32 oracle: (top-2 margin, bound) per token {figures}")
    return res


@pytest.mark.gpu
def test_engine_eager_and_graphed(cuda):
    """Greedy requests with repetition_penalty = 2 next to plain ones: wherever the fp32 oracle's penalised argmax is
    decided, the engine drew it — and some of those tokens are not the raw argmax, so the penalty was applied; the
    plain requests give the tokens of a run without the feature; the hipGraph engine gives the eager engine's tokens."""
    cfg = dict(model="tiny-llama", device="cuda:0", num_kv_blocks=512, max_model_len=2048)
    n = 16
    kw = dict(max_tokens=n, ignore_eos=True)
    eager = LLMEngine(EngineConfig(**cfg))
    eager.runner.fixed_decode_items = True  # the graph engine's decode split, so both sum in the same order
    model = eager.model
    g = torch.Generator().manual_seed(21)
    prompts = [torch.randint(0, 5000, (m,), generator=g).tolist() for m in (17, 23, 19, 12, 30, 9, 41, 14)]
    # request 0 is also compared with the hand loop itself, for the tokens that loop decides from the start: its prompt
    # is the first of a fixed list whose penalised oracle run decides at least its first token (the oracle alone says)
    for pseed in range(100, 140):
        prompts[0] = torch.randint(0, 5000, (17,), generator=torch.Generator().manual_seed(pseed)).tolist()
        hand, _ = hand_loop(model, prompts[0], 4, 2.0, fp32=True)
        k = 0
        for _, sure, _ in decided(model, prompts[0], hand, 2.0):
            if not sure:
                break
            k += 1
        if k >= 1:
            break
    else:
        pytest.fail("no prompt of the list has a penalised oracle run that decides its first token")
    rep_greedy = SamplingParams(temperature=0.0, repetition_penalty=2.0, **kw)
    sps = [rep_greedy, SamplingParams(temperature=1.2, seed=6, **kw),
           SamplingParams(temperature=1.2, seed=5, repetition_penalty=1.3, presence_penalty=0.5, **kw),
           SamplingParams(temperature=0.0, **kw), rep_greedy, rep_greedy, rep_greedy, rep_greedy]
    got = eager.generate(prompts, sps)
    assert all(len(o) == n for o in got)
    assert eager.runner.lp.stats["rep_rows"] == 6 * n and eager.runner.lp.stats["seen_uploads"] == 6
    checked = decisive = 0
    for j in (0, 4, 5, 6, 7):
        for i, (want, sure, moved) in enumerate(decided(model, prompts[j], got[j], 2.0)):
            if sure:
                assert got[j][i] == want, f"request {j} token {i}: engine {got[j][i]}, penalised oracle {want}"
                checked += 1
                decisive += moved
    print(f"{checked} of {5 * n} tokens decided, {decisive} of them not the raw argmax")
    assert checked >= 5 and decisive >= 1
    assert k >= 1 and got[0][:k] == hand[:k], f"request 0: engine {got[0][:k]}, hand loop {hand[:k]}"
    plain = LLMEngine(EngineConfig(**cfg), model=model)
    plain.runner.fixed_decode_items = True
    no_rep = SamplingParams(temperature=0.0, **kw)
    base = plain.generate(prompts, [no_rep, sps[1], SamplingParams(temperature=1.2, seed=5, presence_penalty=0.5, **kw),
                                    sps[3], no_rep, no_rep, no_rep, no_rep])
    assert base[1] == got[1] and base[3] == got[3]  # the plain requests do not notice
    assert sum(base[j] != got[j] for j in (0, 4, 5, 6, 7)) >= 1
    graphed = LLMEngine(EngineConfig(**cfg, use_graphs=True), model=model)
    got_g = graphed.generate(prompts, sps)
    assert not graphed.runner.graphs.disabled, "hipGraph capture failed (see log)"
    assert graphed.runner.graphs.stats["replays"] > 0 and got_g == got
