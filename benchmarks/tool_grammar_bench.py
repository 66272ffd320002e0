"""Tool grammar kernel time at V = 128,256 (the Llama-3 token table) for 1, 16 and 64 rows: tool mask + advance
(ops/csrc/table_grammar.hip) per phase of the envelope, beside schema mask + advance (the same kernels) over the
same table, state and row count in the same process as the yardstick. Two call bodies: the shell tools (table staged in
LDS) and a tool with a 600-member enum (table walked in global memory); the BODY rows stand inside a free string.
Device events around 200 back-to-back launches; everything measured alternates round by round (5 rounds) and the
medians are reported, one JSON line per (body, phase, rows).
"""
import argparse
import json
import statistics

import numpy as np
import torch

from kafka_llm_service_amd import ops
from kafka_llm_service_amd.engine import json_mode as jm
from kafka_llm_service_amd.engine import json_schema as js
from kafka_llm_service_amd.engine import tool_automaton as ta
from kafka_llm_service_amd.engine.tokenizer import get_tokenizer
from kafka_llm_service_amd.ops import reference as ref

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, nargs="*", default=[1, 16, 64])
ap.add_argument("--tag", default="")
a = ap.parse_args()


def fn(name, params):
    return {"type": "function", "function": {"name": name, "parameters": params}}


STR = {"type": "string"}
BODIES = {
    "shell": ([fn("shell_exec", {"type": "object", "properties": {"shell_id": STR, "command": STR},
                                 "required": ["shell_id", "command"]}),
               fn("create_shell", {"type": "object", "properties": {"shell_id": STR}, "required": ["shell_id"]})],
              b'{"name":"shell_exec","parameters":{"shell_id":"ma'),
    "large": ([fn("pick", {"type": "object", "required": ["s", "e"], "properties": {
        "s": STR, "e": {"enum": ["member-%04d" % (i * 7919 % 10000) for i in range(600)]}}})],
        b'{"name":"pick","parameters":{"s":"va'),
}
PHASES = {"free": ta.TOOL_FREE, "open": ta.TOOL_OPEN, "body": ta.TOOL_BODY, "body-done": ta.TOOL_BODY,
          "text": ta.TOOL_TEXT, "closed": ta.TOOL_CLOSED}

dev = torch.device("cuda:0")
tok = get_tokenizer()
table = jm.table_for(tok, tok.eos_ids)
tabs = ops.JsonTables(table, dev)
V, ROW0 = table.V, 512
OPEN, CLOSE = tok.special_id("<|python_tag|>"), tok.special_id("<|eom_id|>")
dfas = {n: ta.compile_tool_body(t, [x["function"]["name"] for x in t], "llama3") for n, (t, _) in BODIES.items()}
assert dfas["shell"].nbytes <= js.SCHEMA_LDS_BYTES < dfas["large"].nbytes
pool = ops.SchemaTables(2, dev)
BUF = {n: i for i, n in enumerate(BODIES)}
for n, d in dfas.items():
    pool.load(BUF[n], d.cls, d.trans)


def window(f) -> float:
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(20):
        f()
    torch.cuda.synchronize()
    s.record()
    for _ in range(200):
        f()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / 200


for B in a.rows:
    lg = (torch.randn(B, V, generator=torch.Generator().manual_seed(0)) * 3).to(torch.bfloat16).to(dev)
    mask_tab = torch.zeros(ROW0 + B, table.W, dtype=torch.int32, device=dev)
    proc = np.zeros((B, 8), dtype=np.int32)
    proc[:, 0], proc[:, 1], proc[:, 2] = 1, ROW0 + np.arange(B), -1
    proc = torch.from_numpy(proc).to(dev)
    t = torch.full((B,), 0.7, device=dev)
    sd = torch.arange(B, dtype=torch.int64, device=dev)
    bias = torch.zeros(1, 2 * ops.LOGIT_BIAS_MAX, dtype=torch.int32, device=dev)
    scratch0 = torch.zeros(B, 4, dtype=torch.int32, device=dev)
    scratch = scratch0.clone()
    fns = {"reset": lambda: scratch.copy_(scratch0)}
    for name, dfa in dfas.items():
        s0 = ref.schema_walk(js.START, BODIES[name][1], dfa)
        assert s0 not in (js.DEAD, js.DONE)
        # the yardstick: the schema kernels over the same table in the same state
        st0 = torch.from_numpy(np.tile(js.state_record(s0, BUF[name]), (B, 1))).to(dev)
        st = st0.clone()
        rows = torch.from_numpy(np.stack([np.arange(B), np.arange(B), np.full(B, BUF[name])], axis=1)
                                .astype(np.int32)).to(dev)
        out = torch.zeros(B, dtype=torch.int64, device=dev)
        ops.schema_mask(tabs, pool, rows, B, st, mask_tab, ROW0, used=[BUF[name]])
        ops.sample(lg, t, seeds=sd, out=out, proc=proc, mask_tab=mask_tab, bias_tab=bias)  # ids the advances walk

        def schema(st=st, st0=st0, rows=rows, out=out, name=name):
            st.copy_(st0)
            ops.schema_mask(tabs, pool, rows, B, st, mask_tab, ROW0, used=[BUF[name]])
            ops.schema_advance(tabs, pool, rows, out, st)

        fns[(name, "schema")] = schema
        trows = torch.from_numpy(np.stack([np.arange(B), np.arange(B), np.full(B, BUF[name]), np.full(B, OPEN),
                                           np.full(B, CLOSE)], axis=1).astype(np.int32)).to(dev)
        for phase, ph in PHASES.items():
            s = js.DONE if phase in ("body-done", "closed") else s0 if phase == "body" else js.START
            r0 = torch.from_numpy(np.tile(ta.tool_record(s, ph, BUF[name]), (B, 1))).to(dev)
            r = r0.clone()

            def tool(r=r, r0=r0, trows=trows, out=out, name=name):
                r.copy_(r0)
                ops.tool_mask(tabs, pool, trows, B, r, mask_tab, ROW0, used=[BUF[name]])
                ops.tool_advance(tabs, pool, trows, out, r)

            fns[(name, phase)] = tool
    res = {k: [] for k in fns}
    for _ in range(5):  # interleaved rounds
        for k, f in fns.items():
            res[k].append(window(f))
    med = {k: statistics.median(v) for k, v in res.items()}
    for k in fns:
        if isinstance(k, tuple) and k[1] != "schema":
            name, phase = k
            us, yard = med[k] - med["reset"], med[(name, "schema")] - med["reset"]
            print(json.dumps({"bench": "tool_grammar", "tag": a.tag, "body": name, "states": dfas[name].S,
                              "classes": dfas[name].C, "table_bytes": dfas[name].nbytes,
                              "table_in": "lds" if dfas[name].nbytes <= js.SCHEMA_LDS_BYTES else "global",
                              "phase": phase, "rows": B, "vocab": V, "mask_plus_advance_us": round(us, 2),
                              "schema_kernels_us": round(yard, 2), "ratio_to_schema": round(us / yard, 3),
                              "state_reset_us": round(med["reset"], 2),
                              "min_max": [round(min(res[k]), 2), round(max(res[k]), 2)]}), flush=True)
