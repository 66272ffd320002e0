"""Structured-output kernel time at V = 128,256 (the Llama-3 token table) for 1, 16 and 64 rows: schema mask + advance
(ops/csrc/table_grammar.hip) for four schemas — tiny, about ten properties, one padded to just under SCHEMA_LDS_BYTES (all
three staged in LDS; the last sets the launch's LDS allocation to its maximum), large (table walked in global memory) —
and two states (inside a free string, after a value), beside the JSON-mode kernels
(ops/csrc/json_mask.hip) over the same token table, row counts and kind of state as the yardstick. Device events
around 200 back-to-back launches; everything measured alternates round by round (5 rounds) and the medians are
reported, one JSON line per (schema, state, rows) with the ratio to the yardstick.

  --tokens N ...   tokens one workgroup walks per staged table (default: 1024 2048 4096; the first listed that equals
                   ops.SCHEMA_MASK_TOKENS is the shipped one)
  --bytewise       also time the byte-at-a-time token loads
"""
import argparse
import json
import statistics

import numpy as np
import torch

from kafka_llm_service_amd import ops
from kafka_llm_service_amd.engine import json_mode as jm
from kafka_llm_service_amd.engine import json_schema as js
from kafka_llm_service_amd.engine.tokenizer import get_tokenizer
from kafka_llm_service_amd.ops import reference as ref

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, nargs="*", default=[1, 16, 64])
ap.add_argument("--tokens", type=int, nargs="*", default=[1024, 2048, 4096])
ap.add_argument("--bytewise", action="store_true")
ap.add_argument("--tag", default="")
a = ap.parse_args()


def obj(props):
    return {"type": "object", "properties": props, "required": list(props), "additionalProperties": False}


STR, INT, NUM, BOOL = ({"type": t} for t in ("string", "integer", "number", "boolean"))
SCHEMAS = {
    "tiny": obj({"s": STR, "n": INT}),
    "ten-properties": obj({"s": STR, "n": INT, "price": NUM, "ok": BOOL, "color": {"enum": ["red", "green", "blue"]},
                           "tags": {"type": "array", "items": STR}, "note": {"type": ["string", "null"]},
                           "pos": obj({"x": NUM, "y": NUM}), "count": INT, "last": BOOL}),
    "lds-limit": None,  # (below: the tiny schema and an enum padded until the table just fits SCHEMA_LDS_BYTES)
    "large": obj({"s": STR, "n": INT, "e": {"enum": ["member-%04d" % (i * 7919 % 10000) for i in range(600)]},
                  "items": {"type": "array", "items": obj({"name": STR, "qty": INT})}}),
}
PREFIX = {"in-string": b'{"s":"va', "after-value": b'{"s":"v","n":1 '}
JSON_PREFIX = {"in-string": b'{"k":"va', "after-value": b'{"k":[1 '}

dev = torch.device("cuda:0")
tok = get_tokenizer()
table = jm.table_for(tok, tok.eos_ids)
tabs = ops.JsonTables(table, dev)
V, ROW0 = table.V, 512


def _limit(k):
    return obj({"s": STR, "n": INT, "pad": {"enum": ["m%03d" % i for i in range(k)]}})


k = 1
while js.compile_schema(_limit(k + 1)).nbytes <= js.SCHEMA_LDS_BYTES:
    k += 1
SCHEMAS["lds-limit"] = _limit(k)
dfas = {n: js.compile_schema(s) for n, s in SCHEMAS.items()}
assert dfas["ten-properties"].nbytes <= js.SCHEMA_LDS_BYTES < dfas["large"].nbytes
assert js.SCHEMA_LDS_BYTES - 4 * dfas["lds-limit"].C * 2 < dfas["lds-limit"].nbytes <= js.SCHEMA_LDS_BYTES
pool = ops.SchemaTables(4, dev)
BUF = {n: i for i, n in enumerate(SCHEMAS)}
for n, d in dfas.items():
    pool.load(BUF[n], d.cls, d.trans)


def window(fn) -> float:
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(200):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / 200


for state_name in PREFIX:
    jst = ref.json_walk(jm.START_STATE, JSON_PREFIX[state_name])
    for B in a.rows:
        lg = (torch.randn(B, V, generator=torch.Generator().manual_seed(0)) * 3).to(torch.bfloat16).to(dev)
        mask_tab = torch.zeros(ROW0 + B, table.W, dtype=torch.int32, device=dev)
        proc = np.zeros((B, 8), dtype=np.int32)
        proc[:, 0], proc[:, 1], proc[:, 2] = 1, ROW0 + np.arange(B), -1
        proc = torch.from_numpy(proc).to(dev)
        t = torch.full((B,), 0.7, device=dev)
        sd = torch.arange(B, dtype=torch.int64, device=dev)
        bias = torch.zeros(1, 2 * ops.LOGIT_BIAS_MAX, dtype=torch.int32, device=dev)
        fns, outs = {}, {}
        # the yardstick: JSON mode in the same kind of state
        jstate0 = torch.from_numpy(np.tile(jm.state_record(jst), (B, 1))).to(dev)
        jstate = jstate0.clone()
        jrows = torch.from_numpy(np.stack([np.arange(B), np.arange(B)], axis=1).astype(np.int32)).to(dev)
        jout = torch.zeros(B, dtype=torch.int64, device=dev)
        ops.json_mask(tabs, jrows, jstate, mask_tab, ROW0)
        ops.sample(lg, t, seeds=sd, out=jout, proc=proc, mask_tab=mask_tab, bias_tab=bias)  # ids the advance walks

        def json_mode():
            jstate.copy_(jstate0)
            ops.json_mask(tabs, jrows, jstate, mask_tab, ROW0)
            ops.json_advance(tabs, jrows, jout, jstate)

        fns["json_mode"] = json_mode
        fns["reset"] = lambda: jstate.copy_(jstate0)
        live = {}
        for name, dfa in dfas.items():
            s0 = ref.schema_walk(js.START, PREFIX[state_name], dfa)
            live[name] = int(np.unpackbits(ref.schema_mask_ref(s0, dfa, table).view(np.uint8)).sum())
            st0 = torch.from_numpy(np.tile(js.state_record(s0, BUF[name]), (B, 1))).to(dev)
            st = st0.clone()
            rows = torch.from_numpy(np.stack([np.arange(B), np.arange(B), np.full(B, BUF[name])], axis=1)
                                    .astype(np.int32)).to(dev)
            out = torch.zeros(B, dtype=torch.int64, device=dev)
            ops.schema_mask(tabs, pool, rows, B, st, mask_tab, ROW0)
            ops.sample(lg, t, seeds=sd, out=out, proc=proc, mask_tab=mask_tab, bias_tab=bias)
            for tokens in a.tokens:
                for dword in ([True, False] if a.bytewise else [True]):
                    def schema(st=st, st0=st0, rows=rows, out=out, tokens=tokens, dword=dword):
                        st.copy_(st0)
                        ops.schema_mask(tabs, pool, rows, B, st, mask_tab, ROW0, tokens=tokens, dword=dword)
                        ops.schema_advance(tabs, pool, rows, out, st)

                    fns[(name, tokens, dword)] = schema
        res = {k: [] for k in fns}
        for _ in range(5):  # interleaved rounds
            for k, fn in fns.items():
                res[k].append(window(fn))
        med = {k: statistics.median(v) for k, v in res.items()}
        yard = med["json_mode"] - med["reset"]
        for k in fns:
            if isinstance(k, tuple):
                name, tokens, dword = k
                us = med[k] - med["reset"]
                print(json.dumps({"bench": "json_schema", "tag": a.tag, "schema": name, "states": dfas[name].S,
                                  "classes": dfas[name].C, "table_bytes": dfas[name].nbytes,
                                  "table_in": "lds" if dfas[name].nbytes <= js.SCHEMA_LDS_BYTES else "global",
                                  "state": state_name, "rows": B, "vocab": V, "live_tokens": live[name],
                                  "tokens_per_workgroup": tokens, "dword_loads": dword,
                                  "mask_plus_advance_us": round(us, 2), "json_mode_us": round(yard, 2),
                                  "ratio_to_json_mode": round(us / yard, 3), "state_reset_us": round(med["reset"], 2),
                                  "min_max": [round(min(res[k]), 2), round(max(res[k]), 2)]}), flush=True)
