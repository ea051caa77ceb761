"""Decode A/B of the token log-probabilities (profiles/r16_logprobs.md).

One process, one GPU, one engine, batch 1, random-init weights: the same prompt decoded with
``logprobs`` off, with ``logprobs = 20``, and with penalties plus ``logprobs = 20`` (the raw-row copy
between the stages), all over captured graphs, measured alternately. Decode ms/token =
(time of prompt + N tokens - time of prompt + n tokens) / (N - n), host clock around runs that end in
a device synchronise, so the prefill and the bind cancel. Then the two launches alone at the model's
vocabulary, device events around replays of a captured graph of 100 pairs (back to back on one
stream), for N = 20, 5 and 0.

    python scripts/logprobs_decode_ab.py [--model llama-3-8b] [--prompt 1900] [--tokens 128] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from llm_consensus_amd import ops  # noqa: E402
from llm_consensus_amd.engine import Engine, EngineConfig, SamplingForm  # noqa: E402
from llm_consensus_amd.models.config import FAMILIES  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="llama-3-8b")
ap.add_argument("--prompt", type=int, default=1900)
ap.add_argument("--tokens", type=int, default=128)
ap.add_argument("--short", type=int, default=8)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--ctx", type=int, default=4096)
ap.add_argument("--out", default="")
a = ap.parse_args()
assert torch.cuda.is_available(), "needs a GPU"
res = {"model": a.model, "prompt": a.prompt, "tokens": a.tokens}


def emit(key, val):
    res[key] = val
    print(json.dumps({key: val}), flush=True)


cfg = FAMILIES[a.model]
prompt = [(i * 7919) % 30000 + 256 for i in range(a.prompt)]
PEN = dict(repetition_penalty=1.3, frequency_penalty=0.2, presence_penalty=0.5)
forms = {"off": {}, "logprobs20": dict(logprobs=20), "penalised": PEN, "penalised_logprobs20": dict(logprobs=20, **PEN)}
e = Engine(cfg, EngineConfig(device="cuda:0", max_context=a.ctx, seed=1))
# every bucket's decode graph of the four forms now: nothing is captured inside a timed run
for pen in (False, True):
    for lp in (False, True):
        e.warmup_graphs([1], SamplingForm(penalties=pen, logprobs=lp))
outs = {tag: e.generate_ids(prompt, 16, temperature=0.0, stop_on_eos=False, **kw) for tag, kw in forms.items()}
assert list(outs["off"]) == list(outs["logprobs20"]) and list(outs["penalised"]) == list(outs["penalised_logprobs20"])
emit("engine", {"packed": bool(e.packed), "graphs": sorted(str(k) for k in e._graphs), "vocab": cfg.vocab})


def timed(kw, n):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = e.generate_ids(prompt, n, temperature=0.0, stop_on_eos=False, **kw)
    torch.cuda.synchronize()
    assert len(out) == n
    return time.perf_counter() - t


runs = {tag: [] for tag in forms}
for _ in range(a.reps):
    for tag, kw in forms.items():  # alternated
        short = timed(kw, a.short)
        runs[tag].append(1000 * (timed(kw, a.short + a.tokens) - short) / a.tokens)
emit("decode_ms_per_token", {tag: [round(v, 4) for v in vs] for tag, vs in runs.items()})
mean = {tag: sum(vs) / len(vs) for tag, vs in runs.items()}
emit("decode_ms_per_token_mean", {tag: round(v, 4) for tag, v in mean.items()})
for on, off in (("logprobs20", "off"), ("penalised_logprobs20", "penalised")):
    emit(f"cost_us_per_token_{on}", round(1000 * (mean[on] - mean[off]), 3))
    emit(f"cost_share_of_step_{on}", round((mean[on] - mean[off]) / mean[off], 5))
del e
torch.cuda.empty_cache()

# -- the two launches alone -----------------------------------------------------------------------------
V = cfg.vocab
side = torch.cuda.Stream()
for B, n in ((1, 20), (1, 5), (1, 0), (4, 20)):
    logits = torch.randn(B, V, device="cuda") * 3
    tokens = torch.randint(0, V, (B,), dtype=torch.int32, device="cuda")
    ws = ops.logprobs_workspace(B, n, "cuda")
    lt = torch.zeros(B, 1, device="cuda")
    tv = torch.zeros(B, 1, 20, device="cuda")
    ti = torch.zeros(B, 1, 20, dtype=torch.int32, device="cuda")

    def pair():
        ops.logprobs_stage1(logits, n, ws)
        ops.logprobs_stage2(logits, tokens, n, ws, lt, tv, ti)

    for _ in range(20):
        pair()
    per_graph, iters = 100, 4000
    torch.cuda.synchronize()
    for what, fn in (("pair", pair), ("stage1", lambda: ops.logprobs_stage1(logits, n, ws))):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            for _ in range(per_graph):
                fn()
        graph.replay()
        best = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(iters // per_graph):
                graph.replay()
            e1.record()
            torch.cuda.synchronize()
            best.append(1000 * e0.elapsed_time(e1) / iters)
        emit(f"logprobs_{what}_us_B{B}_N{n}", {"per_launch": [round(v, 3) for v in best], "row_bytes": 4 * B * V})

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        json.dump(res, f, indent=1)
