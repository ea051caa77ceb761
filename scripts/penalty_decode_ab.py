"""Decode A/B of the sampling penalties (profiles/r15_sampling_penalties.md).

One process, one GPU, one engine, batch 1, random-init weights: the same prompt decoded unpenalised
and with repetition / frequency / presence penalties (the penalty launch ahead of the sampler, the
count in the state advance), both over captured graphs, measured alternately. Decode ms/token =
(time of prompt + N tokens - time of prompt + n tokens) / (N - n), host clock around runs that end in
a device synchronise, so the prefill, the bind and the seeding of the history words cancel. Then
``penalize_logits`` alone at the model's vocabulary with a history of the prompt's size, device events
around replays of a captured graph of 100 launches (back to back on one stream: the launch rate when
the kernel is shorter than a launch).

    python scripts/penalty_decode_ab.py [--model llama-3-8b] [--prompt 1900] [--tokens 128] [--out FILE]
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
forms = {"plain": {}, "penalised": PEN}
e = Engine(cfg, EngineConfig(device="cuda:0", max_context=a.ctx, seed=1))
e.warmup_graphs([1])  # every bucket's decode graph of both forms now: nothing is captured inside a timed run
e.warmup_graphs([1], SamplingForm(penalties=True))
for kw in forms.values():
    e.generate_ids(prompt, 16, temperature=0.0, stop_on_eos=False, **kw)
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
emit("penalty_cost_us_per_token", round(1000 * (mean["penalised"] - mean["plain"]), 3))
emit("penalty_cost_share_of_step", round((mean["penalised"] - mean["plain"]) / mean["plain"], 5))
del e
torch.cuda.empty_cache()

# -- the kernel alone ---------------------------------------------------------------------------------
V = cfg.vocab
side = torch.cuda.Stream()
for B in (1, 4):
    logits = torch.randn(B, V, device="cuda") * 3
    words = torch.zeros(B, V, dtype=torch.int16, device="cuda")
    ids = torch.tensor(prompt, dtype=torch.int32, device="cuda")
    for b in range(B):
        ops.penalty_seed(words[b], ids)
        words[b, 1000:1100] += 3  # a hundred generated ids
    rep, freq, pres = (torch.full((B,), v, device="cuda") for v in (1.3, 0.2, 0.5))
    for _ in range(20):
        ops.penalize_logits(logits, words, rep, freq, pres)
    per_graph, iters = 100, 4000
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
        for _ in range(per_graph):
            ops.penalize_logits(logits, words, rep, freq, pres)
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
    touched = int((words != 0).sum().item())
    emit(f"penalize_logits_us_B{B}", {"per_launch": [round(v, 3) for v in best], "words_bytes": 2 * B * V,
                                     "logit_bytes_touched": 8 * touched})

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        json.dump(res, f, indent=1)
