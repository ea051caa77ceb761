"""Qwen3-8B decode A/B: what the per-head q/k norm launch costs per token (profiles/r14_qwen3.md).

One process, one GPU, batch 1, random-init weights: an engine of ``qwen3-8b`` (qkv GEMV with the
bf16 epilogue, then the norm + RoPE + KV-write launch of csrc/kernels/qk_norm_rope.hip) and an engine
of ``qwen3-8b.with_(qk_norm=False)`` (the same shapes through the fused RoPE epilogue), measured
alternately. Decode ms/token = (time of prompt + N tokens - time of prompt + n tokens) / (N - n),
host clock around runs that end in a device synchronise, so the prefill cancels. Then the norm kernel
alone at T = 1 and T = 8192 beside the plain ``rope_kv_write``, device events around back-to-back
launches on one stream (at T = 1 that is the launch rate, not the kernel's own duration).

    python scripts/qwen3_decode_ab.py [--prompt 1900] [--tokens 128] [--reps 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from llm_consensus_amd import ops  # noqa: E402
from llm_consensus_amd.engine import Engine, EngineConfig  # noqa: E402
from llm_consensus_amd.models.config import FAMILIES, rope_inv_freq  # noqa: E402
from llm_consensus_amd.ops import oracle  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="qwen3-8b")
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


# -- engines --------------------------------------------------------------------------------------
cfg = FAMILIES[a.model]
assert cfg.qk_norm
prompt = [(i * 7919) % 30000 + 256 for i in range(a.prompt)]
engines = {}
for tag, c in (("qk_norm", cfg), ("fused_rope", cfg.with_(name=cfg.name + "-nonorm", qk_norm=False))):
    e = Engine(c, EngineConfig(device="cuda:0", max_context=a.ctx, seed=1))
    e.warmup_graphs([1])  # every bucket's decode graph now: nothing is captured inside a timed run
    e.generate_ids(prompt, 16, stop_on_eos=False)
    engines[tag] = e
    emit(tag + "_engine", {"packed": bool(e.packed), "attn_oproj_buckets": sum(1 for ch in e.ao_chunks if ch),
                           "qkv_attn_buckets": sum(1 for p in e.qa_plan if p)})


def timed(e, n):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = e.generate_ids(prompt, n, stop_on_eos=False)
    torch.cuda.synchronize()
    assert len(out) == n
    return time.perf_counter() - t


runs = {tag: [] for tag in engines}
for _ in range(a.reps):
    for tag, e in engines.items():  # alternated
        short = timed(e, a.short)
        runs[tag].append(1000 * (timed(e, a.short + a.tokens) - short) / a.tokens)
emit("decode_ms_per_token", {tag: [round(v, 4) for v in vs] for tag, vs in runs.items()})
mean = {tag: sum(vs) / len(vs) for tag, vs in runs.items()}
emit("decode_ms_per_token_mean", {tag: round(v, 4) for tag, v in mean.items()})
emit("norm_launch_cost_us_per_layer", round(1000 * (mean["qk_norm"] - mean["fused_rope"]) / cfg.n_layers, 3))
del engines, e
torch.cuda.empty_cache()

# -- the kernel alone ---------------------------------------------------------------------------------
nh, nkv, D, bs = cfg.n_heads, cfg.n_kv_heads, cfg.head_dim, 64
cos_t, sin_t = (t.cuda() for t in oracle.rope_tables(rope_inv_freq(cfg), 16384))
gq = (1 + 0.3 * torch.randn(D, device="cuda")).to(torch.bfloat16)
gk = (1 + 0.3 * torch.randn(D, device="cuda")).to(torch.bfloat16)
side = torch.cuda.Stream()
for T, iters in ((1, 4000), (8192, 200)):
    qkv = torch.randn(T, (nh + 2 * nkv) * D, device="cuda").to(torch.bfloat16)
    q = torch.zeros(T, nh * D, dtype=torch.bfloat16, device="cuda")
    nb = (T + bs - 1) // bs + 1
    kc = torch.zeros(nb, nkv, bs, D, dtype=torch.bfloat16, device="cuda")
    vc = torch.zeros_like(kc)
    pos = torch.arange(T, dtype=torch.int32, device="cuda")
    slots = torch.randperm(nb * bs, device="cuda")[:T].to(torch.int32)
    row = {}
    for tag, kw in (("qk_norm_rope_kv_write", dict(q_norm=gq, k_norm=gk, qk_eps=cfg.rms_eps)), ("rope_kv_write", {})):
        def launch():
            ops.rope_kv_write(qkv, pos, cos_t, sin_t, kc, vc, slots, nh, nkv, D, bs, q, **kw)

        for _ in range(20):
            launch()
        # a captured graph of 100 launches, replayed: the host's Python is out of the timed window
        per_graph = 100
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            for _ in range(per_graph):
                launch()
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
            best.append(1000 * e0.elapsed_time(e1) / (iters // per_graph * per_graph))
        row[tag] = [round(v, 3) for v in best]
    nbytes = T * ((nh + 2 * nkv) * D + (nh + 2 * nkv) * D) * 2  # read the row, write q, k and v
    row["bytes_moved"] = nbytes
    emit(f"kernel_us_T{T}", row)

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        json.dump(res, f, indent=1)
