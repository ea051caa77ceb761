"""Engines whose every decode GEMV has a K off the 2048-weight unit, decoding from 12-bit twins with a
row tail (``ops.wpack.PackedWeight12Tail``).

The tail GEMVs return the bf16 GEMVs' bits, so the engine must produce the token ids of the same
engine with packed weights off: greedy and seeded sampling, graph replay and eager steps, one-row
and two-row engines, with and without the q/k/v bias of the Qwen2 family. The 13-bit format has no
tail: under LLMC_PACKED_FORMAT=13 such an engine builds no twin and streams bf16.
"""

import pytest

from llm_consensus_amd.engine import Engine, EngineConfig, SamplingParams
from llm_consensus_amd.models.config import ModelConfig
from llm_consensus_amd.ops import wpack

pytestmark = pytest.mark.gpu

# Llama-shaped: hidden 2560 (qkv, gate_up, lm_head: K = 2560), 20 q / 10 kv heads x 128 (o_proj: K = 2560),
# intermediate 3584 (down: K = 3584)
LLAMA_TAIL = ModelConfig("llama-tail-test", "llama", 2, 2560, 20, 10, 128, 3584, 2048, 500000.0, max_position=4096)
CONFIGS = {"llama": LLAMA_TAIL, "qkv-bias": LLAMA_TAIL.with_(name="llama-tail-bias-test", qkv_bias=True)}
PROMPT = [1, 17, 300, 45, 1999, 7, 7, 1024, 512, 3]
N_NEW = 32


def _engine(cfg, packed, graphs, max_batch=1):
    return Engine(cfg, EngineConfig(device="cuda:0", max_context=512, seed=3, use_graphs=graphs,
                                    steps_per_graph=4, packed_weights=packed, max_batch=max_batch))


def _tokens(eng, two_rows=False):
    greedy = eng.generate_ids(PROMPT, N_NEW, temperature=0.0, stop_on_eos=False)
    sampled = eng.generate_ids(PROMPT, N_NEW, temperature=0.9, top_p=0.95, top_k=40, seed=1234, stop_on_eos=False)
    out = [greedy, sampled]
    if two_rows:
        ps = [SamplingParams(N_NEW, 0.0, 1.0, 0, 0, False), SamplingParams(N_NEW, 0.8, 1.0, 0, 99, False)]
        out += eng.generate_batch([PROMPT, PROMPT[::-1]], ps)
    assert all(len(t) == N_NEW for t in out)
    return out


def _twins(eng):
    ts = [eng.w.p_lm_head]
    for L in eng.w.layers:
        ts += [L.p_qkv, L.p_gu, L.p_down, L.p_o]
    return [t for t in ts if t is not None]


@pytest.mark.parametrize("max_batch", [1, 2], ids=["one-row", "two-rows"])
@pytest.mark.parametrize("graphs", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("model", list(CONFIGS))
def test_packed12_tail_engine_tokens(cuda, monkeypatch, model, graphs, max_batch):
    cfg, two = CONFIGS[model], max_batch == 2
    monkeypatch.delenv("LLMC_PACKED_FORMAT", raising=False)
    off = _engine(cfg, "off", graphs, max_batch)
    assert not off.packed and not _twins(off)
    want = _tokens(off, two)
    del off

    eng = _engine(cfg, "on", graphs, max_batch)
    with_o = two or not all(eng.ao_chunks)
    assert eng.packed and len(_twins(eng)) == 1 + 2 * (4 if with_o else 3)
    assert all(type(t) is wpack.PackedWeight12Tail for t in _twins(eng))
    assert 0 < eng.w.packed_nbytes() <= eng.w.packed_demand(with_o=with_o)
    assert _tokens(eng, two) == want
    del eng

    monkeypatch.setenv("LLMC_PACKED_FORMAT", "13")  # no 13-bit tail: bf16, the same tokens
    e13 = _engine(cfg, "on", graphs, max_batch)
    assert not e13.packed and not _twins(e13)
    assert _tokens(e13, two) == want
