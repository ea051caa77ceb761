"""Engines decoding from the 12-bit packed weight twins (LLMC_PACKED_FORMAT=12, the default).

The P12 GEMVs return the bf16 GEMVs' bits, as the P13 ones do, so an engine on either format
must produce the token ids of the same engine with packed weights off: greedy and seeded sampling,
graph replay and eager steps, one-row and two-row engines. The twins are the P12 class and smaller
than the P13 ones.
"""

import pytest

from llm_consensus_amd.engine import Engine, EngineConfig, SamplingParams
from llm_consensus_amd.models.config import ModelConfig
from llm_consensus_amd.ops import wpack

pytestmark = pytest.mark.gpu

# Llama-shaped, every decode GEMV's K a whole number of units: hidden 2048 (qkv, gate_up, lm_head),
# q size 2048 (o_proj), intermediate 4096 (down)
LLAMA_P13 = ModelConfig("llama-p13-test", "llama", 2, 2048, 16, 4, 128, 4096, 2048, 500000.0, max_position=4096)
PROMPT = [1, 17, 300, 45, 1999, 7, 7, 1024, 512, 3]
N_NEW = 32


def _engine(packed, graphs, max_batch=1):
    return Engine(LLAMA_P13, EngineConfig(device="cuda:0", max_context=512, seed=3, use_graphs=graphs,
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
    L = eng.w.layers[0]
    return [t for t in (eng.w.p_lm_head, L.p_qkv, L.p_gu, L.p_down, L.p_o) if t is not None]


@pytest.mark.parametrize("max_batch", [1, 2], ids=["one-row", "two-rows"])
@pytest.mark.parametrize("graphs", [True, False], ids=["graph", "eager"])
def test_packed12_engine_tokens(cuda, monkeypatch, graphs, max_batch):
    two = max_batch == 2
    monkeypatch.delenv("LLMC_PACKED_FORMAT", raising=False)
    off = _engine("off", graphs, max_batch)
    assert not off.packed
    want = _tokens(off, two)
    del off

    monkeypatch.setenv("LLMC_PACKED_FORMAT", "13")
    e13 = _engine("on", graphs, max_batch)
    assert e13.packed and _twins(e13) and all(isinstance(t, wpack.PackedWeight) for t in _twins(e13))
    bytes13 = e13.w.packed_nbytes()
    assert _tokens(e13, two) == want
    del e13

    monkeypatch.setenv("LLMC_PACKED_FORMAT", "12")
    e12 = _engine("on", graphs, max_batch)
    assert e12.packed and len(_twins(e12)) >= 4 and all(isinstance(t, wpack.PackedWeight12) for t in _twins(e12))
    assert 0 < e12.w.packed_nbytes() < bytes13
    assert e12.w.packed_nbytes() <= e12.w.packed_demand(with_o=two or not all(e12.ao_chunks))
    assert _tokens(e12, two) == want


def test_the_default_format_is_12(cuda, monkeypatch):
    monkeypatch.delenv("LLMC_PACKED_FORMAT", raising=False)
    eng = _engine("auto", False)
    assert eng.packed and all(isinstance(t, wpack.PackedWeight12) for t in _twins(eng))
