"""Engines decoding from the 13-bit packed weight twins (EngineConfig.packed_weights).

The packed GEMVs return the bf16 GEMVs' bits, so an engine with the option on must produce the
token ids of the same engine with it off: greedy and seeded sampling, graph replay and eager steps.
A model whose rows are shorter than one 2048-weight unit runs with the option on and packs nothing.
"""

import pytest
import torch

from llm_consensus_amd.engine import Engine, EngineConfig, SamplingParams
from llm_consensus_amd.models.config import LLAMA_TINY, ModelConfig

pytestmark = pytest.mark.gpu

# Llama-shaped, every decode GEMV's K a whole number of units: hidden 2048 (qkv, gate_up, lm_head),
# q size 2048 (o_proj), intermediate 4096 (down)
LLAMA_P13 = ModelConfig("llama-p13-test", "llama", 2, 2048, 16, 4, 128, 4096, 2048, 500000.0, max_position=4096)
PROMPT = [1, 17, 300, 45, 1999, 7, 7, 1024, 512, 3]
N_NEW = 32


def _engine(cfg, packed, graphs, attn_oproj=True, max_batch=1):
    return Engine(cfg, EngineConfig(device="cuda:0", max_context=512, seed=3, use_graphs=graphs, steps_per_graph=4,
                                    packed_weights=packed, attn_oproj=attn_oproj, max_batch=max_batch))


def _tokens(eng, two_rows=False):
    greedy = eng.generate_ids(PROMPT, N_NEW, temperature=0.0, stop_on_eos=False)
    sampled = eng.generate_ids(PROMPT, N_NEW, temperature=0.9, top_p=0.95, top_k=40, seed=1234, stop_on_eos=False)
    out = [greedy, sampled]
    if two_rows:
        ps = [SamplingParams(N_NEW, 0.0, 1.0, 0, 0, False), SamplingParams(N_NEW, 0.8, 1.0, 0, 99, False)]
        out += eng.generate_batch([PROMPT, PROMPT[::-1]], ps)
    assert all(len(t) == N_NEW for t in out)
    return out


@pytest.mark.parametrize("attn_oproj", [True, False], ids=["fused-attn-oproj", "o-gemv"])
@pytest.mark.parametrize("graphs", [True, False], ids=["graph", "eager"])
def test_packed_engine_tokens(cuda, graphs, attn_oproj):
    off = _engine(LLAMA_P13, "off", graphs, attn_oproj)
    assert not off.packed and off.w.p_lm_head is None
    want = _tokens(off)
    del off
    eng = _engine(LLAMA_P13, "on", graphs, attn_oproj)
    assert eng.packed
    L = eng.w.layers[0]
    assert eng.w.p_lm_head is not None and L.p_qkv is not None and L.p_gu is not None and L.p_down is not None
    # the o_proj twin only where some bucket runs the o GEMV
    assert (L.p_o is None) == (attn_oproj and all(eng.ao_chunks))
    assert eng.w.packed_nbytes() > 0
    assert _tokens(eng) == want


def test_graph_equals_eager_and_two_rows(cuda):
    """Two-row engine (M = 2 GEMVs, the o GEMV in every bucket): packed graph == packed eager == bf16."""
    want = _tokens(_engine(LLAMA_P13, "off", True, max_batch=2), two_rows=True)
    for graphs in (True, False):
        eng = _engine(LLAMA_P13, "on", graphs, max_batch=2)
        assert eng.packed and eng.w.layers[0].p_o is not None
        assert _tokens(eng, two_rows=True) == want


def test_auto_is_on_for_a_dense_gpu_engine(cuda):
    eng = _engine(LLAMA_P13, "auto", False)
    assert eng.packed
    eng = _engine(LLAMA_P13, "auto", False, max_batch=4)  # decodes on the MFMA form: bf16 only
    assert not eng.packed


def test_short_rows_pack_nothing(cuda):
    prompt = [1, 17, 300, 45, 999, 7]
    on, off = _engine(LLAMA_TINY, "on", True), _engine(LLAMA_TINY, "off", True)
    assert not on.packed and on.w.p_lm_head is None and on.w.packed_nbytes() == 0
    a = on.generate_ids(prompt, N_NEW, temperature=0.0, stop_on_eos=False)
    b = off.generate_ids(prompt, N_NEW, temperature=0.0, stop_on_eos=False)
    assert a == b and len(a) == N_NEW
