"""MoE engines decoding from the 12-bit twins of their expert stacks (and of their dense weights).

The packed expert GEMVs return the bf16 launches' bits, so a MoE engine with packed weights on must
produce the token ids of the same engine with them off: greedy and seeded sampling, graph replay and
eager steps, one-row and two-row engines. The expert stacks' twins are ``PackedExperts12``; a
three-row engine decodes on the MFMA form and stays unpacked.
"""

import pytest

from llm_consensus_amd.engine import Engine, EngineConfig, SamplingParams
from llm_consensus_amd.models.config import ModelConfig
from llm_consensus_amd.ops import wpack

pytestmark = pytest.mark.gpu

# Mixtral-shaped, every decode GEMV's K one 2048-weight unit: 2 layers, hidden 2048, 16 / 4 heads x 128,
# intermediate 2048, 4 experts, top-2, vocab 2048
MOE_P12 = ModelConfig("moe-p12-test", "mixtral", 2, 2048, 16, 4, 128, 2048, 2048, 1000000.0, max_position=4096,
                      n_experts=4, top_k_experts=2)
PROMPT = [1, 17, 300, 45, 1999, 7, 7, 1024, 512, 3]
N_NEW = 32


def _engine(packed, graphs=True, max_batch=1):
    return Engine(MOE_P12, EngineConfig(device="cuda:0", max_context=512, seed=3, use_graphs=graphs,
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


def _check_twins(eng, with_o):
    assert eng.packed
    E, I, H = MOE_P12.n_experts, MOE_P12.intermediate, MOE_P12.hidden
    for L in eng.w.layers:
        assert isinstance(L.p_gu, wpack.PackedExperts12) and (L.p_gu.E, L.p_gu.rows, L.p_gu.K) == (E, 2 * I, H)
        assert isinstance(L.p_down, wpack.PackedExperts12) and (L.p_down.E, L.p_down.rows, L.p_down.K) == (E, H, I)
        assert isinstance(L.p_qkv, wpack.PackedWeight12) and not isinstance(L.p_qkv, wpack.PackedExperts12)
        assert (L.p_o is not None) == with_o
    assert isinstance(eng.w.p_lm_head, wpack.PackedWeight12)
    assert 0 < eng.w.packed_nbytes() <= eng.w.packed_demand(with_o) <= MOE_P12.packed_twin_bytes()
    assert eng.w.packed_nbytes() < 0.77 * eng.w.nbytes()  # 12/16 and the records, of all but the embedding and the router


@pytest.mark.parametrize("max_batch", [1, 2], ids=["one-row", "two-rows"])
@pytest.mark.parametrize("graphs", [True, False], ids=["graph", "eager"])
def test_packed12_moe_engine_tokens(cuda, monkeypatch, graphs, max_batch):
    two = max_batch == 2
    monkeypatch.delenv("LLMC_PACKED_FORMAT", raising=False)
    off = _engine("off", graphs, max_batch)
    assert not off.packed and off.w.layers[0].p_gu is None
    want = _tokens(off, two)
    del off
    on = _engine("on", graphs, max_batch)
    _check_twins(on, with_o=two or not all(on.ao_chunks))
    assert _tokens(on, two) == want


def test_auto_packs_a_moe_engine_and_three_rows_stay_bf16(cuda, monkeypatch):
    monkeypatch.delenv("LLMC_PACKED_FORMAT", raising=False)
    monkeypatch.delenv("LLMC_PACKED_WEIGHTS", raising=False)
    eng = _engine("auto")
    _check_twins(eng, with_o=not all(eng.ao_chunks))
    del eng
    three = _engine("on", max_batch=3)
    assert not three.packed and three.w.layers[0].p_gu is None and three.w.p_lm_head is None
