"""Decode graphs are keyed by ``GraphKey(rows, bucket, form)``: a warm-up captures exactly the keys of
its form, and a decode in that form finds them."""

from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu

PROMPT = list(range(300, 320))


def test_warmup_captures_the_keys_decode_looks_up(cuda):
    from llm_consensus_amd.engine import Engine, EngineConfig, GraphKey, SamplingForm
    from llm_consensus_amd.models.config import FAMILIES
    from llm_consensus_amd.models.transformer import TransformerWeights
    from llm_consensus_amd.parallel.comm import TPGroup

    cfg = FAMILIES["llama-tiny"]
    w = TransformerWeights(cfg, TPGroup.single(), torch.device("cuda:0"), 5, 1.0)
    eg, ee = (Engine(cfg, EngineConfig(device="cuda:0", max_context=512, use_graphs=g), weights=w) for g in (True, False))
    forms = {SamplingForm(): dict(temperature=0.0),
             SamplingForm(True, True, True): dict(temperature=1.0, top_k=40, seed=11, repetition_penalty=1.3,
                                                  presence_penalty=0.5, logprobs=3)}
    for f in forms:
        assert eg.warmup_graphs([1], f) == len(eg.buckets())
    keys = {GraphKey(1, b, f) for b in eg.buckets() for f in forms}
    assert set(eg._graphs) == keys and not eg.capture_on_demand  # nothing below may capture
    for f, kw in forms.items():
        got = eg.generate_ids(PROMPT, 20, stop_on_eos=False, **kw)
        want = ee.generate_ids(PROMPT, 20, stop_on_eos=False, **kw)
        assert set(eg._graphs) == keys and not ee._graphs
        assert list(got) == list(want) and len(got) == 20
        assert (got.logprobs is not None) == f.logprobs
