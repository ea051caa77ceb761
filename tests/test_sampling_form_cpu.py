"""SamplingForm: the one value that says which launches a decode step issues around the sampler, and
the engine's ownership of its per-row sampling state (``row_state`` / ``move_row``)."""

from __future__ import annotations

import pytest
import torch

from llm_consensus_amd.engine import Engine, EngineConfig, GraphKey, SamplingForm, SamplingParams
from llm_consensus_amd.engine.batcher import ContinuousBatcher
from llm_consensus_amd.models.config import FAMILIES

F = SamplingForm
PEN = dict(repetition_penalty=1.3, presence_penalty=0.5)
FORM_CASES = [({}, F()),
              (dict(top_k=40), F(topkp=True)),
              (dict(top_p=0.9), F(topkp=True)),
              (dict(min_p=0.05), F(topkp=True)),
              (dict(repetition_penalty=1.2), F(penalties=True)),
              (dict(presence_penalty=0.5), F(penalties=True)),
              (dict(frequency_penalty=0.2), F(penalties=True)),
              (dict(logprobs=0), F(logprobs=True)),
              (dict(top_k=40, frequency_penalty=0.2, logprobs=3), F(True, True, True))]


@pytest.mark.parametrize("kw,want", FORM_CASES, ids=[",".join(kw) or "neutral" for kw, _ in FORM_CASES])
def test_params_form(kw, want):
    p = SamplingParams(**kw)
    assert p.form == want == (p.topkp, p.penalised, p.logprobs is not None)
    assert SamplingForm.of([p]) == want and SamplingForm.of([SamplingParams(), p, SamplingParams()]) == want


def test_form_is_a_hashable_value_and_of_is_the_fieldwise_any():
    assert F() == F(False, False, False) == SamplingForm.of([]) == SamplingForm.of(iter(()))
    singles = [SamplingParams(top_p=0.5), SamplingParams(presence_penalty=1.0), SamplingParams(logprobs=0)]
    assert SamplingForm.of(singles[:2]) == F(True, True, False)
    assert SamplingForm.of(p for p in singles) == F(True, True, True)  # any iterable, read once
    with pytest.raises(AttributeError):
        F().topkp = True
    key = GraphKey(1, 0, F(penalties=True))
    assert {key: 1}[GraphKey(rows=1, bucket=0, form=F(False, True, False))] == 1 and len(key) == len(GraphKey(2, 1, F()))


def _tiny_engine(**kw):
    return Engine(FAMILIES["llama-tiny"], EngineConfig(device="cpu", max_context=256, use_graphs=False, seed=5, **kw))


PROMPT = list(range(300, 320))


def test_a_decode_does_not_inherit_the_previous_form():
    """A penalised top-k decode with logprobs, then a greedy default decode and ``debug_decode_layers``
    on the same engine: the tokens and hidden states of a fresh engine, bit for bit."""
    fresh, used = _tiny_engine(), _tiny_engine()
    hot = used.generate_ids(PROMPT, 12, temperature=1.0, top_k=40, seed=3, stop_on_eos=False, logprobs=3, **PEN)
    assert len(hot) == 12 == len(hot.logprobs) and used.pen_words is not None and used.lp_raw is not None
    want = fresh.generate_ids(PROMPT, 12, temperature=0.0, stop_on_eos=False)
    got = used.generate_ids(PROMPT, 12, temperature=0.0, stop_on_eos=False)
    assert list(got) == list(want) and got.logprobs is None
    (hs, pos), (whs, wpos) = used.debug_decode_layers(PROMPT), fresh.debug_decode_layers(PROMPT)
    assert pos == wpos and torch.equal(hs, whs)
    assert fresh.pen_words is None and fresh.lp_tok is None and fresh.lp_raw is None


def test_moved_rows_keep_their_sampling_state():
    """A plain row, a penalised row with logprobs and a sampled row of different lengths: the first
    retires early, the rows behind it move down (``Engine.move_row``), and each keeps the tokens and
    the entries of its solo run. The engine's ``row_state`` then lists the penalty buffers too."""
    eng = _tiny_engine(max_batch=3, steps_per_graph=4)
    assert len(eng.row_state()) == 13
    reqs = [([300 + i for i in range(12)], SamplingParams(max_tokens=6, temperature=0.0, stop_on_eos=False)),
            ([400 + i for i in range(7)], SamplingParams(max_tokens=22, temperature=0.0, stop_on_eos=False, logprobs=20,
                                                         **PEN)),
            ([500 + i for i in range(9)], SamplingParams(max_tokens=18, temperature=0.9, top_k=40, seed=7,
                                                         stop_on_eos=False))]
    solo = [eng.generate_batch([p], [sp]) for p, sp in reqs]
    bat, rows, moved = ContinuousBatcher(eng), [], []
    move_row = eng.move_row
    eng.move_row = lambda dst, src, lp_cols=None: (moved.append((dst, src, lp_cols)), move_row(dst, src, lp_cols))
    for k, (prompt, sp) in enumerate(reqs):
        seq = eng.new_sequence()
        eng.prefill([seq], [prompt])
        rows.append(bat.admit(seq, sp, tag=k))
    bat.drain()
    # rows 1 and 2 moved down once row 0 retired; only the row with logprobs names ring columns (an
    # empty range here: the CPU path consumes every column before it compacts)
    assert [(d, s, c is None) for d, s, c in moved] == [(0, 1, False), (1, 2, True)]
    for k, r in enumerate(rows):
        assert r.error is None and r.tokens == list(solo[k][0]), k
        want = solo[k].logprobs[0]
        if want is None:
            assert r.logprobs is None
            continue
        assert len(r.logprobs) == len(r.tokens) == len(want)
        # The CPU oracle's bf16 matmuls are not batch-invariant (a row's logits move by about 1e-2 with the
        # rows beside it: tests/test_logprobs_cpu.py), so the values get that test's bound; a row that
        # picked up another row's columns, or lost its own in the move, would be off by nats. The GPU
        # batcher tests compare the bits.
        for (lp, top), (wlp, wtop) in zip(r.logprobs, want):
            assert len(top) == len(wtop) == 20 and abs(lp - wlp) < 0.05
            assert all(abs(a[1] - b[1]) < 0.05 for a, b in zip(top, wtop))
    state = eng.row_state()
    assert len(state) == 17 and any(t is eng.pen_words for t in state)
    assert all(t.shape[0] == eng.ecfg.max_batch for t in state)
