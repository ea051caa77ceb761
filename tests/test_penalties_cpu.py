"""Sampling penalties and min-p without a GPU: the float32 reference of penalty_ref.py checks
itself, oracle.sample with the new keywords equals it on every shared case, each case keeps within
the 2 % undecided cap, the wrong kernels the cases have to reject are rejected, and the public
interface (flags, server keys, validation, --model-sampling) carries the parameters to the engine."""

import json
from fractions import Fraction

import numpy as np
import pytest
import torch

import penalty_ref as pr
import sampler_ref as sr
from llm_consensus_amd import ops
from llm_consensus_amd.ops import oracle

SAMPLED = pr.all_sampled_cases()
IDS = [c.name for c in SAMPLED]


# -- the reference checks itself --------------------------------------------------------------------
def test_round_f32_is_round_to_nearest_even():
    """Against numpy's float64 -> float32 conversion (correctly rounded) on random doubles, exact
    ties, the subnormal range and the overflow threshold."""
    rs = np.random.RandomState(1)
    xs = list((rs.randn(2000) * 10.0 ** rs.randint(-45, 39, size=2000)))
    one = np.float32(1.0)
    ulp = float(np.nextafter(one, np.float32(2)) - one)
    xs += [1.0 + ulp / 2, 1.0 + 3 * ulp / 2, -(1.0 + ulp / 2), 2.0 ** -149 / 2, 2.0 ** -149 * 1.5, 2.0 ** -150 * 1.0001,
           float(np.finfo(np.float32).max), float(np.finfo(np.float32).max) * (1 + 2.0 ** -25), 2.0 ** 128, 2.0 ** -126]
    with np.errstate(over="ignore"):
        for x in xs:
            want, got = np.float32(x), pr.round_f32(Fraction(float(x)))
            assert pr.bits(want) == pr.bits(got), (x, want, got)


def test_fused_step_rounds_once():
    """fma(-0.2, c, l): against the oracle's float64 round-to-odd construction, and differing from the
    multiply rounded first somewhere (else the 'unfused' model would be no model at all)."""
    rs = np.random.RandomState(2)
    c = rs.randint(1, 32768, size=4000).astype(np.float32)
    l = (rs.randn(4000) * 5).astype(np.float32)
    f = np.float32(-0.2)
    want = np.array([pr.fma_f32(f, ci, li) for ci, li in zip(c, l)], dtype=np.float32)
    got = oracle.fma32(torch.full((4000,), float(f)), torch.from_numpy(c), torch.from_numpy(l)).numpy()
    assert np.array_equal(pr.bits(want), pr.bits(got))
    unfused = (l + (f * c).astype(np.float32)).astype(np.float32)
    assert (pr.bits(unfused) != pr.bits(want)).any()


def test_min_p_mask_rules():
    row = np.array([1.0, 3.0, 2.5, -np.inf, np.nan, 3.0], dtype=np.float32)
    assert pr.min_p_mask(row, 1.0, 0.0).all() and pr.min_p_mask(row, 0.0, 0.5).all()  # off; greedy
    assert pr.min_p_mask(row, 1.0, 0.5).tolist() == [False, True, True, False, False, True]  # ln 0.5 = -0.69
    assert pr.min_p_mask(row, 1.0, 1.0).tolist() == [False, True, False, False, False, True]  # the maximum only
    assert pr.min_p_mask(row, 0.5, 0.3).tolist() == [True, True, True, False, False, True]  # -2 * 0.5 >= ln 0.3
    inf = np.array([1.0, np.inf, 2.0], dtype=np.float32)  # inf - inf is NaN: the maximum survives all the same
    assert pr.min_p_mask(inf, 1.0, 0.1).tolist() == [False, True, False]


def test_words_of_the_shared_cases():
    for V, _ in pr.SHARED_VS:
        raw, w = pr.shared_raw(V)
        assert w[0] & pr.CTX and w[V - 1] & pr.CTX
        assert 295 <= int((w & pr.CTX != 0).sum()) <= 302
        c = (w & pr.COUNT).astype(int)
        assert 60 <= int((c > 0).sum()) <= 75 and int((c == pr.COUNT).sum()) == 1
        assert set(c[(c > 0) & (c < pr.COUNT)]) == {1, 2, 3, 4, 5}
        assert ((c > 0) & (w & pr.CTX == 0)).any() and ((c > 0) & (w & pr.CTX != 0)).any()
        # the penalties move the argmax
        assert int(np.argmax(pr.penalise(raw.numpy(), w, pr.R, pr.F, pr.P))) != int(raw.argmax())


# -- oracle == reference ----------------------------------------------------------------------------
def _oracle_run(pc, model="right", advance=True):
    it, tk, tp, seeds, pos, lmp, words, rep, freq, pres = pr.case_tensors(pc)
    logits = pc.raw.unsqueeze(0).repeat(pc.B, 1)
    toks, counted = oracle.sample(logits, it, tk, tp, seeds, pos, words=words, rep=rep, freq=freq, pres=pres,
                                  ln_min_p=lmp)
    return logits, toks.tolist(), counted


@pytest.mark.parametrize("pc", SAMPLED, ids=IDS)
def test_oracle_equals_reference(pc):
    """The penalised row written back is the reference's to the bit, the tokens obey the decided-row
    rule, and the returned words count each row's token once."""
    logits, toks, counted = _oracle_run(pc)
    want = pc.case.row.numpy()
    for b in range(pc.B):
        assert pr.same_bits(logits[b].numpy(), want).all(), b
    pr.check_tokens(pc, toks)
    for b in (0, pc.B // 2, pc.B - 1):
        assert np.array_equal(pr.words_array(counted[b]), pr.advance_words(pc.words, toks[b])), b


@pytest.mark.parametrize("pc", SAMPLED, ids=IDS)
def test_undecided_cap(pc):
    ex = pr.expectation(pc)
    share = sum(not e.decided for e in ex) / len(ex)
    assert share <= sr.UNDECIDED_CAP, (pc.name, share)


def test_min_p_winner_lies_outside_the_mask():
    """The min-p cases bite: on most rows the token picked WITHOUT the mask is one the mask drops."""
    for pc in pr.min_p_winner_cases():
        c = pc.case
        mask = pr.min_p_mask(c.row.numpy(), float(c.inv_temp[0]), float(pc.min_p[0]))
        assert 1 <= int(mask.sum()) <= 12
        ex = pr.expectation(pc)
        outside = 0
        for b in range(c.B):
            _, free, _ = sr.expected_tokens(c.row, float(c.inv_temp[b]), 0, 1.0, c.seeds[b], int(c.pos[b]))
            outside += not mask[free]
            assert mask[ex[b].tok]
        assert outside >= c.B // 2, (pc.name, outside)


# -- wrong kernels ----------------------------------------------------------------------------------
def _rejects(pc, toks) -> bool:
    try:
        pr.check_tokens(pc, toks)
    except AssertionError:
        return True
    return False


def _sample_plain(pc, prow, lmp=None):
    """oracle.sample over an already penalised row (no words)."""
    it, tk, tp, seeds, pos, lmp0, *_ = pr.case_tensors(pc)
    logits = torch.from_numpy(np.asarray(prow, dtype=np.float32)).unsqueeze(0).repeat(pc.B, 1)
    return oracle.sample(logits, it, tk, tp, seeds, pos, ln_min_p=lmp0 if lmp is None else lmp).tolist()


def test_unfused_multiply_subtract_differs():
    pc = pr.large_count_case()
    right = pc.case.row.numpy()
    wrong = pr.penalise(pc.raw.numpy(), pc.words, pc.r, pc.f, pc.p, model="unfused")
    assert (~pr.same_bits(right, wrong)).any()


@pytest.mark.parametrize("model", ["rep-on-generated-only", "presence-on-context", "div-mul-swapped"])
def test_wrong_transforms_are_rejected(model):
    """Each wrong transform changes bits of every shared row (the GPU bit-equality test sees that)
    and tokens of at least one shared case (the sampling test sees that)."""
    rejected = 0
    for pc in pr.shared_cases()[:len(pr.PARAM_SETS)]:  # V = 1500
        wrong = pr.penalise(pc.raw.numpy(), pc.words, pc.r, pc.f, pc.p, model=model)
        assert (~pr.same_bits(pc.case.row.numpy(), wrong)).any(), pc.name
        rejected += _rejects(pc, _sample_plain(pc, wrong))
    assert rejected >= 1


def test_min_p_before_top_p_is_rejected():
    """min-p first shrinks the mass top-p works on, so top-p then cuts earlier."""
    pc = pr.shared_cases()[pr.MINP_ORDER_SET]
    c = pc.case
    assert float(c.top_p[0]) < 1 and float(pc.min_p[0]) > 0
    prow = c.row.numpy().copy()
    prow[~pr.min_p_mask(prow, float(c.inv_temp[0]), float(pc.min_p[0]))] = -np.inf
    off = torch.full((pc.B,), float("-inf"))
    assert _rejects(pc, _sample_plain(pc, prow, lmp=off))
    assert not _rejects(pc, _sample_plain(pc, c.row.numpy()))


# -- chained calls: the count --------------------------------------------------------------------------
def test_chained_calls_count_on_the_cpu():
    pr.check_chain(pr.chain_run("cpu"))


def test_bare_call_leaves_the_words_alone_on_the_cpu():
    pc = pr.shared_cases()[0]
    it, tk, tp, seeds, pos, lmp, words, rep, freq, pres = pr.case_tensors(pc)
    before = words.clone()
    nxt = torch.zeros(pc.B, dtype=torch.int32)
    ops.sample(pc.raw.unsqueeze(0).repeat(pc.B, 1), it, tk, tp, seeds, pos, nxt, words=words, rep=rep, freq=freq,
               pres=pres)
    assert torch.equal(words, before)


def test_count_not_advanced_is_noticed():
    """A kernel that never counts leaves the words of call 1 for call 2: check_chain fails on it."""
    out = pr.chain_run("cpu")
    frozen = [(t, out[0][1] if i else w, l, p) for i, (t, w, l, p) in enumerate(out)]
    frozen[0] = (out[0][0], pr.chain_inputs()[1], out[0][2], out[0][3])
    with pytest.raises(AssertionError):
        pr.check_chain(frozen)


# -- neutral parameters -------------------------------------------------------------------------------
def test_neutral_parameters_leave_every_bit():
    pc = pr.shared_cases()[0]
    it, tk, tp, seeds, pos, lmp, words, rep, freq, pres = pr.case_tensors(pc)
    raw = pc.raw.clone()
    raw[5], raw[6], raw[7] = float("nan"), -0.0, float("inf")
    logits = raw.unsqueeze(0).repeat(pc.B, 1)
    one, zero = torch.ones(pc.B), torch.zeros(pc.B)
    toks, _ = oracle.sample(logits, it, tk, tp, seeds, pos, words=words, rep=one, freq=zero, pres=zero)
    assert np.array_equal(pr.bits(logits.numpy()), np.tile(pr.bits(raw.numpy()), (pc.B, 1)))
    assert toks.tolist() == oracle.sample(raw.unsqueeze(0).repeat(pc.B, 1), it, tk, tp, seeds, pos).tolist()
    assert np.array_equal(pr.bits(pr.penalise(raw.numpy(), pc.words, 1.0, 0.0, 0.0)), pr.bits(raw.numpy()))


def test_penalty_seed_on_the_cpu():
    V = 50
    buf = torch.full((3, V), 7, dtype=torch.int16)
    buf[1].zero_()
    ops.penalty_seed(buf[1], torch.tensor([3, 3, -1, V, 0, V - 1, 1 << 20], dtype=torch.int32))
    want = np.zeros(V, dtype=np.uint16)
    want[[0, 3, V - 1]] = pr.CTX
    assert np.array_equal(pr.words_array(buf[1]), want)
    assert (buf[0] == 7).all() and (buf[2] == 7).all()


# -- public interface ---------------------------------------------------------------------------------
def _parse(argv):
    import io

    from llm_consensus_amd import cli

    err = io.StringIO()
    return cli.parse_flags(argv, stdout=io.StringIO(), stderr=err), err


def test_cli_flags_reach_the_request_template():
    from llm_consensus_amd import cli

    cfg, _ = _parse(["--models", "stub-a", "--min-p", "0.05", "--repetition-penalty", "1.05", "--presence-penalty=0.5",
                     "--frequency-penalty", "-0.25", "--model-sampling", "hi"])
    assert (cfg.min_p, cfg.repetition_penalty, cfg.presence_penalty, cfg.frequency_penalty) == (0.05, 1.05, 0.5, -0.25)
    assert cfg.model_sampling is True and cfg.prompt == "hi"
    t = cli._request_template(cfg)
    assert (t.min_p, t.repetition_penalty, t.presence_penalty, t.frequency_penalty) == (0.05, 1.05, 0.5, -0.25)
    cfg, _ = _parse(["--models", "stub-a", "hi"])
    assert (cfg.min_p, cfg.repetition_penalty, cfg.presence_penalty, cfg.frequency_penalty) == (0.0, 1.0, 0.0, 0.0)
    assert cfg.model_sampling is False


@pytest.mark.parametrize("flag,value", [("min-p", "1.5"), ("min-p", "-0.1"), ("min-p", "nan"),
                                        ("repetition-penalty", "0"), ("repetition-penalty", "-1"),
                                        ("repetition-penalty", "inf"), ("presence-penalty", "nan"),
                                        ("frequency-penalty", "-inf")])
def test_cli_rejects_bad_values_like_a_bad_flag(flag, value):
    """Error line, usage, exit 2: before any engine starts (llama-tiny is never resolved)."""
    import io

    from llm_consensus_amd import cli

    err = io.StringIO()
    with pytest.raises(SystemExit) as ex:
        cli.parse_flags(["--models", "llama-tiny", f"--{flag}={value}", "hi"], stdout=io.StringIO(), stderr=err)
    assert ex.value.code == 2
    text = err.getvalue()
    assert text.startswith(f'invalid value "') and f"for flag -{flag}: " in text.splitlines()[0]
    assert "Usage of llm-consensus:" in text


def test_check_sampling():
    from llm_consensus_amd.provider.base import check_sampling

    check_sampling()
    check_sampling(min_p=0.0, repetition_penalty=1e-3, presence_penalty=-2.0, frequency_penalty=2.0)
    check_sampling(min_p=1.0)
    for bad in (dict(min_p=1.0001), dict(min_p=float("nan")), dict(repetition_penalty=0.0),
                dict(repetition_penalty=float("inf")), dict(presence_penalty=float("inf")),
                dict(frequency_penalty=float("nan")), dict(min_p="0.1"), dict(presence_penalty=True)):
        with pytest.raises(ValueError) as ex:
            check_sampling(**bad)
        assert str(ex.value).startswith(next(iter(bad)) + ": ")


@pytest.fixture
def stub_service():
    from llm_consensus_amd.server import ConsensusService

    svc = ConsensusService(["stub-a"], "stub-j", concurrency=1, min_p=0.02, repetition_penalty=1.1)
    yield svc
    svc.close()


def test_server_keys_and_defaults(stub_service):
    from llm_consensus_amd.server import BadRequest

    svc = stub_service
    req = svc.parse({"prompt": "hi"})
    assert (req["min_p"], req["repetition_penalty"], req["presence_penalty"], req["frequency_penalty"]) == \
        (0.02, 1.1, 0.0, 0.0)
    req = svc.parse({"prompt": "hi", "min_p": 0, "repetition_penalty": 1, "presence_penalty": 0.5,
                     "frequency_penalty": 0.25})
    assert (req["min_p"], req["repetition_penalty"], req["presence_penalty"], req["frequency_penalty"]) == \
        (0.0, 1.0, 0.5, 0.25)
    for body in ({"min_p": 2}, {"min_p": -0.5}, {"repetition_penalty": 0}, {"repetition_penalty": "x"},
                 {"presence_penalty": float("inf")}, {"frequency_penalty": float("nan")}, {"min_p": [0.1]}):
        with pytest.raises(BadRequest) as ex:
            svc.parse({"prompt": "hi", **body})
        assert str(ex.value).startswith(next(iter(body)) + ": ")


def test_server_answers_400(stub_service):
    import threading
    import urllib.error
    import urllib.request

    from llm_consensus_amd.server import ConsensusServer

    srv = ConsensusServer(("127.0.0.1", 0), stub_service)
    t = threading.Thread(target=srv.serve_forever, kwargs={"poll_interval": 0.05}, daemon=True)
    t.start()
    try:
        url = f"http://127.0.0.1:{srv.server_address[1]}/v1/consensus"
        for body, code in (({"prompt": "hi", "repetition_penalty": -1}, 400), ({"prompt": "hi", "min_p": 0.5}, 200)):
            rq = urllib.request.Request(url, data=json.dumps(body).encode(), headers={"Content-Type": "application/json"})
            try:
                with urllib.request.urlopen(rq, timeout=60) as r:
                    got, text = r.status, r.read().decode()
            except urllib.error.HTTPError as e:
                got, text = e.code, e.read().decode()
            assert got == code, text
            if code == 400:
                assert json.loads(text)["error"].startswith("repetition_penalty: ")
    finally:
        srv.shutdown()
        srv.server_close()


def test_server_rejects_bad_startup_defaults():
    from llm_consensus_amd.server import ConsensusService

    with pytest.raises(ValueError):
        ConsensusService(["stub-a"], "stub-j", repetition_penalty=0.0)


def _tiny_checkpoint(tmp_path, gen):
    """config.json + generation_config.json of a tiny Qwen2-shaped checkpoint (no weights: only the
    configuration is read here)."""
    d = tmp_path / "qwen-tiny-ckpt"
    d.mkdir()
    (d / "config.json").write_text(json.dumps({
        "model_type": "qwen2", "hidden_size": 128, "num_attention_heads": 4, "num_key_value_heads": 2,
        "num_hidden_layers": 2, "intermediate_size": 256, "vocab_size": 512, "max_position_embeddings": 1024,
        "rms_norm_eps": 1e-6, "rope_theta": 1000000.0, "eos_token_id": 3}))
    if gen is not None:
        (d / "generation_config.json").write_text(json.dumps(gen))
    return str(d)


def test_checkpoint_reads_generation_config(tmp_path):
    from llm_consensus_amd.models.checkpoint import CheckpointError, config_from_hf
    from llm_consensus_amd.models.config import SamplingDefaults

    cfg = config_from_hf(_tiny_checkpoint(tmp_path, {"eos_token_id": [3, 4], "repetition_penalty": 1.05,
                                                     "temperature": 0.7, "top_k": 20, "top_p": 0.8, "do_sample": True}))
    assert cfg.eos_ids == (3, 4)
    assert cfg.sampling == SamplingDefaults(temperature=0.7, top_k=20, top_p=0.8, min_p=0.0, repetition_penalty=1.05)
    (tmp_path / "a").mkdir()
    assert config_from_hf(_tiny_checkpoint(tmp_path / "a", {"eos_token_id": 3})).sampling is None
    (tmp_path / "b").mkdir()
    assert config_from_hf(_tiny_checkpoint(tmp_path / "b", None)).sampling is None
    (tmp_path / "c").mkdir()
    with pytest.raises(CheckpointError):
        config_from_hf(_tiny_checkpoint(tmp_path / "c", {"min_p": "lots"}))


def test_model_sampling_precedence(tmp_path):
    """Without the flag nothing changes; with it the checkpoint's values fill the knobs the request
    left neutral and never override one it set."""
    from llm_consensus_amd.engine.engine import SamplingParams
    from llm_consensus_amd.models.checkpoint import config_from_hf
    from llm_consensus_amd.models.config import FAMILIES
    from llm_consensus_amd.provider.base import Request
    from llm_consensus_amd.provider.local import sampling_form, sampling_knobs

    cfg = config_from_hf(_tiny_checkpoint(tmp_path, {"repetition_penalty": 1.05, "temperature": 0.7, "top_k": 20,
                                                     "top_p": 0.8, "min_p": 0.01}))
    neutral = dict(temperature=1.0, top_p=1.0, top_k=0, min_p=0.0, repetition_penalty=1.0, presence_penalty=0.0,
                   frequency_penalty=0.0)
    bare = Request(model="m", prompt="p")
    assert sampling_knobs(bare, cfg, False) == neutral
    assert sampling_form(bare, cfg, False) == (False, False)
    own = dict(neutral, temperature=0.7, top_k=20, top_p=0.8, min_p=0.01, repetition_penalty=1.05)
    assert sampling_knobs(bare, cfg, True) == own
    assert sampling_form(bare, cfg, True) == (True, True)
    # neutral values given explicitly count as left neutral; set ones win
    req = Request(model="m", prompt="p", temperature=1.0, top_k=0, top_p=0.95, repetition_penalty=1.2,
                  presence_penalty=0.5)
    assert sampling_knobs(req, cfg, True) == dict(own, top_p=0.95, repetition_penalty=1.2, presence_penalty=0.5)
    assert sampling_knobs(req, cfg, False) == dict(neutral, top_p=0.95, repetition_penalty=1.2, presence_penalty=0.5)
    # a catalog family has no values of its own: the flag changes nothing
    assert sampling_knobs(bare, FAMILIES["llama-tiny"], True) == neutral
    assert sampling_form(Request(model="m", prompt="p", min_p=0.1), FAMILIES["llama-tiny"], False) == (True, False)
    # what the provider sends is what SamplingParams takes
    p = SamplingParams(max_tokens=4, seed=1, stop_on_eos=True, **sampling_knobs(req, cfg, True))
    assert p.penalised and p.topkp and p.repetition_penalty == 1.2


def test_sampling_form_is_the_params_own_predicates(tmp_path):
    """The provider's (top-k/top-p launch, penalty launch) pair restates nothing: over the request and
    config cases above it is what SamplingParams says of the same knobs."""
    from llm_consensus_amd.engine.engine import SamplingParams
    from llm_consensus_amd.models.checkpoint import config_from_hf
    from llm_consensus_amd.models.config import FAMILIES
    from llm_consensus_amd.provider.base import Request
    from llm_consensus_amd.provider.local import sampling_form, sampling_knobs

    cfg = config_from_hf(_tiny_checkpoint(tmp_path, {"repetition_penalty": 1.05, "temperature": 0.7, "top_k": 20,
                                                     "top_p": 0.8, "min_p": 0.01}))
    bare = Request(model="m", prompt="p")
    req = Request(model="m", prompt="p", temperature=1.0, top_k=0, top_p=0.95, repetition_penalty=1.2,
                  presence_penalty=0.5)
    cases = [(bare, cfg, False), (bare, cfg, True), (req, cfg, True), (req, cfg, False),
             (bare, FAMILIES["llama-tiny"], True), (Request(model="m", prompt="p", min_p=0.1), FAMILIES["llama-tiny"], False),
             (None, None, False)]
    seen = set()
    for r, c, ms in cases:
        p = SamplingParams(**sampling_knobs(r, c, ms))
        assert sampling_form(r, c, ms) == (p.topkp, p.penalised) == tuple(p.form[:2])
        seen.add(sampling_form(r, c, ms))
    assert seen == {(False, False), (True, False), (True, True)}


# -- engine -------------------------------------------------------------------------------------------
def _tiny_engine(**kw):
    from llm_consensus_amd.engine.engine import Engine, EngineConfig
    from llm_consensus_amd.models.config import FAMILIES

    return Engine(FAMILIES["llama-tiny"], EngineConfig(device="cpu", max_context=256, use_graphs=False, seed=5, **kw))


PROMPT = list(range(300, 320))


def test_engine_neutral_decode_never_allocates_the_table():
    eng = _tiny_engine()
    a = eng.generate_ids(PROMPT, 16, temperature=0.0, stop_on_eos=False)
    b = eng.generate_ids(PROMPT, 16, temperature=0.0, stop_on_eos=False, min_p=0.1)  # greedy: min-p does nothing
    assert eng.pen_words is None and a == b
    eng.generate_ids(PROMPT, 4, temperature=0.0, stop_on_eos=False, presence_penalty=0.5)
    assert eng.pen_words is not None and eng.pen_words.shape == (1, eng.cfg.vocab)
    assert eng.generate_ids(PROMPT, 16, temperature=0.0, stop_on_eos=False) == a


def test_engine_second_decode_counts_the_first_as_context():
    """A sequence bound again: everything it holds is context (bit 15), counts start at 0, and the
    first token of the second decode is penalised already."""
    from llm_consensus_amd.engine.engine import SamplingParams

    eng = _tiny_engine()
    seq = eng.new_sequence()
    eng.prefill([seq], [PROMPT])
    sp = SamplingParams(6, 0.0, 1.0, 0, 0, False, repetition_penalty=1.3, frequency_penalty=0.2, presence_penalty=0.5)
    first = eng.decode([seq], [sp])[0]
    assert seq.ids == PROMPT + first and seq.length == len(seq.ids)
    w = pr.words_array(eng.pen_words[0])
    assert set(np.flatnonzero(w & pr.CTX)) == set(PROMPT)
    gen = np.zeros(eng.cfg.vocab, dtype=int)
    for t in first:
        gen[t] += 1
    assert np.array_equal((w & pr.COUNT).astype(int), gen)
    eng.prefill([seq], [[7, 8, 9]])
    second = eng.decode([seq], [sp])[0]
    w = pr.words_array(eng.pen_words[0])
    assert set(np.flatnonzero(w & pr.CTX)) == set(PROMPT + first + [7, 8, 9])
    gen = np.zeros(eng.cfg.vocab, dtype=int)
    for t in second:
        gen[t] += 1
    assert np.array_equal((w & pr.COUNT).astype(int), gen)
    eng.free_sequence(seq)


def test_engine_steps_obey_the_reference():
    """Every token of a penalised decode against the reference applied to that step's raw logits and
    the running history (the eager debug path returns the raw rows)."""
    from llm_consensus_amd.engine.engine import SamplingParams

    eng = _tiny_engine()
    sp = SamplingParams(12, 1.0, 1.0, 40, 11, False, min_p=0.02, repetition_penalty=1.3, presence_penalty=0.5,
                        frequency_penalty=0.2)
    toks, lg = eng.debug_decode_logits_batch([PROMPT], 12, params=[sp])
    assert toks[0] == eng.generate_ids(PROMPT, 12, temperature=1.0, top_k=40, seed=11, stop_on_eos=False, min_p=0.02,
                                       repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.2)
    pr.check_steps(toks[0], lg[0].numpy(), PROMPT, sp)


def test_batcher_rows_keep_their_solo_tokens():
    """Neutral, penalised and differently penalised requests admitted at different steps, one
    retiring early so a row moves down: each yields the tokens of its solo run."""
    from llm_consensus_amd.engine.batcher import ContinuousBatcher
    from llm_consensus_amd.engine.engine import SamplingParams

    eng = _tiny_engine(max_batch=3, steps_per_graph=4)
    reqs = pr.batcher_requests(SamplingParams)
    solo = [eng.generate_batch([p], [sp])[0] for p, sp in reqs]
    assert pr.run_staggered(eng, reqs, ContinuousBatcher) == solo


# -- CPU worker, end to end ---------------------------------------------------------------------------
def test_worker_presence_penalty_never_repeats(monkeypatch):
    """LLMC_DEVICE=cpu worker, llama-tiny, greedy: with presence_penalty = 1e4 no id comes twice in
    64 tokens; the same run without it repeats (so the property is not vacuous)."""
    from llm_consensus_amd.catalog import resolve
    from llm_consensus_amd.context import Context
    from llm_consensus_amd.provider.base import Request
    from llm_consensus_amd.provider.local import LocalBackend

    monkeypatch.setenv("LLMC_DEVICE", "cpu")
    be = LocalBackend([resolve("llama-tiny@pen")], max_context={"llama-tiny@pen": 512})
    try:
        prov = be.provider("llama-tiny@pen")
        seen = []
        deliver = be._deliver

        def tap(msg):
            if msg[0] == "tokens":
                seen.extend(msg[2])
            deliver(msg)

        be._deliver = tap
        out = []
        for pp in (None, 1e4):
            seen.clear()
            r = prov.query(Context.background(), Request(model="llama-tiny@pen", prompt="tell me about loops",
                                                         max_tokens=64, temperature=0.0, stop_on_eos=False,
                                                         presence_penalty=pp))
            assert r.output_tokens == 64 == len(seen)
            out.append(list(seen))
        assert len(set(out[0])) < 64
        assert len(set(out[1])) == 64
    finally:
        be.close()


@pytest.mark.parametrize("B", pr.BIT_BS)
@pytest.mark.parametrize("V", pr.BIT_VS)
def test_oracle_penalize_on_the_bit_equality_inputs(V, B):
    """The inputs of the GPU bit-equality test (0.0, -0.0, +-inf, NaN, a count of 32767, a neutral
    row) through the CPU path of ops.penalize_logits."""
    logits, words, rep, freq, pres = pr.bit_inputs(V, B)
    got = torch.from_numpy(logits.copy())
    ops.penalize_logits(got, torch.stack([pr.words_tensor(words[b]) for b in range(B)]), torch.from_numpy(rep),
                        torch.from_numpy(freq), torch.from_numpy(pres))
    for b in range(B):
        assert pr.same_bits(got[b].numpy(), pr.penalise(logits[b], words[b], rep[b], freq[b], pres[b])).all(), b
    if B == 3:
        assert np.array_equal(pr.bits(got[1].numpy()), pr.bits(logits[1]))
