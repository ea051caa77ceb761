"""Sampling penalties and min-p on the GPU (csrc/kernels/sampler.hip): penalize_logits alone is
bit-equal to the float32 reference of penalty_ref.py, penalty_seed marks only what it may, sampling
through both launches obeys the decided-row rule on the shared cases (test_penalties_cpu.py shows
their undecided cap and which wrong kernels they reject), the state advance counts on the device,
and the engine keeps all of it through graph decode, the batcher and tensor parallelism."""

import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import penalty_ref as pr
import sampler_ref as sr
from llm_consensus_amd import ops

pytestmark = pytest.mark.gpu


# -- penalize_logits alone ------------------------------------------------------------------------------
def _penalize(logits, words, rep, freq, pres, pad=0):
    """One launch over a [B, V] view of a [B, V + pad] buffer; returns (result, padding)."""
    B, V = logits.shape
    buf = torch.full((B, V + pad), 123.0, device="cuda")
    buf[:, :V] = torch.from_numpy(logits).cuda()
    wbuf = torch.full((B, V + pad), -1, dtype=torch.int16, device="cuda")
    wbuf[:, :V] = torch.stack([pr.words_tensor(words[b]) for b in range(B)]).cuda()
    view = buf[:, :V]
    ops.penalize_logits(view, wbuf[:, :V], torch.from_numpy(rep).cuda(), torch.from_numpy(freq).cuda(),
                        torch.from_numpy(pres).cuda())
    torch.cuda.synchronize()
    return view.cpu().numpy(), buf[:, V:].cpu().numpy()


@pytest.mark.parametrize("B", pr.BIT_BS)
@pytest.mark.parametrize("V", pr.BIT_VS)
def test_penalize_logits_bit_equal(cuda, V, B):
    """V around the 64 parts and the 256-thread stride, ids 0 and V - 1 touched, 0.0 / -0.0 / +-inf /
    NaN among the seen ids, a count of 32767, and (B = 3) a neutral row between two penalised ones."""
    logits, words, rep, freq, pres = pr.bit_inputs(V, B)
    assert all(words[b, 0] and words[b, V - 1] for b in range(B))
    if V > 100:
        assert ((words & pr.COUNT) == pr.COUNT).any()
        assert np.isnan(logits[words != 0]).any() and np.isinf(logits[words != 0]).any()
    got, _ = _penalize(logits, words, rep, freq, pres)
    for b in range(B):
        want = pr.penalise(logits[b], words[b], rep[b], freq[b], pres[b])
        bad = np.flatnonzero(~pr.same_bits(got[b], want))
        assert bad.size == 0, (b, bad[:5], got[b][bad[:5]], want[bad[:5]], words[b][bad[:5]])
        if B == 3 and b == 1:  # the neutral row keeps every bit although its words are set
            assert np.array_equal(pr.bits(got[b]), pr.bits(logits[b]))
        else:
            assert V == 1 or (~pr.same_bits(got[b], logits[b])).any()


def test_penalize_logits_strided(cuda):
    """A [B, V] view of a wider buffer (logits and words): the padding comes back intact."""
    logits, words, rep, freq, pres = pr.bit_inputs(1025, 3)
    got, padding = _penalize(logits, words, rep, freq, pres, pad=37)
    for b in range(3):
        assert pr.same_bits(got[b], pr.penalise(logits[b], words[b], rep[b], freq[b], pres[b])).all(), b
    assert (padding == 123.0).all()


def test_penalize_logits_large_counts_are_fused(cuda):
    """The case on which a multiply rounded before the subtraction differs from the fused form."""
    pc = pr.large_count_case()
    one = lambda v: np.array([v], dtype=np.float32)  # noqa: E731
    got, _ = _penalize(pc.raw.numpy()[None], pc.words[None], one(pc.r), one(pc.f), one(pc.p))
    assert pr.same_bits(got[0], pc.case.row.numpy()).all()
    assert (~pr.same_bits(got[0], pr.penalise(pc.raw.numpy(), pc.words, pc.r, pc.f, pc.p, model="unfused"))).any()


# -- penalty_seed ---------------------------------------------------------------------------------------
def test_penalty_seed_marks_only_its_row(cuda):
    """Duplicates are benign, ids -1 and V (and far outside) are skipped, and the row is a slice of a
    sentinel-filled buffer whose surroundings come back intact."""
    V, sentinel = 1000, 0x1234
    buf = torch.full((3, V + 16), sentinel, dtype=torch.int16, device="cuda")
    row = buf[1, 8:8 + V]
    row.zero_()
    ids = [0, V - 1, 5, 5, 5, -1, V, V + 3, -(1 << 31), (1 << 31) - 1, 700] + list(range(100, 400)) + [5] * 300
    ops.penalty_seed(row, torch.tensor(ids, dtype=torch.int32, device="cuda"))
    ops.penalty_seed(row, torch.empty(0, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    want = np.zeros(V, dtype=np.uint16)
    want[[i for i in ids if 0 <= i < V]] = pr.CTX
    assert np.array_equal(pr.words_array(row), want)
    out = buf.cpu()
    assert (out[0] == sentinel).all() and (out[2] == sentinel).all()
    assert (out[1, :8] == sentinel).all() and (out[1, 8 + V:] == sentinel).all()


# -- sampling through both launches -----------------------------------------------------------------------
SAMPLED = pr.all_sampled_cases()


def _sample(pc, topkp):
    it, tk, tp, seeds, pos, lmp, words, rep, freq, pres = pr.case_tensors(pc, "cuda")
    logits = pc.raw.cuda().unsqueeze(0).repeat(pc.B, 1)
    P = ops.sample_parts()
    wv, wi = torch.empty(pc.B, P, device="cuda"), torch.empty(pc.B, P, dtype=torch.int32, device="cuda")
    nxt = torch.full((pc.B,), -1, dtype=torch.int32, device="cuda")
    before = words.clone()
    ops.sample(logits, it, tk, tp, seeds, pos, nxt, wv, wi, use_topkp=topkp, words=words, rep=rep, freq=freq,
               pres=pres, ln_min_p=lmp)
    toks = nxt.cpu().tolist()
    assert torch.equal(words, before), "a bare call changed the history words"
    assert pos.cpu().tolist() == pc.case.pos.tolist(), "a bare call moved the position"
    return toks, logits.cpu().numpy()


@pytest.mark.parametrize("pc", SAMPLED, ids=[c.name for c in SAMPLED])
def test_sampling_shared_cases(cuda, pc):
    """penalize_logits, then the sampler: the penalised rows are the reference's bits and every token
    obeys the decided-row rule. Cases without top-k, top-p or min-p go through the two-stage launch too."""
    toks, plog = _sample(pc, True)
    assert pr.same_bits(plog, np.tile(pc.case.row.numpy(), (pc.B, 1))).all()
    pr.check_tokens(pc, toks)
    c = pc.case
    if not (c.top_k > 0).any() and not (c.top_p < 1).any() and not (pc.min_p > 0).any():
        pr.check_tokens(pc, _sample(pc, False)[0])


def test_min_p_drops_the_unmasked_winner(cuda):
    for pc in pr.min_p_winner_cases():
        toks, _ = _sample(pc, True)
        pr.check_tokens(pc, toks)
        mask = pr.min_p_mask(pc.case.row.numpy(), float(pc.case.inv_temp[0]), float(pc.min_p[0]))
        assert all(mask[t] for t in toks)


def test_min_p_off_is_the_launch_without_it(cuda):
    """ln_min_p of -inf, and no array at all: the tokens of today's launch."""
    case = sr.mixed_batch_case()
    it, tk, tp, seeds, pos = sr.case_tensors(case, "cuda")
    logits = case.row.cuda().unsqueeze(0).expand(case.B, case.V).contiguous()
    out = []
    for lmp in (None, torch.full((case.B,), float("-inf"), device="cuda")):
        nxt = torch.full((case.B,), -1, dtype=torch.int32, device="cuda")
        ops.sample(logits, it, tk, tp, seeds, pos, nxt, use_topkp=True, ln_min_p=lmp)
        out.append(nxt.cpu().tolist())
    assert out[0] == out[1]
    sr.check_tokens(case, out[0])


# -- state advance ------------------------------------------------------------------------------------------
def test_chained_calls_count_on_the_device(cuda):
    """Three calls with state advance: the penalised rows, the tokens and the words after each call
    are the reference's; 32767 stays 32767."""
    pr.check_chain(pr.chain_run("cuda"))


# -- engine -------------------------------------------------------------------------------------------------
PROMPT = [(i * 13) % 700 + 256 for i in range(40)]
PEN = dict(repetition_penalty=1.3, frequency_penalty=0.2, presence_penalty=0.5)


def _engines(**kw):
    from llm_consensus_amd.engine.engine import Engine, EngineConfig
    from llm_consensus_amd.models.config import FAMILIES
    from llm_consensus_amd.models.transformer import TransformerWeights
    from llm_consensus_amd.parallel.comm import TPGroup

    cfg = FAMILIES["llama-tiny"]
    w = TransformerWeights(cfg, TPGroup.single(), torch.device("cuda:0"), 5, 1.0)
    return [Engine(cfg, EngineConfig(device="cuda:0", max_context=512, use_graphs=g, **kw), weights=w) for g in (True, False)]


def test_engine_graph_decode_equals_eager_steps(cuda):
    """24 tokens (three replays of 8 steps) with r = 1.3, f = 0.2, p = 0.5 and top-k 40 over captured
    graphs are exactly the tokens of the eager step-by-step path, and each of those obeys the
    decided-row rule against the reference applied to that step's raw logits and the running history."""
    from llm_consensus_amd.engine.engine import SamplingParams

    eg, ee = _engines()
    sp = SamplingParams(24, 1.0, 1.0, 40, 11, False, **PEN)
    graph = eg.generate_ids(PROMPT, 24, temperature=1.0, top_k=40, seed=11, stop_on_eos=False, **PEN)
    assert any(k.form.penalties for k in eg._graphs) and len(graph) == 24
    toks, lg = ee.debug_decode_logits_batch([PROMPT], 24, params=[sp])
    assert graph == toks[0]
    pr.check_steps(toks[0], lg[0].numpy(), PROMPT, sp)
    # the replays counted on the device: every kept token, plus the steps the last replay ran past them
    w = pr.words_array(eg.pen_words[0])
    assert set(np.flatnonzero(w & pr.CTX)) == set(PROMPT)
    cnt = (w & pr.COUNT).astype(int)
    assert all(cnt[t] >= graph.count(t) for t in graph) and cnt.sum() == 1 + 3 * eg.ecfg.steps_per_graph


def test_engine_presence_penalty_never_repeats(cuda):
    eg, _ = _engines()
    plain = eg.generate_ids(PROMPT, 64, temperature=0.0, stop_on_eos=False)
    assert eg.pen_words is None  # a neutral decode never allocates the table
    pen = eg.generate_ids(PROMPT, 64, temperature=0.0, stop_on_eos=False, presence_penalty=1e4)
    assert len(set(plain)) < 64 and len(set(pen)) == 64
    # ... and a neutral decode afterwards gives the tokens it gave before
    assert eg.generate_ids(PROMPT, 64, temperature=0.0, stop_on_eos=False) == plain


def test_engine_second_decode_counts_the_first_as_context(cuda):
    from llm_consensus_amd.engine.engine import SamplingParams

    eg, _ = _engines()
    sp = SamplingParams(12, 0.0, 1.0, 0, 0, False, **PEN)
    seq = eg.new_sequence()
    eg.prefill([seq], [PROMPT])
    first = eg.decode([seq], [sp])[0]
    eg.prefill([seq], [[7, 8, 9]])
    second = eg.decode([seq], [sp])[0]
    eg.synchronize()
    w = pr.words_array(eg.pen_words[0])
    assert set(np.flatnonzero(w & pr.CTX)) == set(PROMPT + first + [7, 8, 9])
    # the device row ran up to one replay past the 12 kept tokens: the kept ones are all counted
    cnt = (w & pr.COUNT).astype(int)
    assert all(cnt[t] >= second.count(t) for t in second) and 12 <= cnt.sum() <= 12 + 2 * eg.ecfg.steps_per_graph
    assert seq.ids == PROMPT + first + [7, 8, 9] + second
    eg.free_sequence(seq)


def test_batcher_rows_keep_their_solo_tokens(cuda):
    """Neutral, penalised and differently penalised requests admitted at different replays, the
    first retiring early so the rows behind it move down: each yields the tokens of its solo run."""
    from llm_consensus_amd.engine.batcher import ContinuousBatcher
    from llm_consensus_amd.engine.engine import SamplingParams

    eg, _ = _engines(max_batch=3)
    reqs = pr.batcher_requests(SamplingParams)
    solo = [eg.generate_batch([p], [sp])[0] for p, sp in reqs]
    assert pr.run_staggered(eg, reqs, ContinuousBatcher) == solo


# -- TP = 2 on one GPU ----------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _tp_worker(rank, world, port, q):
    import torch.distributed as dist

    try:
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
        from llm_consensus_amd.engine import Engine, EngineConfig, SamplingForm
        from llm_consensus_amd.models.config import FAMILIES
        from llm_consensus_amd.parallel.comm import TPGroup

        tp = TPGroup(dist.group.WORLD, rank, world)
        tp.enable_custom("cuda:0")
        e = Engine(FAMILIES["llama-small"], EngineConfig(device="cuda:0", max_context=512, seed=5), tp=tp)
        e.warmup_graphs()
        e.warmup_graphs(form=SamplingForm(penalties=True))
        gen = e.generate_ids(PROMPT, 32, temperature=0.0, stop_on_eos=False, presence_penalty=1e4)
        torch.cuda.synchronize()
        graphs = sorted((k.rows, tuple(k.form)) for k in e._graphs)  # (rows, (topkp, penalties, logprobs))
        q.put((rank, gen, graphs, tp.custom_timed_out()))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as ex:  # noqa: BLE001
        import traceback

        q.put((rank, repr(ex) + traceback.format_exc(), None, True))


def test_tp2_penalised_decode(cuda):
    """Two rank processes on one GPU: every rank keeps the full table and penalises the gathered
    row, so both end with identical tokens, none of them twice."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_tp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got = dict((r, (gen, graphs, tmo)) for r, gen, graphs, tmo in (q.get(timeout=400) for _ in range(2)))
    finally:
        for p in procs:
            p.join(timeout=120)
            if p.is_alive():
                p.terminate()
    for r in (0, 1):
        assert not isinstance(got[r][0], str), got[r][0]
        assert not got[r][2]
        assert (1, (False, True, False)) in got[r][1]  # the penalised form was captured, not run eagerly
    assert got[0][0] == got[1][0]
    assert len(got[0][0]) == 32 == len(set(got[0][0]))
