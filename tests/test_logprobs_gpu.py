"""Token log-probabilities on the GPU (csrc/kernels/logprobs.hip): the two launches alone on every
shared case of logprob_ref.py, their column rule with a decode state, and the engine keeping the
values through graph decode, penalties, the batcher and tensor parallelism.

The value bound (logprob_ref.TOL = 1e-4 nats against the float64 reference) was derived, not
measured on the kernel: a float32 emulation of the two-stage sum (64 parts x 256 strided lanes, a
tree per part, the exp(m_p - M) rescale) run on the CPU stayed within 4e-6 of float64 up to
V = 152064 and |l| up to about 80; ``l - lse`` adds one rounding at magnitude <= 128 (7.6e-6); the
fast ``exp`` adds a few ulp per term. 1e-4 is roughly 5x that total. Ids are compared exactly: the
ranking is comparisons only, so no case is undecided. (test_logprobs_cpu.py shows which wrong
kernels the shared cases reject.)"""

import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import logprob_ref as lr
from llm_consensus_amd import ops

pytestmark = pytest.mark.gpu

CASES = lr.cases()
PAD = 1e30


def _device_logits(c):
    """The case's logits on the device; a strided case as a [B, V] view of its wider buffer."""
    if c.buffer is None:
        return torch.from_numpy(np.ascontiguousarray(c.logits)).cuda(), None
    buf = torch.from_numpy(c.buffer).cuda()
    return buf[:, :c.V], buf


# -- the kernels alone --------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_kernel_shared_cases(cuda, c):
    """Ids exactly the reference's, finite values within 1e-4 nats, -inf exact, the sampled token's
    value the bits of its top entry, the logits (and a strided case's padding) untouched, and a
    second run the same bits."""
    lg, buf = _device_logits(c)
    before = (buf if buf is not None else lg).clone()
    tok = torch.from_numpy(c.tokens).cuda()
    t, tv, ti = ops.token_logprobs(lg, tok, c.n)
    t2, tv2, ti2 = ops.token_logprobs(lg, tok, c.n)
    torch.cuda.synchronize()
    assert tv.shape == (c.B, c.n) and ti.shape == (c.B, c.n) and t.shape == (c.B,)
    lr.check(c, t.cpu().numpy(), tv.cpu().numpy(), ti.cpu().numpy())
    after = buf if buf is not None else lg
    assert torch.equal(after.view(torch.int32), before.view(torch.int32))
    if buf is not None:
        assert (buf[:, c.V:] == PAD).all()
    for a, b in ((t, t2), (tv, tv2)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(ti, ti2)


def test_kernel_writes_only_its_columns(cuda):
    """The rings are sentinel-filled and wider (20) than the launch (N = 5): only column 0, places
    [0, 5) of the first B rows change; the workspace rows past B stay as they were."""
    c = next(x for x in CASES if x.name == "gauss-B3-V1025-N5")
    lg, _ = _device_logits(c)
    rows, cap, W = c.B + 2, 3, 20
    lt = torch.full((rows, cap), 7.0, device="cuda")
    tv = torch.full((rows, cap, W), 7.0, device="cuda")
    ti = torch.full((rows, cap, W), 77, dtype=torch.int32, device="cuda")
    ws = ops.logprobs_workspace(rows, 5, "cuda")
    for w in ws:
        w.fill_(9)
    ops.token_logprobs(lg, torch.from_numpy(c.tokens).cuda(), 5, lp_tok=lt, lp_top_v=tv, lp_top_i=ti, ws=ws)
    torch.cuda.synchronize()
    lr.check(c, lt[:c.B, 0].cpu().numpy(), tv[:c.B, 0, :5].cpu().numpy(), ti[:c.B, 0, :5].cpu().numpy())
    assert (lt[c.B:] == 7).all() and (lt[:, 1:] == 7).all()
    assert (tv[c.B:] == 7).all() and (tv[:, 1:] == 7).all() and (tv[:, 0, 5:] == 7).all()
    assert (ti[c.B:] == 77).all() and (ti[:, 1:] == 77).all() and (ti[:, 0, 5:] == 77).all()
    assert all((w[c.B:] == 9).all() for w in ws)


def test_out_of_contract_rows_stay_in_bounds(cuda):
    """A row with +inf, an all -inf row, an all-NaN row: ids in [0, V) or -1, nothing outside written."""
    V = 1025
    lg = torch.randn(3, V, device="cuda")
    lg[0, 5] = float("inf")
    lg[1] = float("-inf")
    lg[2] = float("nan")
    tok = torch.tensor([5, 0, V - 1], dtype=torch.int32, device="cuda")
    _, _, ti = ops.token_logprobs(lg, tok, 20)
    ti = ti.cpu().numpy()
    assert ((ti >= -1) & (ti < V)).all()
    assert ti[0, 0] == 5 and ti[1].tolist() == list(range(20)) and (ti[2] == -1).all()


def test_ops_refuses_what_the_kernels_cannot_take(cuda):
    lg = torch.zeros(1, 64, device="cuda")
    tok = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        ops.token_logprobs(lg, tok, 21)
    with pytest.raises(ValueError):
        ops.token_logprobs(lg, tok, True)
    with pytest.raises(TypeError):
        ops.token_logprobs(lg.half(), tok, 1)
    with pytest.raises(TypeError):
        ops.token_logprobs(lg, tok.long(), 1)
    with pytest.raises(ValueError):  # 64 parts of 4096 floats
        ops.token_logprobs(torch.zeros(1, 64 * 4096 + 1, device="cuda"), tok, 1)


# -- with a decode state --------------------------------------------------------------------------------------
def test_chained_calls_follow_the_count(cuda):
    """Five bare calls with a decode state whose counts start at (0, 1, 2, cap - 1) and advance by one
    per call, as the sampler's launch does ahead of stage 2: call k writes column count - 1; a count
    of 0 (column -1) and counts past cap write nothing."""
    rng = np.random.default_rng(5)
    B, V, cap, n = 4, 257, 4, 5
    lt = torch.full((B, cap), 7.0, device="cuda")
    tv = torch.full((B, cap, 20), 7.0, device="cuda")
    ti = torch.full((B, cap, 20), 77, dtype=torch.int32, device="cuda")
    start = np.array([0, 1, 2, cap - 1], np.int32)
    count = torch.from_numpy(start.copy()).cuda()
    want = {}
    for k in range(5):
        logits = rng.standard_normal((B, V)).astype(np.float32) * 5
        tokens = rng.integers(0, V, B).astype(np.int32)
        ops.token_logprobs(torch.from_numpy(logits).cuda(), torch.from_numpy(tokens).cuda(), n, out_count=count,
                           lp_tok=lt, lp_top_v=tv, lp_top_i=ti)
        ref = lr.reference(logits, tokens, n)
        for b in range(B):
            col = int(start[b]) + k - 1
            if 0 <= col < cap:
                want[(b, col)] = (ref[0][b], ref[1][b], ref[2][b])
        count += 1
    torch.cuda.synchronize()
    lt, tv, ti = lt.cpu().numpy(), tv.cpu().numpy(), ti.cpu().numpy()
    assert (0, 0) in want and (3, cap - 1) in want and len(want) == 4 + 4 + 3 + 2
    for b in range(B):
        for col in range(cap):
            if (b, col) in want:
                r = want[(b, col)]
                assert np.array_equal(ti[b, col, :n], r[2])
                assert abs(lt[b, col] - r[0]) <= lr.TOL and np.abs(tv[b, col, :n] - r[1]).max() <= lr.TOL
            else:
                assert lt[b, col] == 7 and (tv[b, col] == 7).all() and (ti[b, col] == 77).all()
            assert (tv[b, col, n:] == 7).all() and (ti[b, col, n:] == 77).all()


# -- engine ---------------------------------------------------------------------------------------------------
PROMPT = [(i * 13) % 700 + 256 for i in range(40)]
PEN = dict(repetition_penalty=1.3, presence_penalty=0.5)


def _engines(**kw):
    from llm_consensus_amd.engine.engine import Engine, EngineConfig
    from llm_consensus_amd.models.config import FAMILIES
    from llm_consensus_amd.models.transformer import TransformerWeights
    from llm_consensus_amd.parallel.comm import TPGroup

    cfg = FAMILIES["llama-tiny"]
    w = TransformerWeights(cfg, TPGroup.single(), torch.device("cuda:0"), 5, 1.0)
    return [Engine(cfg, EngineConfig(device="cuda:0", max_context=512, use_graphs=g, **kw), weights=w) for g in (True, False)]


def _bits(entries):
    """Entries as exact values: Python floats hold the float32 results exactly."""
    return [(np.float32(lp).tobytes(), [(i, np.float32(v).tobytes()) for i, v in top]) for lp, top in entries]


@pytest.mark.parametrize("pen", [{}, PEN], ids=["plain", "penalised"])
def test_engine_graph_decode_equals_eager_steps(cuda, pen):
    """24 tokens (three replays of 8 steps) over captured graphs: the tokens and the log-probability
    entries of the eager path, bit for bit; the form has a graph key of its own."""
    eg, ee = _engines()
    kw = dict(temperature=1.0, top_k=40, seed=11, stop_on_eos=False, logprobs=20, **pen)
    g = eg.generate_ids(PROMPT, 24, **kw)
    e = ee.generate_ids(PROMPT, 24, **kw)
    assert len(g) == 24 == len(g.logprobs) and all(len(top) == 20 for _, top in g.logprobs)
    assert list(g) == list(e) and _bits(g.logprobs) == _bits(e.logprobs)
    assert any(k.form.logprobs and k.form.penalties == bool(pen) for k in eg._graphs) and not ee._graphs
    assert [t for _, top in g.logprobs for t, _ in top[:1]] != list(g)  # sampled, not always the argmax


@pytest.mark.parametrize("kw", [dict(temperature=0.0), dict(temperature=1.0, seed=3),
                                dict(temperature=0.8, seed=4, top_k=40, top_p=0.9),
                                dict(temperature=1.0, seed=5, top_k=40, **PEN)],
                         ids=["greedy", "sampled", "topkp", "topk-penalised"])
def test_engine_tokens_do_not_depend_on_logprobs(cuda, kw):
    """The same seeds with and without ``logprobs`` give the same tokens; len(logprobs) == len(tokens),
    each row truncated to the n it asked for; the off run holds no ring and no new graph key."""
    eg, _ = _engines()
    off = eg.generate_ids(PROMPT, 20, stop_on_eos=False, **kw)
    assert off.logprobs is None and eg.lp_tok is None and not any(k.form.logprobs for k in eg._graphs)
    for n in (0, 3):
        on = eg.generate_ids(PROMPT, 20, stop_on_eos=False, logprobs=n, **kw)
        assert list(on) == list(off) and len(on.logprobs) == 20
        assert all(len(top) == n for _, top in on.logprobs)
    if kw["temperature"] == 0.0 and n:
        assert all(top[0][0] == t and top[0][1] == lp for t, (lp, top) in zip(on, on.logprobs))
    assert list(eg.generate_ids(PROMPT, 20, stop_on_eos=False, **kw)) == list(off)


def test_engine_eos_and_max_tokens_cut_the_entries(cuda):
    """Entries stop where tokens stop: an EOS is cut and max_tokens (no multiple of the 8 steps) caps."""
    eg, _ = _engines()
    free = eg.generate_ids(PROMPT, 21, temperature=0.0, stop_on_eos=False, logprobs=2)
    assert len(free) == 21 == len(free.logprobs)
    from llm_consensus_amd.engine.engine import Engine, EngineConfig

    stop = Engine(eg.cfg.with_(eos_ids=(free[10],)), EngineConfig(device="cuda:0", max_context=512), weights=eg.w)
    cut = stop.generate_ids(PROMPT, 21, temperature=0.0, stop_on_eos=True, logprobs=2)
    k = list(free).index(free[10])
    assert list(cut) == list(free)[:k] and _bits(cut.logprobs) == _bits(free.logprobs[:k])


@pytest.mark.parametrize("pen", [{}, PEN], ids=["plain", "penalised"])
def test_engine_values_are_the_raw_rows(cuda, pen):
    """Eager steps: every step's ring column against the float64 reference of that step's RAW logits
    (debug_decode_logits_batch returns them before any penalty). Ids exact, values within the bound,
    also while a repetition + presence penalty rewrites the row the sampler reads."""
    from llm_consensus_amd.engine.engine import SamplingParams

    _, ee = _engines(max_batch=2)
    n = 12
    sps = [SamplingParams(n, 1.0, 1.0, 40, 11, False, logprobs=20, **pen),
           SamplingParams(n, 0.0, 1.0, 0, 0, False, logprobs=5, **pen)]
    toks, lg = ee.debug_decode_logits_batch([PROMPT, PROMPT[:17]], n, params=sps)
    lt, tv, ti = (t[:2, :n].cpu().numpy() for t in (ee.lp_tok, ee.lp_top_v, ee.lp_top_i))
    # the buffer the sampler read at the last step: the penalty launch rewrote it in place, and a kernel
    # that took its values from there would be told from the right one on these very rows
    last, read = lg[:, n - 1].numpy(), ee.logits_local[:2].float().cpu().numpy()
    assert bool(pen) == bool((last != read).any())
    if pen:
        tk = np.array([toks[0][-1], toks[1][-1]], np.int32)
        assert lr.differs(lr.reference(last, tk, 20), lr.reference(last, tk, 20, model="penalised_row", penalised=read))
    for b in range(2):
        for j in range(n):
            c = lr.Case(f"row{b}-step{j}", lg[b, j].numpy()[None], np.array([toks[b][j]], np.int32), 20)
            lr.check(c, lt[b, j:j + 1], tv[b, j:j + 1], ti[b, j:j + 1])


def test_batcher_rows_keep_their_solo_logprobs(cuda):
    """Requests with and without logprobs (and a penalised one) admitted at different replays, the
    first retiring early so the rows behind it move down: tokens and entries are the solo run's bits."""
    from llm_consensus_amd.engine.batcher import ContinuousBatcher
    from llm_consensus_amd.engine.engine import SamplingParams as SP

    eg, _ = _engines(max_batch=3)
    reqs = [([300 + i for i in range(12)], SP(max_tokens=6, temperature=0.0, stop_on_eos=False, logprobs=1)),
            ([400 + i for i in range(7)], SP(max_tokens=22, temperature=0.0, stop_on_eos=False, logprobs=20, **PEN)),
            ([500 + i for i in range(9)], SP(max_tokens=18, temperature=0.9, top_k=40, seed=7, stop_on_eos=False)),
            ([600 + i for i in range(5)], SP(max_tokens=27, temperature=0.9, seed=8, stop_on_eos=False, logprobs=4))]
    solo = [eg.generate_batch([p], [sp]) for p, sp in reqs]
    seen = {}
    bat = ContinuousBatcher(eg, on_logprobs=lambda row, ent: seen.setdefault(row.tag, []).extend(ent))
    rows = []
    for k, (prompt, sp) in enumerate(reqs):  # one admission per step: the rows join at different replays
        while not bat.free_rows:
            bat.step()
        seq = eg.new_sequence()
        eg.prefill([seq], [prompt])
        rows.append(bat.admit(seq, sp, tag=k))
        bat.step()
    bat.drain()
    for k, r in enumerate(rows):
        assert r.error is None and r.tokens == list(solo[k][0]), k
        if reqs[k][1].logprobs is None:
            assert r.logprobs is None and k not in seen
        else:
            assert len(r.logprobs) == len(r.tokens) and _bits(r.logprobs) == _bits(solo[k].logprobs[0]), k
            assert _bits(seen[k]) == _bits(r.logprobs)
        eg.free_sequence(r.seq)


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
        e.warmup_graphs([1])
        e.warmup_graphs([1], SamplingForm(logprobs=True))
        kw = dict(temperature=1.0, seed=9, top_k=0, stop_on_eos=False)
        off = e.generate_ids(PROMPT, 24, **kw)
        on = e.generate_ids(PROMPT, 24, logprobs=5, **kw)
        torch.cuda.synchronize()
        ring = [t[0, :24].cpu().numpy().tobytes() for t in (e.lp_tok, e.lp_top_v, e.lp_top_i)]
        graphs = sorted((k.rows, tuple(k.form)) for k in e._graphs if k.form.logprobs)  # plain values
        q.put((rank, (list(off), list(on), ring, on.logprobs, graphs), tp.custom_timed_out()))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as ex:  # noqa: BLE001
        import traceback

        q.put((rank, repr(ex) + traceback.format_exc(), True))


def test_tp2_logprobs(cuda):
    """Two rank processes on one GPU: every rank computes the gathered row's values, so both rings
    hold the same bits; the tokens are those of the run without logprobs; only the leader reports."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_tp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got = dict((r, (res, tmo)) for r, res, tmo in (q.get(timeout=400) for _ in range(2)))
    finally:
        for p in procs:
            p.join(timeout=120)
            if p.is_alive():
                p.terminate()
    for r in (0, 1):
        assert not isinstance(got[r][0], str), got[r][0]
        assert not got[r][1]
        off, on, ring, entries, graphs = got[r][0]
        assert off == on and len(on) == 24
        assert graphs and all(rows == 1 and form[2] for rows, form in graphs)  # the form was captured, not run eagerly
    assert got[0][0][1] == got[1][0][1] and got[0][0][2] == got[1][0][2]
    lead, peer = got[0][0][3], got[1][0][3]
    assert len(lead) == 24 and all(len(top) == 5 for _, top in lead) and peer == []
    ring_tok = np.frombuffer(got[0][0][2][0], np.float32)
    assert [np.float32(lp).tobytes() for lp, _ in lead] == [v.tobytes() for v in ring_tok]
