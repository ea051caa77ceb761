"""Token log-probabilities without a GPU: the torch oracle against the float64 reference of
logprob_ref.py on every shared case, the wrong kernels those cases have to reject, a CPU engine
through decode and the batcher, and the knob's way up: check_sampling, the server, the worker pipe
and the CLI."""

import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import logprob_ref as lr
from llm_consensus_amd import ops
from llm_consensus_amd.ops import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = lr.cases()


# -- reference, oracle, wrong models ------------------------------------------------------------------
def test_the_shared_cases_cover_what_they_claim():
    names = {c.name for c in CASES}
    for B in (1, 3):
        for V in (1, 19, 63, 64, 65, 255, 257, 1025, 16385):
            for n in (0, 1, 5, 20):
                assert f"gauss-B{B}-V{V}-N{n}" in names
    assert all(np.nanmax(np.abs(np.where(np.isinf(c.logits), 0, c.logits))) <= 70 for c in CASES)
    c = next(x for x in CASES if x.name == "ties-straddle-N-and-part")
    _, _, ti = lr.reference(c.logits, c.tokens, c.n)
    assert ti[0].tolist() == [3, 16, 17, 18, 500]  # seven tied: the five smallest ids, across the part boundary
    c = next(x for x in CASES if x.name == "part-of-minus-inf")
    assert np.isinf(c.logits[:, 85:102]).all()
    c = next(x for x in CASES if x.name == "nan-V-below-N")
    _, tv, ti = lr.reference(c.logits, c.tokens, c.n)
    assert (ti[0, 16:] == -1).all() and np.isneginf(tv[0, 16:]).all() and (ti[0, :16] >= 0).all()
    assert any(c.buffer is not None for c in CASES)
    assert any(0 in lr.reference(c.logits, c.tokens, c.n)[2] and c.V - 1 in lr.reference(c.logits, c.tokens, c.n)[2]
               for c in CASES if c.name.startswith("edge-ids"))


def _oracle(c):
    lg = torch.from_numpy(c.buffer)[:, :c.V] if c.buffer is not None else torch.from_numpy(np.ascontiguousarray(c.logits))
    return [t.numpy() for t in ops.token_logprobs(lg, torch.from_numpy(c.tokens), c.n)]


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_oracle_equals_reference(c):
    """CPU tensors go to oracle.token_logprobs: ids exact, values within the bound, token = top bits."""
    t, tv, ti = _oracle(c)
    assert t.dtype == np.float32 and tv.dtype == np.float32 and ti.dtype == np.int32
    lr.check(c, t, tv, ti)
    if c.buffer is not None:
        assert (c.buffer[:, c.V:] == np.float32(1e30)).all()


@pytest.mark.parametrize("model", lr.MODELS)
def test_wrong_models_are_rejected(model):
    """Every wrong kernel disagrees with the reference on at least one shared case, by the very
    comparison the GPU test makes (ids exact, values within TOL)."""
    assert lr.rejected_by(model), model


def test_the_right_model_is_not_rejected():
    for c in CASES:
        r = lr.reference(c.logits, c.tokens, c.n)
        assert not lr.differs(r, lr.reference(c.logits, c.tokens, c.n, model="right"))


def test_ops_checks_its_arguments():
    lg = torch.zeros(2, 64)
    tok = torch.zeros(2, dtype=torch.int32)
    for bad in (21, -1, True, 2.0):
        with pytest.raises(ValueError):
            ops.token_logprobs(lg, tok, bad)
    with pytest.raises(TypeError):
        ops.token_logprobs(lg.double(), tok, 1)
    with pytest.raises(TypeError):
        ops.token_logprobs(lg.t(), tok, 1)
    with pytest.raises(TypeError):
        ops.token_logprobs(lg, tok.long(), 1)
    with pytest.raises(ValueError):
        ops.token_logprobs(torch.zeros(1, 64 * 4096 + 1), tok, 1)
    with pytest.raises(ValueError):
        ops.token_logprobs(lg, tok, 1, out_count=torch.ones(2, dtype=torch.int32))
    t, tv, ti = ops.token_logprobs(lg, tok, 0)
    assert tv.shape == (2, 0) and torch.allclose(t, torch.full((2,), -float(np.log(64))))


def test_columns_follow_the_count_on_the_cpu():
    B, V, cap = 2, 65, 3
    lt = torch.full((B, cap), 7.0)
    tv = torch.full((B, cap, 20), 7.0)
    ti = torch.full((B, cap, 20), 77, dtype=torch.int32)
    lg = torch.randn(B, V)
    tok = torch.tensor([3, 64], dtype=torch.int32)
    ops.token_logprobs(lg, tok, 2, out_count=torch.tensor([2, 9], dtype=torch.int32), lp_tok=lt, lp_top_v=tv, lp_top_i=ti)
    want = oracle.token_logprobs(lg, tok, 2)
    assert lt[0, 1] == want[0][0] and torch.equal(tv[0, 1, :2], want[1][0]) and torch.equal(ti[0, 1, :2], want[2][0])
    assert (lt[1] == 7).all() and (lt[0, [0, 2]] == 7).all() and (tv[:, :, 2:] == 7).all() and (ti[1] == 77).all()


# -- engine -------------------------------------------------------------------------------------------------
PROMPT = list(range(300, 320))
PEN = dict(repetition_penalty=1.3, presence_penalty=0.5)


def _tiny_engine(**kw):
    from llm_consensus_amd.engine.engine import Engine, EngineConfig
    from llm_consensus_amd.models.config import FAMILIES

    return Engine(FAMILIES["llama-tiny"], EngineConfig(device="cpu", max_context=256, use_graphs=False, seed=5, **kw))


def test_engine_off_is_the_engine_of_before():
    eng = _tiny_engine()
    out = eng.generate_ids(PROMPT, 12, temperature=0.0, stop_on_eos=False)
    assert out.logprobs is None and eng.lp_tok is None and eng.lp_raw is None
    on = eng.generate_ids(PROMPT, 12, temperature=0.0, stop_on_eos=False, logprobs=0)
    assert list(on) == list(out) and len(on.logprobs) == 12 and all(top == [] for _, top in on.logprobs)
    assert eng.lp_tok is not None and eng.lp_raw is None  # the raw copy only beside penalties


@pytest.mark.parametrize("pen", [{}, PEN], ids=["plain", "penalised"])
def test_engine_steps_report_the_raw_rows(pen):
    """decode's entries against the reference of each step's raw logits (the rows
    debug_decode_logits_batch returns, before any penalty), also while a penalty rewrites the row."""
    from llm_consensus_amd.engine.engine import SamplingParams

    eng = _tiny_engine()
    n = 10
    sp = SamplingParams(n, 1.0, 1.0, 40, 11, False, logprobs=7, **pen)
    seen = []
    out = eng.generate_batch([PROMPT], [sp], on_logprobs=lambda i, ent: seen.extend(ent))
    assert len(out.logprobs[0]) == n == len(out[0]) and seen == out.logprobs[0]
    toks, lg = eng.debug_decode_logits_batch([PROMPT], n, params=[sp])
    assert toks[0] == list(out[0])
    assert (eng.lp_raw is not None) == bool(pen)
    for j, (lp, top) in enumerate(out.logprobs[0]):
        assert len(top) == 7
        c = lr.Case(f"step{j}", lg[0, j].numpy()[None], np.array([toks[0][j]], np.int32), 7)
        lr.check(c, np.float32([lp]), np.float32([[v for _, v in top]]), np.array([[i for i, _ in top]]))
    if pen:  # the row the sampler read differs from the raw one where it matters
        last, read = lg[:, n - 1].numpy(), eng.logits_local[:1].float().numpy()
        tk = np.array([toks[0][-1]], np.int32)
        assert lr.differs(lr.reference(last, tk, 20), lr.reference(last, tk, 20, model="penalised_row", penalised=read))


def test_engine_entries_stop_where_tokens_stop():
    from llm_consensus_amd.engine.engine import Engine, EngineConfig

    eng = _tiny_engine()
    free = eng.generate_ids(PROMPT, 13, temperature=0.0, stop_on_eos=False, logprobs=2)
    assert len(free) == 13 == len(free.logprobs)
    stop = Engine(eng.cfg.with_(eos_ids=(free[6],)), EngineConfig(device="cpu", max_context=256, use_graphs=False),
                  weights=eng.w)
    cut = stop.generate_ids(PROMPT, 13, temperature=0.0, stop_on_eos=True, logprobs=2)
    k = list(free).index(free[6])
    assert list(cut) == list(free)[:k] and cut.logprobs == free.logprobs[:k]


def test_engine_refuses_a_bad_width():
    from llm_consensus_amd.engine.engine import EngineError

    eng = _tiny_engine()
    for bad in (21, -1, True):
        with pytest.raises(EngineError):
            eng.generate_ids(PROMPT, 2, logprobs=bad)


def test_batcher_rows_keep_their_solo_logprobs():
    from llm_consensus_amd.engine.batcher import ContinuousBatcher
    from llm_consensus_amd.engine.engine import SamplingParams as SP

    eng = _tiny_engine(max_batch=3, steps_per_graph=4)
    reqs = [([300 + i for i in range(12)], SP(max_tokens=6, temperature=0.0, stop_on_eos=False, logprobs=1)),
            ([400 + i for i in range(7)], SP(max_tokens=22, temperature=0.0, stop_on_eos=False, logprobs=20, **PEN)),
            ([500 + i for i in range(9)], SP(max_tokens=18, temperature=0.9, top_k=40, seed=7, stop_on_eos=False)),
            ([600 + i for i in range(5)], SP(max_tokens=15, temperature=0.9, seed=8, stop_on_eos=False, logprobs=4))]
    solo = [eng.generate_batch([p], [sp]) for p, sp in reqs]
    bat = ContinuousBatcher(eng)
    rows = []
    for k, (prompt, sp) in enumerate(reqs):
        while not bat.free_rows:
            bat.step()
        seq = eng.new_sequence()
        eng.prefill([seq], [prompt])
        rows.append(bat.admit(seq, sp, tag=k))
        bat.step()
    bat.drain()
    # The CPU oracle's bf16 matmuls are not batch-invariant (a row's logits move by about 1e-2 with the
    # rows beside it), so the values are compared loosely here: a row that picked up another row's
    # columns would be off by nats. The GPU test compares the bits.
    for k, r in enumerate(rows):
        assert r.error is None and r.tokens == list(solo[k][0]), k
        want = solo[k].logprobs[0]
        if want is None:
            assert r.logprobs is None
            continue
        assert len(r.logprobs) == len(r.tokens) == len(want)
        for (lp, top), (wlp, wtop) in zip(r.logprobs, want):
            assert len(top) == len(wtop) == reqs[k][1].logprobs and abs(lp - wlp) < 0.05
            assert all(abs(a[1] - b[1]) < 0.05 for a, b in zip(top, wtop))
        eng.free_sequence(r.seq)


# -- public interface ---------------------------------------------------------------------------------------
def test_check_sampling():
    from llm_consensus_amd.provider.base import Request, Response, check_sampling

    for ok in (None, 0, 1, 20):
        check_sampling(logprobs=ok)
    for bad in (True, False, 1.0, 3.5, "3", -1, 21, [1]):
        with pytest.raises(ValueError) as ex:
            check_sampling(logprobs=bad)
        assert str(ex.value).startswith("logprobs: ")
    assert Request(model="m", prompt="p").logprobs is None and Response().logprobs is None


def test_sampling_form_keeps_its_two_entries():
    from llm_consensus_amd.provider.base import Request
    from llm_consensus_amd.provider.local import sampling_form

    assert sampling_form(Request(model="", prompt="", logprobs=5), None, False) == (False, False)


def test_cli_flag():
    import io

    from llm_consensus_amd import cli

    def parse(argv):
        err = io.StringIO()
        return cli.parse_flags(argv, stdout=io.StringIO(), stderr=err), err

    cfg, _ = parse(["--models", "stub-a", "hi"])
    assert cfg.logprobs is None and cli._request_template(cfg).logprobs is None
    cfg, _ = parse(["--models", "stub-a", "--logprobs", "0", "hi"])
    assert cfg.logprobs == 0 and cli._request_template(cfg).logprobs == 0
    cfg, _ = parse(["--models", "stub-a", "--logprobs=20", "hi"])
    assert cfg.logprobs == 20
    for bad in ("21", "-2", "1.5", "x"):
        err = io.StringIO()
        with pytest.raises(SystemExit) as ex:
            cli.parse_flags(["--models", "llama-tiny", f"--logprobs={bad}", "hi"], stdout=io.StringIO(), stderr=err)
        assert ex.value.code == 2
        text = err.getvalue()
        assert text.startswith(f'invalid value "{bad}" for flag -logprobs: ') and "Usage of llm-consensus:" in text


@pytest.fixture
def stub_service():
    from llm_consensus_amd.server import ConsensusService

    svc = ConsensusService(["stub-a"], "stub-j", concurrency=1)
    yield svc
    svc.close()


def test_server_parse(stub_service):
    from llm_consensus_amd.server import BadRequest, ConsensusService

    svc = stub_service
    assert svc.parse({"prompt": "hi"})["logprobs"] is None
    assert svc.parse({"prompt": "hi", "logprobs": None})["logprobs"] is None
    assert svc.parse({"prompt": "hi", "logprobs": 0})["logprobs"] == 0
    assert svc.parse({"prompt": "hi", "logprobs": 20})["logprobs"] == 20
    for bad in (21, -1, True, 2.0, "3", [1]):
        with pytest.raises(BadRequest) as ex:
            svc.parse({"prompt": "hi", "logprobs": bad})
        assert str(ex.value).startswith("logprobs: ")
    with pytest.raises(ValueError):
        ConsensusService(["stub-a"], "stub-j", logprobs=21)
    dflt = ConsensusService(["stub-a"], "stub-j", concurrency=1, logprobs=2)
    try:
        assert dflt.parse({"prompt": "hi"})["logprobs"] == 2 and dflt.parse({"prompt": "hi", "logprobs": 0})["logprobs"] == 0
    finally:
        dflt.close()


def _post(url, body):
    import urllib.error
    import urllib.request

    rq = urllib.request.Request(url, data=json.dumps(body).encode(), headers={"Content-Type": "application/json"})
    try:
        with urllib.request.urlopen(rq, timeout=120) as r:
            return r.status, r.read().decode()
    except urllib.error.HTTPError as e:
        return e.code, e.read().decode()


def _serving(svc):
    import threading

    from llm_consensus_amd.server import ConsensusServer

    srv = ConsensusServer(("127.0.0.1", 0), svc)
    threading.Thread(target=srv.serve_forever, kwargs={"poll_interval": 0.05}, daemon=True).start()
    return srv, f"http://127.0.0.1:{srv.server_address[1]}/v1/consensus"


def test_server_answers_400_and_stub_replies(stub_service):
    """A bad value is a 400; the stub ignores the knob, so the reply of a request that asks is today's
    object plus one last key with empty lists; a request that does not ask gets today's keys."""
    srv, url = _serving(stub_service)
    try:
        code, text = _post(url, {"prompt": "hi", "logprobs": 21})
        assert code == 400 and json.loads(text)["error"].startswith("logprobs: ")
        code, plain = _post(url, {"prompt": "hi"})
        assert code == 200 and "logprobs" not in json.loads(plain)
        code, text = _post(url, {"prompt": "hi", "logprobs": 3})
        d = json.loads(text)
        assert code == 200 and list(d)[-1] == "logprobs" and list(d)[:-1] == list(json.loads(plain))
        assert d["logprobs"] == {"responses": {"stub-a": []}, "judge": []}
    finally:
        srv.shutdown()
        srv.server_close()


# -- CPU workers, end to end ------------------------------------------------------------------------------------
def _check_entries(entries, n_top, tok, content=None):
    assert all(set(e) == {"id", "token", "logprob", "top"} and len(e["top"]) == n_top for e in entries)
    for e in entries:
        assert e["logprob"] <= 0 and e["token"] == tok.decode([e["id"]])
        lps = [t["logprob"] for t in e["top"]]
        assert lps == sorted(lps, reverse=True) and all(set(t) == {"id", "token", "logprob"} for t in e["top"])
        assert all(e["logprob"] == t["logprob"] for t in e["top"] if t["id"] == e["id"])
    if content is not None:
        assert tok.decode([e["id"] for e in entries]) == content


def test_worker_pipe_carries_logprobs(monkeypatch):
    """LLMC_DEVICE=cpu worker, llama-tiny: a request that asks gets a "logprobs" message after every
    "tokens" message and one entry per output token; one that does not sees today's messages; a judge
    session carries the knob like any request."""
    from llm_consensus_amd.catalog import resolve
    from llm_consensus_amd.context import Context
    from llm_consensus_amd.provider.base import Request
    from llm_consensus_amd.provider.local import LocalBackend

    monkeypatch.setenv("LLMC_DEVICE", "cpu")
    name = "llama-tiny@lp"
    be = LocalBackend([resolve(name)], judge=name, max_context={name: 512})
    try:
        prov = be.provider(name)
        kinds = []
        deliver = be._deliver

        def tap(msg):
            kinds.append(msg[0])
            deliver(msg)

        be._deliver = tap
        kw = dict(model=name, prompt="tell me about loops", max_tokens=20, temperature=0.0, stop_on_eos=False)
        off = prov.query(Context.background(), Request(**kw))
        assert off.logprobs is None and "logprobs" not in kinds
        kinds.clear()
        on = prov.query(Context.background(), Request(logprobs=3, **kw))
        assert on.content == off.content and on.output_tokens == 20 == len(on.logprobs)
        assert kinds.count("logprobs") == kinds.count("tokens") > 0
        assert all(b == "logprobs" for a, b in zip(kinds, kinds[1:]) if a == "tokens")
        _check_entries(on.logprobs, 3, prov.tok, on.content)
        assert all(e["top"][0]["id"] == e["id"] for e in on.logprobs)  # greedy, no penalty: the argmax
        # judge session: header prefilled ahead, the finish carries the knob
        sess = prov.new_session("Header. ")
        sess.extend("Block one. ")
        r = sess.finish(Context.background(), Request(model=name, prompt="Header. Block one. Trailer.", max_tokens=9,
                                                      temperature=0.0, stop_on_eos=False, logprobs=0), None)
        assert r.output_tokens == 9 == len(r.logprobs)
        _check_entries(r.logprobs, 0, prov.tok, r.content)
    finally:
        be.close()


def _run_cli(args, timeout=600):
    e = dict(os.environ, LLMC_DEVICE="cpu")
    r = subprocess.run([sys.executable, "-m", "llm_consensus_amd", *args], capture_output=True, cwd=ROOT, env=e,
                       timeout=timeout, stdin=subprocess.DEVNULL)
    return r.returncode, r.stdout, r.stderr.decode("utf-8", "replace")


def test_cli_writes_logprobs_json_and_nothing_else_changes(tmp_path):
    """--logprobs 3 with CPU workers: logprobs.json holds one entry per output token of every model
    and of the judge; result.json, prompt.txt, consensus.md and stdout are the bytes of the run
    without the flag (latency_ms, a wall-clock reading that no two runs share, is blanked in both)."""
    from llm_consensus_amd.utils.tokenizer import get_tokenizer

    # one responder model twice (two rows of one batch, greedy: identical blocks), so the order in which
    # the responses complete, which is timing too, cannot change a byte of result.json or of the judge prompt
    base = ["--models", "llama-tiny,llama-tiny", "--judge", "llama-tiny@j", "--max-tokens", "7", "--temperature",
            "0", "--seed", "3", "--quiet"]
    runs = {}
    for tag, extra in (("off", []), ("on", ["--logprobs", "3"])):
        d = tmp_path / tag
        rc, out, err = _run_cli(base + extra + ["--data-dir", str(d), "Explain RoPE."])
        assert rc == 0, err
        run = d / os.listdir(d)[0]
        files = {f: (run / f).read_bytes() for f in os.listdir(run)}
        files["result.json"] = re.sub(rb'"latency_ms": \d+', b'"latency_ms": 0', files["result.json"])
        runs[tag] = (files, re.sub(rb'"latency_ms": \d+', b'"latency_ms": 0', out))
    off, on = runs["off"], runs["on"]
    assert set(off[0]) == {"result.json", "prompt.txt", "consensus.md"}
    assert set(on[0]) == set(off[0]) | {"logprobs.json"}
    for f in off[0]:
        assert on[0][f] == off[0][f], f
    assert on[1] == off[1]
    res = json.loads(on[0]["result.json"])
    lp = json.loads(on[0]["logprobs.json"])
    tok = get_tokenizer(1024)
    assert set(lp) == {"responses", "judge", "summary"} and set(lp["responses"]) == {"llama-tiny"}
    assert len(res["responses"]) == 2
    for r in res["responses"]:
        ent = lp["responses"][r["model"]]
        assert 1 <= len(ent) <= 7
        _check_entries(ent, 3, tok, r["content"])
        s = lp["summary"]["responses"][r["model"]]
        mean = sum(e["logprob"] for e in ent) / len(ent)
        assert s["tokens"] == len(ent) and abs(s["mean_logprob"] - mean) < 1e-9
        assert abs(s["perplexity"] - np.exp(-mean)) < 1e-6 * np.exp(-mean)
    assert 1 <= len(lp["judge"]) <= 7 and lp["summary"]["judge"]["tokens"] == len(lp["judge"])
    _check_entries(lp["judge"], 3, tok, res["consensus"])


def test_server_streams_logprobs_of_local_models(monkeypatch):
    """A CPU-worker service: model_done and judge_done gain "logprobs" with len == output_tokens when
    asked; the non-streaming reply ends in the same object; a request that does not ask sees neither."""
    import http.client

    from llm_consensus_amd.server import ConsensusService

    monkeypatch.setenv("LLMC_DEVICE", "cpu")
    svc = ConsensusService(["llama-tiny@a", "llama-tiny@b"], "llama-tiny@j", concurrency=1, max_tokens=6, temperature=0.0)
    srv, url = _serving(svc)
    try:
        def stream(body):
            conn = http.client.HTTPConnection("127.0.0.1", srv.server_address[1], timeout=120)
            conn.request("POST", "/v1/consensus", body=json.dumps(dict(body, stream=True)).encode())
            text = conn.getresponse().read().decode()
            conn.close()
            evs = []
            for block in text.split("\n\n"):
                lines = block.split("\n")
                if lines[0].startswith("event: "):
                    evs.append((lines[0][7:], "\n".join(ln[6:] for ln in lines[1:] if ln.startswith("data: "))))
            return evs

        evs = stream({"prompt": "hi there", "logprobs": 2})
        done = [json.loads(p) for n, p in evs if n == "model_done"]
        jdone = [json.loads(p) for n, p in evs if n == "judge_done"]
        assert len(done) == 2 and len(jdone) == 1
        for d in done + jdone:
            assert d["output_tokens"] == len(d["logprobs"]) > 0 and all(len(e["top"]) == 2 for e in d["logprobs"])
        result = next(p for n, p in evs if n == "result")
        assert "logprobs" not in json.loads(result)
        evs = stream({"prompt": "hi there"})
        assert all("logprobs" not in json.loads(p) for n, p in evs if n in ("model_done", "judge_done"))
        plain = next(p for n, p in evs if n == "result")
        code, text = _post(url, {"prompt": "hi there", "logprobs": 2})
        d = json.loads(text)
        assert code == 200 and list(d)[-1] == "logprobs" and list(d)[:-1] == list(json.loads(plain))
        assert d["logprobs"]["responses"] == {x["model"]: x["logprobs"] for x in done}
        # the judge prefills its session in the order the responses complete, which moves its bf16 logits
        # a little from run to run: its entries are compared by shape only
        assert len(d["logprobs"]["judge"]) > 0 and all(len(e["top"]) == 2 for e in d["logprobs"]["judge"])
    finally:
        srv.shutdown()
        srv.server_close()
        svc.close()
