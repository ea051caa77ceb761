"""A dense TP = 2 engine decoding from the 12-bit packed twins of each rank's own weight shards: two rank
processes share ONE GPU (as tests/test_tp_gpu.py starts them) and the packed-on engine must produce exactly
the token ids of the packed-off TP = 2 engine (the packed launches return the bf16 launches' bits, the
row-parallel one with the all-reduce in its epilogue included), with the fused all-reduce (each rank on its
own half of the chip) and with separate all-reduce launches. A MoE model under TP stays unpacked.

Per-rank shapes of the model below: qkv 2560 x 2048 (2560 rows keep it off the one-launch qkv + attention),
o_proj 2048 x 2048, gate_up 7168 x 2048, down 2048 x 3584 (a row tail of 3 chunks), lm_head 1024 x 2048."""

import socket

import pytest
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

PROMPT = [1, 17, 300, 45, 1999, 7, 7, 1024, 512, 3]
N_NEW = 32


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q, model, fused):
    import os

    import torch
    import torch.distributed as dist

    try:
        os.environ["LLMC_FUSED_AR"] = "force" if fused else "0"
        if fused:  # each rank on its own half of the chip (as on GPUs of their own)
            os.environ["LLMC_CU_MASK"] = f"{rank * 128}-{rank * 128 + 127}"
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
        from llm_consensus_amd.engine import Engine, EngineConfig, SamplingParams
        from llm_consensus_amd.models.config import FAMILIES, ModelConfig
        from llm_consensus_amd.ops import wpack
        from llm_consensus_amd.parallel.comm import TPGroup
        from llm_consensus_amd.utils.native import kernels

        tp = TPGroup(dist.group.WORLD, rank, world)
        tp.enable_custom("cuda:0")
        assert (tp.custom_fused is not None) == fused
        # the row-parallel launches of the packed-on engine stream the twins: with the fused all-reduce
        # through gemv_ar_p12 (never its bf16 fallback), with separate launches through ops.linear
        k, launched = kernels(), []
        packed_launch = k.gemv_ar_p12

        def spy(*a):
            launched.append(packed_launch(*a))
            return launched[-1]

        k.gemv_ar_p12 = spy
        dense = model == "llama-tp-packed-test"
        cfg = (ModelConfig(model, "llama", 2, 2048, 32, 4, 128, 7168, 2048, 500000.0, max_position=4096)
               if dense else FAMILIES[model])

        def engine(packed, graphs, max_batch):
            e = Engine(cfg, EngineConfig(device="cuda:0", max_context=512, seed=3, use_graphs=graphs, steps_per_graph=4,
                                         packed_weights=packed, max_batch=max_batch), tp=tp)
            e.warmup_graphs()
            return e

        def tokens(eng, two_rows):
            out = [eng.generate_ids(PROMPT, N_NEW, temperature=0.0, stop_on_eos=False),
                   eng.generate_ids(PROMPT, N_NEW, temperature=0.9, top_p=0.95, top_k=40, seed=1234, stop_on_eos=False)]
            if two_rows:
                ps = [SamplingParams(N_NEW, 0.0, 1.0, 0, 0, False), SamplingParams(N_NEW, 0.8, 1.0, 0, 99, False)]
                out += eng.generate_batch([PROMPT, PROMPT[::-1]], ps)
            assert all(len(t) == N_NEW for t in out)
            return out

        def twins(eng):
            return [t for L in eng.w.layers for t in (L.p_qkv, L.p_o, L.p_gu, L.p_down)] + [eng.w.p_lm_head]

        for max_batch, graphs in ((1, True), (1, False), (2, True), (2, False)) if dense else ((1, True), (2, False)):
            off = engine("off", graphs, max_batch)
            assert not off.packed and not any(twins(off))
            want = tokens(off, max_batch == 2)
            assert not launched, "a packed-off engine launched the packed row-parallel GEMV"
            del off
            eng = engine("on", graphs, max_batch)
            if dense:
                assert eng.packed, "a dense TP engine with packed_weights on reports packed False"
                assert all(t is not None for t in twins(eng)), [type(t).__name__ for t in twins(eng)]
                assert all(isinstance(t, wpack.PackedWeight12) for t in twins(eng))
                assert all(type(L.p_down) is wpack.PackedWeight12Tail for L in eng.w.layers)
                assert 0 < eng.w.packed_nbytes() <= eng.w.packed_demand() <= cfg.packed_twin_bytes(tp=2)
            else:
                assert not eng.packed and not any(twins(eng))
            got = tokens(eng, max_batch == 2)
            assert got == want, (max_batch, graphs, got, want)
            if dense and fused:  # o_proj and down of both layers, every eager step or capture
                assert len(launched) >= 4 and all(launched), (len(launched), all(launched))
            else:
                assert not launched
            launched.clear()
            del eng
            torch.cuda.empty_cache()
        torch.cuda.synchronize()
        q.put((rank, None, tp.custom_timed_out()))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as ex:  # noqa: BLE001
        import traceback

        q.put((rank, repr(ex) + traceback.format_exc(), True))


def _run(model, fused):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, model, fused)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=400) for _ in range(2)]
    for p in procs:
        p.join(timeout=120)
    for rank, err, tmo in res:
        assert err is None, f"rank {rank}: {err}"
        assert not tmo, f"rank {rank}: a spin timed out"


@pytest.mark.parametrize("fused", [True, False], ids=["fused-ar", "separate-ar"])
def test_tp2_packed_engine_tokens_equal_packed_off(cuda, fused):
    """max_batch 1 and 2, graph replay and eager steps, greedy and seeded sampling: the packed-off ids."""
    _run("llama-tp-packed-test", fused)


def test_tp2_moe_engine_stays_unpacked(cuda):
    """A MoE model's expert shards under TP have no packed form: packed_weights on builds nothing."""
    _run("mixtral-tiny", False)
