"""The row-parallel decode GEMV with the all-reduce in its epilogue (EPI_AR) streaming the 12-bit packed
twin of each rank's weight shard (csrc/kernels/gemv_ar_p12.hip): rank processes share ONE GPU (gloo
bootstrap, LLMC_FUSED_AR=force, as tests/test_custom_ar_gpu.py runs the bf16 launch) and
``gemv_allreduce(x, W, h, Wp=pack_best(W))`` must equal, bit for bit, both the bf16 fused launch and the
two-launch path (EPI_RESADD on rank 0 / EPI_BF16 elsewhere, then the one-shot all-reduce).

Co-residency. An EPI_AR block waits for the same block of its peers, and on a GPU that the ranks share
without a CU mask the dispatch-order argument does not hold across processes: every rank's whole grid has
to be resident at once. The shared-GPU cases therefore all have N < 2048, where the geometry rule
(gemv.hip pick_waves) gives 4-wave blocks of 256 threads with 8 loads per lane, and the arithmetic is, from
the build's kernel-resource-usage of gemv_ar_p12_kernel<M, 256, 8, TAIL>:

    M = 1: 111 VGPRs (110 without a tail) -> allocated 112 -> min(8, 512 // 112) = 4 waves per SIMD
    M = 2: 144 VGPRs                      -> allocated 144 -> min(8, 512 // 144) = 3 waves per SIMD
    4 SIMDs: 16 / 12 waves per CU (under the 32-wave limit) = 4 / 3 blocks of 4 waves per CU
    LDS: M * K * 2 + 2 * M * 4 * 4 bytes <= 2 * 8704 * 2 + 64 = 34 880 B -> 4 blocks in a CU's 160 KiB

so a CU holds at least 3 blocks and the chip 256 x 3 = 768. N = 512 is a grid of 128 blocks: a world of 4
has 512 in flight; N = 1022 is 256 blocks: a world of 2 has 512. (The bf16 kernels hold fewer registers.)
The 8- to 16-wave geometries (N >= 2048) cannot fit that way and run with each rank's stream on its own
half of the chip (``stream_cu_mask``, as Engine does for LLMC_CU_MASK): there the rank's own dispatch order
makes the wait safe. A mistake in this shows as the bounded 1-s spin giving up, which the tests assert
against, never as a hang."""

import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

# (N, K, waves per block of the geometry rule). K: 2048 one unit (issued before anything else); 4096 two
# units; 2560 / 3072 / 3584 a tail of 1 / 2 / 3 chunks, the three load shapes; 8192 / 8704 four units per row
# (the batch-ahead loop of the 8-loads geometry runs) without and with a tail
KS = (2048, 4096, 2560, 3072, 3584, 8192, 8704)
SHARED = [(512, K, 4) for K in KS] + [(1022, 2048, 4), (1022, 3584, 4)]  # 1022: a last block with waves past N
SHARED_WORLD4 = [(512, K, 4) for K in (2048, 3584, 8704)]
# on CU halves: 8-wave blocks (512 x 4 loads), 16-wave (1024 x 4; K >= 8192 with N <= 4096: 1024 x 8, two
# rows there on one unit per batch), 10-wave (640 x 4; K >= 8192: 640 x 8) and 12-wave (768 x 4)
HALVES = ([(2048, K, 8) for K in (2048, 4096, 2560, 3072, 3584)] +
          [(4096, K, 16) for K in (2048, 4096, 3584, 8192, 8704)] +
          [(2560, 2560, 10), (2560, 8192, 10), (3072, 4096, 12)])


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _plant(W, waves):
    """Rows that exercise the exception patch and the raw-row branch where a block's bookkeeping could go
    wrong: three exact zeros (each an exception: no window of a randn row holds exponent 0) in different
    wave chunks, the last one in the row's last chunk (the tail's where K has one: q >= 4 units), and 17
    zeros (more than the record's 16 slots: a raw row). The first and last row of a block get one each, and
    so does row N - 1, which the clamped waves of a ragged last block read beside its owner."""
    N, K = W.shape
    three, raw = [0, 2 * waves - 1, N - 1], [waves - 1, waves, N - 2]
    for r in three:
        W[r, 5] = 0.0
        W[r, 700] = 0.0
        W[r, K - 3] = 0.0
    for r in raw:
        W[r, torch.arange(17, device=W.device) * (K // 17) + 3] = 0.0
    return three, raw


def _worker(rank, world, port, q, plan, halves):
    try:
        import os

        import torch.distributed as dist

        from llm_consensus_amd import ops
        from llm_consensus_amd.ops import EPI_BF16, EPI_RESADD, wpack
        from llm_consensus_amd.parallel.comm import TPGroup
        from llm_consensus_amd.utils.native import kernels

        os.environ["LLMC_FUSED_AR"] = "force"  # ranks share the GPU (comm.py): see the module docstring
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
        tp = TPGroup(dist.group.WORLD, rank, world)
        assert tp.enable_custom("cuda:0") and tp.custom_fused is not None
        car = tp.custom_fused
        # every geometry below has its packed kernel: no launch may fall back to the bf16 stream (-8)
        k, launched = kernels(), []
        packed_launch = k.gemv_ar_p12

        def spy(*a):
            launched.append(packed_launch(*a))
            return launched[-1]

        k.gemv_ar_p12 = spy
        if halves:  # this rank's launches on its own half of the chip
            lo, hi = rank * 128, rank * 128 + 127
            words = [0] * 8
            for cu in range(lo, hi + 1):
                words[cu // 32] |= 1 << (cu % 32)
            stream = torch.cuda.ExternalStream(kernels().stream_cu_mask(0, words), device=torch.device("cuda:0"))
        else:
            stream = torch.cuda.Stream()
        bad = []

        def weights(N, K, waves, salt):
            g = torch.Generator(device="cuda").manual_seed(7919 * rank + salt)
            W = (torch.randn(N, K, generator=g, device="cuda") / K ** 0.5).to(torch.bfloat16)
            three, raw = _plant(W, waves)
            pw = wpack.pack_best(W)
            want = wpack.PackedWeight12Tail if K % 2048 else wpack.PackedWeight12
            assert isinstance(pw, want) and (pw.N, pw.K) == (N, K), (N, K, type(pw))
            hb = pw.records()[:, 0].to(torch.int64) & 0xFF
            assert bool((hb[raw] == 0xFF).all()), ("planted raw rows are not raw", N, K)
            assert bool((hb[three] != 0xFF).all()), ("a patched row went raw", N, K)
            assert pw.exceptions >= 3 * len(three)
            return W, pw

        def inputs(M, N, K, salt):
            g = torch.Generator(device="cuda").manual_seed(104729 * rank + salt)
            x = torch.randn(M, K, generator=g, device="cuda").to(torch.bfloat16)
            h0 = torch.randn(M, N, generator=torch.Generator(device="cuda").manual_seed(salt), device="cuda")
            return x, h0.to(torch.bfloat16)

        def two_launch(x, W, h):
            ops.linear(x, W, EPI_RESADD if rank == 0 else EPI_BF16, out=h)
            tp.all_reduce_(h)

        with torch.cuda.stream(stream):
            for ci, (N, K, waves) in enumerate(plan):
                W, pw = weights(N, K, waves, ci)
                for M in (1, 2):
                    x, h0 = inputs(M, N, K, 100 * ci + M)
                    hp, hb, hr = h0.clone(), h0.clone(), h0.clone()
                    torch.cuda.synchronize()
                    dist.barrier()
                    car.gemv_allreduce(x, W, hp, Wp=pw)
                    car.gemv_allreduce(x, W, hb)
                    two_launch(x, W, hr)
                    torch.cuda.synchronize()
                    if not torch.equal(hp, hb) or not torch.equal(hp, hr):
                        bad.append((M, N, K, float((hp.float() - hb.float()).abs().max()),
                                    float((hp.float() - hr.float()).abs().max())))
            if not halves:
                # HIP graph: an o-like and a down-like (tail) packed launch per replay, inputs refreshed in
                # place over 4 replays, so the epochs and both data parities advance
                (N1, K1), (N2, K2) = (512, 2048), (512, 3584)
                W1, p1 = weights(N1, K1, 4, 900)
                W2, p2 = weights(N2, K2, 4, 901)
                x1, h = inputs(1, N1, K1, 902)
                x2, _ = inputs(1, N2, K2, 903)
                car.gemv_allreduce(x1, W1, h, Wp=p1)
                torch.cuda.synchronize()
                dist.barrier()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=stream):
                    car.gemv_allreduce(x1, W1, h, Wp=p1)
                    car.gemv_allreduce(x2, W2, h, Wp=p2)
                for rep in range(4):
                    xa, h0 = inputs(1, N1, K1, 950 + rep)
                    xb, _ = inputs(1, N2, K2, 990 + rep)
                    x1.copy_(xa)
                    x2.copy_(xb)
                    h.copy_(h0)
                    torch.cuda.synchronize()
                    dist.barrier()
                    g.replay()
                    torch.cuda.synchronize()
                    hr = h0.clone()
                    two_launch(x1, W1, hr)
                    two_launch(x2, W2, hr)
                    torch.cuda.synchronize()
                    if not torch.equal(h, hr):
                        bad.append(("graph", rep, float((h.float() - hr.float()).abs().max())))
        want = 2 * len(plan) + (0 if halves else 3)  # per case M = 1, 2; the graph: a warm-up and two captured
        if launched != [True] * want:
            bad.append(("packed launches", want, launched))
        q.put((rank, bad, tp.custom_timed_out()))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # noqa: BLE001
        import traceback

        q.put((rank, repr(e) + traceback.format_exc(), True))


def _run(world, plan, halves):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, plan, halves)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
    for rank, bad, tmo in res:
        assert not isinstance(bad, str), bad
        assert not tmo, f"rank {rank}: a spin timed out"
        assert bad == [], (rank, bad)


@pytest.mark.parametrize("world", [2, 4])
def test_packed_fused_allreduce_gemv_shared_gpu(cuda, world):
    """4-wave blocks, every rank's grid resident at once (module docstring); a world of 4 only with N = 512."""
    _run(world, SHARED if world == 2 else SHARED_WORLD4, halves=False)


def test_packed_fused_allreduce_gemv_cu_halves(cuda):
    """The 8-, 10-, 12- and 16-wave geometries, each rank on its own half of the chip."""
    _run(2, HALVES, halves=True)


def test_packed_fused_allreduce_argument_checks(cuda):
    """The entry point's checks run before anything is launched: K off the format, no planes."""
    from llm_consensus_amd.ops import wpack
    from llm_consensus_amd.utils.native import kernels

    W = (torch.randn(64, 2048) / 45).to(torch.bfloat16).cuda()
    pw = wpack.pack12(W)
    x = torch.zeros(1, 2048, dtype=torch.bfloat16, device="cuda")
    h = torch.zeros(1, 64, dtype=torch.bfloat16, device="cuda")
    k, p = kernels(), lambda t: t.data_ptr()
    for M, K, planes, recs in ((1, 1024, p(pw.planes), p(pw.hdr)), (1, 2304, p(pw.planes), p(pw.hdr)),
                               (1, 2048, 0, p(pw.hdr)), (1, 2048, p(pw.planes), p(pw.hdr) + 2),
                               (3, 2048, p(pw.planes), p(pw.hdr))):
        with pytest.raises(RuntimeError, match="rc=-1"):
            k.gemv_ar_p12(M, p(x), 2048, p(W), planes, recs, p(h), 64, 64, K, [p(h)], 0, 0, 1, 1 << 20, 0)
