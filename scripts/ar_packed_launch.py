"""Per-launch time of the row-parallel decode GEMV with the all-reduce in its epilogue (EPI_AR), the
12-bit packed stream against the bf16 stream of the same shard, cold: two rank processes share ONE GPU, each
on its own half of the CUs (as scripts/tp_rehearsal.py runs a group), and every launch of a run reads a
different copy of the shard's weights (enough copies to push the last one out of L2 and the MALL before it
comes round again). The two forms alternate within a run; the figure of a run is its window's time over its
launches, device events around the window. The keep rule of ``ops.wpack.AR_STAYS_BF16`` is applied to the
output: packed must beat bf16 by more than the spread of the runs.

  python scripts/ar_packed_launch.py [--shapes 8192x2048,8192x7168,...] [--runs 5] [--rows 1]
"""
import argparse
import os
import socket
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# the catalog's row-parallel shards that have a twin: o_proj and down of Llama-3-70B on 4 ranks, its down on
# 8 (o_proj K = 1024 has no twin), Llama-3-8B's o_proj and down on 2 ranks, its down on 4 (o_proj K = 1024)
SHAPES = "8192x2048,8192x7168,8192x3584,4096x2048,4096x7168,4096x3584"
COLD_BYTES = 1 << 30  # copies of a shape cover at least this much: L2 (4 MiB per XCD) and the 256-MiB MALL


def _worker(rank, a, port, q):
    os.environ["LLMC_FUSED_AR"] = "force"
    import torch
    import torch.distributed as dist

    from llm_consensus_amd.ops import wpack
    from llm_consensus_amd.parallel.comm import TPGroup
    from llm_consensus_amd.utils.native import kernels

    try:
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=2)
        tp = TPGroup(dist.group.WORLD, rank, 2)
        assert tp.enable_custom("cuda:0") and tp.custom_fused is not None
        car = tp.custom_fused
        words = [0] * 8
        for cu in range(rank * 128, rank * 128 + 128):
            words[cu // 32] |= 1 << (cu % 32)
        stream = torch.cuda.ExternalStream(kernels().stream_cu_mask(0, words), device=torch.device("cuda:0"))
        out = []
        with torch.cuda.stream(stream):
            for N, K in a.shape_list:
                copies = max(4, -(-COLD_BYTES // (N * K * 2)))
                g = torch.Generator(device="cuda").manual_seed(17 * rank + N + K)
                Ws = [(torch.randn(N, K, generator=g, device="cuda") / K ** 0.5).to(torch.bfloat16) for _ in range(copies)]
                Ps = [wpack.pack_best(W) for W in Ws]
                assert all(isinstance(p, wpack.PackedWeight12) for p in Ps), (N, K)
                x = torch.randn(a.rows, K, generator=g, device="cuda").to(torch.bfloat16)
                h = torch.zeros(a.rows, N, dtype=torch.bfloat16, device="cuda")
                for W, P in zip(Ws, Ps):  # one untimed window of each form: code objects, page tables, clocks
                    car.gemv_allreduce(x, W, h)
                for W, P in zip(Ws, Ps):
                    car.gemv_allreduce(x, W, h, Wp=P)
                torch.cuda.synchronize()
                times = {"bf16": [], "p12": []}
                for run in range(a.runs):
                    for form in (("bf16", "p12") if run % 2 == 0 else ("p12", "bf16")):
                        h.zero_()
                        torch.cuda.synchronize()
                        dist.barrier()
                        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        t0.record()
                        for W, P in zip(Ws, Ps):
                            car.gemv_allreduce(x, W, h, Wp=P if form == "p12" else None)
                        t1.record()
                        torch.cuda.synchronize()
                        times[form].append(1000 * t0.elapsed_time(t1) / copies)
                out.append((N, K, copies, times))
                del Ws, Ps
                torch.cuda.empty_cache()
        q.put((rank, out, tp.custom_timed_out()))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as ex:  # noqa: BLE001
        import traceback

        q.put((rank, repr(ex) + traceback.format_exc(), True))


def main():
    import statistics

    import torch.multiprocessing as mp

    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="NxK of a rank's shard, comma separated")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1)
    a = ap.parse_args()
    a.shape_list = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, a, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=900) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
    for rank, out, tmo in res:
        if isinstance(out, str) or tmo:
            print(f"rank {rank} failed (spin timed out: {tmo}): {out}", flush=True)
            sys.exit(1)
    print(f"us per launch, M = {a.rows}, two ranks on CU halves, cold weights; per run, then median and spread "
          "(max - min); the slower rank of each run", flush=True)
    for i, (N, K, copies, _) in enumerate(res[0][1]):
        t = {f: [max(r[1][i][3][f][j] for r in res) for j in range(a.runs)] for f in ("bf16", "p12")}
        med = {f: statistics.median(v) for f, v in t.items()}
        spread = max(max(v) - min(v) for v in t.values())
        gain = med["bf16"] - med["p12"]
        verdict = "keeps its twin" if gain > spread else "STAYS BF16 (no gain beyond the spread)"
        print(f"{N}x{K} ({copies} copies): bf16 {[round(v, 2) for v in t['bf16']]} median {med['bf16']:.2f} | "
              f"p12 {[round(v, 2) for v in t['p12']]} median {med['p12']:.2f} | ratio {med['p12'] / med['bf16']:.3f}, "
              f"gain {gain:.2f} us, spread {spread:.2f} us: {verdict}", flush=True)


if __name__ == "__main__":
    main()
