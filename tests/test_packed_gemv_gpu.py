"""The decode GEMV on the 13-bit packed weight planes (gemv_core.h WF_P13, wpack.hip).

The packed launch picks the bf16 launch's geometry and feeds the decoded chunks to the same
dot-product chain in the same order, so its output must equal the bf16 GEMV's BIT FOR BIT: for 1
and 2 rows, at the smallest shapes that reach each geometry branch, with raw rows (streamed from
the bf16 tensor) planted, over repeated launches and a graph replay. The HIP packer must write the
plain-torch reference's bytes.
"""

import functools

import pytest
import torch

from llm_consensus_amd import ops
from llm_consensus_amd.ops import EPI_BF16, EPI_F32, EPI_RESADD, EPI_ROPE, EPI_SILU, wpack

pytestmark = pytest.mark.gpu

NH, NKV, D, BS = 32, 8, 128, 64  # the EPI_ROPE case: (NH + 2 NKV) D = 6144 rows

# (N, K, epilogue, norm prologue)                 geometry branch
SHAPES = [
    (6144, 2048, EPI_ROPE, True),                # 768 threads x 2 rows per wave
    (7168, 2048, EPI_SILU, True),                # 896 x 2
    (4096, 8192, EPI_RESADD, False),             # 8 loads per lane, two units per batch
    (4096, 10240, EPI_RESADD, False),            # ... with an odd number of units: the masked tail
    (4096, 4096, EPI_RESADD, False),             # 1024 x 1, 4 loads per lane
    (1536, 4096, EPI_F32, True),                 # short output: 4-wave blocks
    (100, 2048, EPI_BF16, False),                # N off the block size, one unit in a two-unit batch
]
IDS = [f"{n}x{k}-epi{e}" for n, k, e, _ in SHAPES]


def _equal_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8),
                                                                    b.contiguous().view(torch.uint8))


@functools.lru_cache(maxsize=None)
def _weights(N, K, planted):
    """(W, packed twin) on the GPU; ``planted``: raw rows first, last and one of a row pair."""
    g = torch.Generator(device="cuda").manual_seed(N * 31 + K)
    W = (torch.randn(N, K, generator=g, device="cuda") * K ** -0.5).to(torch.bfloat16)
    rows = []
    if planted:
        rows = [0, N - 1, (N // 2) | 1]
        for i, r in enumerate(rows):
            W[r, (37 * i + 5) % K] = 0.0
    pw = wpack.pack(W)
    hdr = pw.hdr[:N].cpu()
    for r in rows:
        assert int(hdr[r]) == wpack.RAW
    assert len(rows) <= pw.raw_rows <= len(rows) + N // 100  # the planted ones; Gaussian rows are rarely raw
    return W, pw


def _inputs(M, K):
    g = torch.Generator(device="cuda").manual_seed(M * 7 + K)
    x = torch.randn(M, K, generator=g, device="cuda").to(torch.bfloat16)
    nw = (1.0 + 0.1 * torch.randn(K, generator=g, device="cuda")).to(torch.bfloat16)
    return x, nw


class _Case:
    """One (shape, M): ``run(Wp)`` launches the GEMV into fresh outputs and returns them."""

    def __init__(self, N, K, epi, norm, M, planted):
        self.N, self.K, self.epi, self.M = N, K, epi, M
        self.W, self.pw = _weights(N, K, planted)
        self.x, nw = _inputs(M, K)
        self.nw = nw if norm else None
        dev = self.x.device
        if epi == EPI_ROPE:
            self.pos = torch.tensor([5, 70][:M], dtype=torch.int32, device=dev)
            self.slots = torch.tensor([3 * BS + 5, 1 * BS + 6][:M], dtype=torch.int32, device=dev)
            ang = torch.arange(128, device=dev).float().view(-1, 1) * (0.5 ** torch.arange(D // 2, device=dev).float())
            self.cos_t, self.sin_t = ang.cos().contiguous(), ang.sin().contiguous()
            self.out = [torch.zeros(M, NH * D, dtype=torch.bfloat16, device=dev),
                        torch.zeros(4, NKV, BS, D, dtype=torch.bfloat16, device=dev),
                        torch.zeros(4, NKV, BS, D, dtype=torch.bfloat16, device=dev)]
        elif epi == EPI_RESADD:
            g = torch.Generator(device="cuda").manual_seed(11)
            self.h0 = torch.randn(M, N, generator=g, device=dev).to(torch.bfloat16)
            self.out = [torch.empty_like(self.h0)]
        else:
            n_out = N // 2 if epi == EPI_SILU else N
            self.out = [torch.zeros(M, n_out, dtype=torch.float32 if epi == EPI_F32 else torch.bfloat16, device=dev)]

    def launch(self, Wp):
        if self.epi == EPI_ROPE:
            q, kc, vc = self.out
            ops.qkv_rope(self.x, self.W, self.nw, 1e-5, q, kc, vc, self.pos, self.slots, self.cos_t, self.sin_t,
                         NH, NKV, D, BS, Wp=Wp)
        elif self.epi == EPI_RESADD:
            self.out[0].copy_(self.h0)
            ops.linear(self.x, self.W, EPI_RESADD, out=self.out[0], Wp=Wp)
        else:
            ops.linear(self.x, self.W, self.epi, out=self.out[0], norm_w=self.nw, eps=1e-5, Wp=Wp)

    def run(self, Wp):
        for o in self.out:
            o.zero_()
        self.launch(Wp)
        torch.cuda.synchronize()
        return [o.clone() for o in self.out]


@pytest.mark.parametrize("planted", [False, True], ids=["packed", "raw-rows"])
@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_packed_gemv_bits(cuda, shape, M, planted):
    N, K, epi, norm = shape
    c = _Case(N, K, epi, norm, M, planted)
    want = c.run(None)
    assert any(bool(w.float().abs().sum() > 0) for w in want)  # the reference wrote something
    # repeated launches
    for _ in range(3):
        got = c.run(c.pw)
        for g, w in zip(got, want):
            assert _equal_bits(g, w), f"max |diff| {(g.float() - w.float()).abs().max().item()}"
    # graph replay
    for o in c.out:
        o.zero_()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c.launch(c.pw)  # warm-up outside capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            c.launch(c.pw)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        if epi != EPI_RESADD:  # (the captured RESADD launch restores h itself)
            for o in c.out:
                o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for g, w in zip(c.out, want):
            assert _equal_bits(g, w)


@pytest.mark.parametrize("N,K", [(100, 2048), (1536, 4096), (64, 6144)])
def test_hip_packer_matches_reference(cuda, N, K):
    g = torch.Generator().manual_seed(N + K)
    W = (torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16)
    W[0] = 0.0                      # packable, base 0
    W[1, 9] = 0.0                   # raw
    W[2, 3] = float("inf")          # raw
    W[3, K - 1] = float("nan")      # raw
    W[N - 1, 0] = 0.0               # raw, last row
    W[5] = W[5].abs()               # signs all clear
    W[6] = -W[6].abs()              # signs all set
    ref = wpack.pack_reference(W)
    got = wpack.pack(W.to(cuda))
    assert got.raw_rows == ref.raw_rows == 4
    assert torch.equal(got.hdr.cpu(), ref.hdr)
    assert torch.equal(got.planes.cpu(), ref.planes)
    assert _equal_bits(wpack.unpack_reference(got, W.to(cuda)).cpu(), W)


def test_packed_entry_rejects_what_it_does_not_cover(cuda):
    W, pw = _weights(100, 2048, False)
    x, _ = _inputs(3, 2048)
    # 3 rows read bf16 (ops.linear's rule), whatever twin is passed: same bits as without
    assert _equal_bits(ops.linear(x, W, EPI_BF16, Wp=pw), ops.linear(x, W, EPI_BF16))
    from llm_consensus_amd.utils.native import kernels

    out = torch.zeros(3, 100, dtype=torch.bfloat16, device=cuda)
    with pytest.raises(RuntimeError):
        kernels().gemv_p13(3, x.data_ptr(), 2048, 0, 1e-5, W.data_ptr(), pw.planes.data_ptr(), pw.hdr.data_ptr(),
                           out.data_ptr(), 100, 100, 2048, EPI_BF16, torch.cuda.current_stream().cuda_stream)
