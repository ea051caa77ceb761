"""The decode GEMV on the 12-bit packed weight planes (gemv_core.h WF_P12, wpack.hip).

The P12 twin of ``test_packed_gemv_gpu``: the same seven shapes (the smallest that reach each
geometry branch), 1 and 2 rows. The decoded chunk, patched with the row's exceptions, is the bf16
tensor's chunk and enters the same dot-product chain in the same order, so the output must equal
the bf16 GEMV's BIT FOR BIT, over repeated launches and a graph replay. Exceptions are planted
(zeros and tiny values, far below any 16-exponent window) at every position class the patch
distinguishes, and the row headers must show that each row took the intended path. The HIP packer
must write the plain-torch reference's bytes.
"""

import functools

import pytest
import torch

from llm_consensus_amd import ops
from llm_consensus_amd.ops import EPI_BF16, EPI_F32, EPI_RESADD, EPI_ROPE, EPI_SILU, wpack

pytestmark = pytest.mark.gpu

NH, NKV, D, BS = 32, 8, 128, 64  # the EPI_ROPE case: (NH + 2 NKV) D = 6144 rows
E = wpack.MAX_EXC

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

ROW_E, ROW_E1 = 20, 21  # rows with exactly E and E + 1 exceptions


def _equal_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8),
                                                                    b.contiguous().view(torch.uint8))


def _plan(N, K):
    """{row: [k, ...]} of the planted exceptions. k = 512 q + 8 lane + element."""
    last = K - 2048  # the last unit: the masked tail's only live unit at K = 10240
    spread = [(i * K) // (E + 1) + 3 * i for i in range(E + 1)]
    return {
        0: [0, K - 1],                               # first weight; lane 63, chunk 3, element 7 of the last unit
        1: [8 * 5 + 1, 8 * 5 + 6],                   # two in one 8-weight chunk of one lane
        2: [512 + 8 * 3 + 2, 512 + 8 * 40 + 7],      # two in one wave chunk, different lanes
        3: [1024 + 8 * 10, 1536 + 8 * 10 + 3],       # one in each of two consecutive chunks
        4: [last + 100],                             # the tail unit
        10: [777],                                   # one row of a two-rows-per-wave pair ...
        12: [300], 13: [300 + 512],                  # ... and both rows of a pair
        ROW_E: spread[:E],
        ROW_E1: spread,
        N - 1: [K // 2 + 1],                         # the last row
    }


@functools.lru_cache(maxsize=None)
def _weights(N, K, planted):
    """(W, P12 twin) on the GPU."""
    g = torch.Generator(device="cuda").manual_seed(N * 31 + K)
    W = (torch.randn(N, K, generator=g, device="cuda") * K ** -0.5).to(torch.bfloat16)
    plan = _plan(N, K) if planted else {}
    for r in (ROW_E, ROW_E1):
        if planted:  # one exponent: no exceptions of their own
            W[r] = ((1 + 0.9 * torch.rand(K, generator=g, device="cuda")) * K ** -0.5).to(torch.bfloat16)
    tiny = [0.0, -0.0, 1e-30, -3e-33]
    for r, ks in plan.items():
        for i, k in enumerate(ks):
            W[r, k] = tiny[i % 4]
    pw = wpack.pack12(W)
    assert isinstance(pw, wpack.PackedWeight12)
    rec = pw.records().cpu().to(torch.int64) & 0xFFFFFFFF
    base, cnt = rec[:, 0] & 0xFF, (rec[:, 0] >> 8) & 0xFF
    for r, ks in plan.items():
        if r == ROW_E1:
            assert int(base[r]) == wpack.RAW and int(cnt[r]) == 0
            continue
        assert int(base[r]) != wpack.RAW
        assert int(cnt[r]) == E if r == ROW_E else len(ks) <= int(cnt[r]) <= E
        listed = set((rec[r, 1:1 + int(cnt[r])] & 0xFFFF).tolist())
        assert set(ks) <= listed, (r, ks, listed)
    planted_raw = 1 if planted else 0  # Gaussian rows almost never have more than E exceptions
    assert planted_raw <= pw.raw_rows <= planted_raw + N // 100
    assert pw.raw_share <= wpack.MAX_RAW_SHARE
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


@pytest.mark.parametrize("planted", [False, True], ids=["packed", "planted"])
@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_packed12_gemv_bits(cuda, shape, M, planted):
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
def test_hip_packer12_matches_reference(cuda, N, K):
    g = torch.Generator().manual_seed(N + K)
    W = (torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16)
    for r, ks in _plan(N, K).items():
        for i, k in enumerate(ks):
            W[r, k] = [0.0, -0.0, 1e-30, -3e-33][i % 4]
    W[5] = 0.0                      # packable, base 0, no exceptions
    W[6, 3] = float("inf")          # raw
    W[7, K - 1] = float("nan")      # raw
    W[8] = W[8].abs()               # signs all clear
    W[9] = -W[9].abs()              # signs all set
    W[11] = 1.5 * 2.0 ** -16        # a row whose best window is one step below the top-anchored one
    W[11, :3] = 1.0
    ref = wpack.pack12_reference(W)
    got = wpack.pack12(W.to(cuda))
    assert got.raw_rows == ref.raw_rows and ref.raw_rows >= 3
    assert got.exceptions == ref.exceptions > 0
    assert torch.equal(got.hdr.cpu(), ref.hdr)
    assert int(ref.records()[11, 0]) == 55 | 3 << 8
    assert torch.equal(got.planes.cpu(), ref.planes)
    assert got.nbytes() == wpack.packed12_nbytes(N, K)
    assert _equal_bits(wpack.unpack12_reference(got, W.to(cuda)).cpu(), W)
    # the bytes do not depend on timing: a second pack writes the same
    again = wpack.pack12(W.to(cuda))
    assert torch.equal(again.hdr, got.hdr) and torch.equal(again.planes, got.planes)


def test_packed12_entry_rejects_what_it_does_not_cover(cuda):
    W, pw = _weights(100, 2048, False)
    x, _ = _inputs(3, 2048)
    # 3 rows read bf16 (ops.linear's rule), whatever twin is passed: same bits as without
    assert _equal_bits(ops.linear(x, W, EPI_BF16, Wp=pw), ops.linear(x, W, EPI_BF16))
    from llm_consensus_amd.utils.native import kernels

    st = torch.cuda.current_stream().cuda_stream
    out = torch.zeros(3, 100, dtype=torch.bfloat16, device=cuda)
    with pytest.raises(RuntimeError):  # 3 rows
        kernels().gemv_p12(3, x.data_ptr(), 2048, 0, 1e-5, W.data_ptr(), pw.planes.data_ptr(), pw.hdr.data_ptr(),
                           out.data_ptr(), 100, 100, 2048, EPI_BF16, st)
    with pytest.raises(RuntimeError):  # no records
        kernels().gemv_p12(1, x.data_ptr(), 2048, 0, 1e-5, W.data_ptr(), pw.planes.data_ptr(), 0,
                           out.data_ptr(), 100, 100, 2048, EPI_BF16, st)
    with pytest.raises(RuntimeError):  # K off the unit
        kernels().gemv_p12(1, x.data_ptr(), 2048, 0, 1e-5, W.data_ptr(), pw.planes.data_ptr(), pw.hdr.data_ptr(),
                           out.data_ptr(), 100, 100, 1024, EPI_BF16, st)
    with pytest.raises(RuntimeError):  # the RoPE epilogue has its own entry point
        kernels().gemv_p12(1, x.data_ptr(), 2048, 0, 1e-5, W.data_ptr(), pw.planes.data_ptr(), pw.hdr.data_ptr(),
                           out.data_ptr(), 100, 100, 2048, EPI_ROPE, st)
    with pytest.raises(RuntimeError):  # K beyond the 16-bit positions
        kernels().wpack12(W.data_ptr(), pw.planes.data_ptr(), pw.hdr.data_ptr(), out.data_ptr(), 1, 65536, st)
    with pytest.raises(ValueError):
        wpack.pack12(torch.zeros(4, 1024, dtype=torch.bfloat16, device=cuda))
    torch.cuda.synchronize()
