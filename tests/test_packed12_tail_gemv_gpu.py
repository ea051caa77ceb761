"""The decode GEMV on 12-bit packed planes whose rows end in a tail (gemv_core.h WF_P12 with TAIL,
wpack.hip "P12 with a tail"): K a multiple of 512 off the 2048-weight unit.

The tail's chunks are decoded, patched and summed after the last whole unit's, which is the order in
which the bf16 loop sums a lane's chunks, so ``ops.linear`` / ``ops.qkv_rope`` with the tail twin
must return the bits of the same call without it: 1 and 2 rows, repeated launches, a graph replay.
The shapes are the smallest that reach each geometry branch with a tail; exceptions are planted
(zeros and tiny values) at every position class the tail adds, and the records must show that each
row took the intended path. The HIP packer must write the plain-torch reference's bytes.
"""

import functools

import pytest
import torch

from llm_consensus_amd import ops
from llm_consensus_amd.ops import EPI_BF16, EPI_F32, EPI_RESADD, EPI_ROPE, EPI_SILU, wpack

pytestmark = pytest.mark.gpu

D, BS = 128, 64
E = wpack.MAX_EXC

# (N, K, epilogue, norm prologue, (q heads, kv heads, q/k/v bias) of the RoPE cases)      geometry branch
SHAPES = [
    (6144, 2560, EPI_ROPE, True, (32, 8, False)),    # 768 threads x 2 rows per wave, U = 1, Q = 1
    (7168, 3072, EPI_SILU, True, None),              # 896 x 2, Q = 2
    (4096, 3584, EPI_RESADD, False, None),           # 1024 x 1, 4 loads per lane, Q = 3
    (4096, 8704, EPI_RESADD, False, None),           # 8 loads per lane (two units per batch), even U = 4, Q = 1
    (4096, 11776, EPI_RESADD, False, None),          # ... odd U = 5 (masked last batch), then Q = 3
    (1536, 2560, EPI_F32, True, None),               # 4-wave blocks, 8 loads: one unit in a two-unit batch, then the tail
    (100, 3584, EPI_BF16, False, None),              # N off the block size
    (4608, 3584, EPI_ROPE, True, (28, 4, True)),     # Qwen2.5-7B's qkv with its bias: 768 x 1
]
IDS = [f"{n}x{k}-epi{e}" for n, k, e, _, _ in SHAPES]

ROW_E, ROW_E1 = 20, 21  # a two-rows-per-wave pair: exactly E exceptions beside a raw partner (E + 1)


def _equal_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8),
                                                                    b.contiguous().view(torch.uint8))


def _plan(N, K):
    """{row: [k, ...]} of the planted exceptions. k = 512 q + 8 lane + element; T: the first tail weight."""
    T = K // 2048 * 2048
    # E + 1 positions in k order: E - 2 over the whole units, then three in the tail (two of them among the first E)
    spread = [(i * T) // (E - 2) + 3 * i for i in range(E - 2)] + [T + 5, T + 8 * 20 + 4, K - 2]
    assert len(spread) == E + 1 and spread == sorted(set(spread)) and sum(k >= T for k in spread[:E]) == 2
    return {
        0: [T, K - 1],                               # the first tail weight and the last weight
        1: [T + 8 * 5 + 1, T + 8 * 5 + 6],           # two in one lane's 8 weights
        2: [T + 8 * 3 + 2, T + 8 * 40 + 7],          # two in one tail chunk, different lanes
        3: [T - 512 + 8 * 10, T + 8 * 10 + 3],       # chunk 3 of the last whole unit, then tail chunk 0
        4: [100, K - 512 + 77],                      # a whole unit and the last tail chunk
        10: [T + 301],                               # one row of a two-rows-per-wave pair ...
        12: [K - 300], 13: [K - 200],                # ... and both rows of a pair
        ROW_E: spread[:E],
        ROW_E1: spread,
        N - 1: [K - 9],                              # the last row
    }


@functools.lru_cache(maxsize=None)
def _weights(N, K, planted):
    """(W, tail twin) on the GPU."""
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
    pw = wpack.pack12_tail(W)
    assert type(pw) is wpack.PackedWeight12Tail
    assert pw.planes.shape == (N, K // 2048 * 3072 + K % 2048 // 512 * 768)
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

    def __init__(self, N, K, epi, norm, heads, M, planted):
        self.N, self.K, self.epi, self.M = N, K, epi, M
        self.W, self.pw = _weights(N, K, planted)
        self.x, nw = _inputs(M, K)
        self.nw = nw if norm else None
        dev = self.x.device
        if epi == EPI_ROPE:
            self.nh, self.nkv, bias = heads
            assert (self.nh + 2 * self.nkv) * D == N
            g = torch.Generator(device="cuda").manual_seed(N)
            self.bias = torch.randn(N, generator=g, device=dev).to(torch.bfloat16) if bias else None
            self.pos = torch.tensor([5, 70][:M], dtype=torch.int32, device=dev)
            self.slots = torch.tensor([3 * BS + 5, 1 * BS + 6][:M], dtype=torch.int32, device=dev)
            ang = torch.arange(128, device=dev).float().view(-1, 1) * (0.5 ** torch.arange(D // 2, device=dev).float())
            self.cos_t, self.sin_t = ang.cos().contiguous(), ang.sin().contiguous()
            self.out = [torch.zeros(M, self.nh * D, dtype=torch.bfloat16, device=dev),
                        torch.zeros(4, self.nkv, BS, D, dtype=torch.bfloat16, device=dev),
                        torch.zeros(4, self.nkv, BS, D, dtype=torch.bfloat16, device=dev)]
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
                         self.nh, self.nkv, D, BS, Wp=Wp, bias=self.bias)
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
def test_packed12_tail_gemv_bits(cuda, shape, M, planted):
    N, K, epi, norm, heads = shape
    c = _Case(N, K, epi, norm, heads, M, planted)
    want = c.run(None)
    assert all(bool(w.float().abs().sum() > 0) for w in want)  # the reference wrote every output
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


@pytest.mark.parametrize("N,K", [(100, 2560), (1536, 3584), (64, 6656)])
def test_hip_tail_packer_matches_reference(cuda, N, K):
    g = torch.Generator().manual_seed(N + K)
    W = (torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16)
    for r, ks in _plan(N, K).items():
        for i, k in enumerate(ks):
            W[r, k] = [0.0, -0.0, 1e-30, -3e-33][i % 4]
    W[5] = 0.0                      # packable, base 0, no exceptions
    W[6, 3] = float("inf")          # raw
    W[7, K - 1] = float("nan")      # raw, the NaN in the tail
    W[8] = W[8].abs()               # signs all clear
    W[9] = -W[9].abs()              # signs all set
    W[11] = 1.5 * 2.0 ** -16        # a row whose best window is one step below the top-anchored one
    W[11, K - 3:] = 1.0             # ... its three large weights in the tail
    ref = wpack.pack12_tail_reference(W)
    got = wpack.pack12_tail(W.to(cuda))
    assert type(got) is wpack.PackedWeight12Tail
    assert got.raw_rows == ref.raw_rows and ref.raw_rows >= 3
    assert got.exceptions == ref.exceptions > 0
    assert torch.equal(got.hdr.cpu(), ref.hdr)
    assert int(ref.records()[11, 0]) == 55 | 3 << 8
    assert got.planes.shape == ref.planes.shape and torch.equal(got.planes.cpu(), ref.planes)
    assert got.nbytes() == wpack.packed12_tail_nbytes(N, K)
    assert _equal_bits(wpack.unpack12_tail_reference(got, W.to(cuda)).cpu(), W)
    # the bytes do not depend on timing: a second pack writes the same
    again = wpack.pack12_tail(W.to(cuda))
    assert torch.equal(again.hdr, got.hdr) and torch.equal(again.planes, got.planes)


def test_tail_entries_reject_what_they_do_not_cover(cuda):
    W, pw = _weights(100, 3584, False)
    x, _ = _inputs(3, 3584)
    # 3 rows read bf16 (ops.linear's rule), whatever twin is passed: same bits as without
    assert _equal_bits(ops.linear(x, W, EPI_BF16, Wp=pw), ops.linear(x, W, EPI_BF16))
    from llm_consensus_amd.utils.native import kernels

    st = torch.cuda.current_stream().cuda_stream
    out = torch.zeros(3, 100, dtype=torch.bfloat16, device=cuda)

    def gemv(M, K):
        kernels().gemv_p12(M, x.data_ptr(), 3584, 0, 1e-5, W.data_ptr(), pw.planes.data_ptr(), pw.hdr.data_ptr(),
                           out.data_ptr(), 100, 100, K, EPI_BF16, st)

    for M, K in ((1, 2304), (1, 1024), (3, 3584)):  # K off the wave chunk, no whole unit, 3 rows
        with pytest.raises(RuntimeError):
            gemv(M, K)
    with pytest.raises(RuntimeError):  # K beyond the 16-bit positions
        kernels().wpack12(W.data_ptr(), pw.planes.data_ptr(), pw.hdr.data_ptr(), out.data_ptr(), 1, 65536 - 512, st)
    with pytest.raises(ValueError):
        wpack.pack12_tail(torch.zeros(4, 1024, dtype=torch.bfloat16, device=cuda))
    with pytest.raises(ValueError):
        wpack.pack12_tail(torch.zeros(4, 4096, dtype=torch.bfloat16, device=cuda))
    gemv(1, 3584)  # the entry takes the shape itself
    torch.cuda.synchronize()
    assert _equal_bits(out[:1], ops.linear(x[:1], W, EPI_BF16))
