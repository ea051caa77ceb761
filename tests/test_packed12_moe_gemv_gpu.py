"""The MoE decode GEMVs on the 12-bit twin of the expert stack (gemv_core.h WF_P12 with EXPERT,
gemv_moe_p12.hip).

``test_packed12_gemv_gpu`` for the expert forms, E = 4 experts: the pair form (gate_up with the norm
prologue and the SiLU epilogue, the separate down GEMV) at the smallest (N, K) that reach each
geometry of ``moe_gemv_geom``, and the down projection fused with the top-2 combine. The twin is that of
the ``[E * N, K]`` view, so row n of expert e is its row e * N + n; the decoded and patched chunk is the
bf16 tensor's, in the bf16 loop's order, so the output must equal the bf16 expert launch's BIT FOR BIT,
for 1 and 2 tokens, over repeated launches and a graph replay after the ids were rewritten in place.
Exceptions are planted at every position class the patch distinguishes, in rows of different experts
(the last row of the last expert among them), and one raw row in expert 1 only, so the combine meets a
raw row beside a packed partner in both slot orders. The records must show that each planted row took
the intended path.
"""

import functools

import pytest
import torch

from llm_consensus_amd import ops
from llm_consensus_amd.ops import EPI_BF16, EPI_SILU, wpack
from llm_consensus_amd.utils.native import kernels

pytestmark = pytest.mark.gpu

E = 4
X = wpack.MAX_EXC
COMBINE = "combine"

# (N, K, form, norm prologue)                      geometry (threads x rows per wave)
SHAPES = [
    (8192, 2048, EPI_SILU, True),                 # gate_up: 1024 x 2
    (7168, 2048, EPI_SILU, True),                 # 896 x 2
    (4096, 2048, EPI_SILU, True),                 # 1024 x 1 (pairs meet through LDS)
    (3584, 2048, EPI_SILU, True),                 # 896 x 1
    (3072, 2048, EPI_SILU, True),                 # 768 x 1
    (2048, 2048, EPI_SILU, True),                 # 512 x 1
    (1536, 2048, EPI_SILU, True),                 # short output: 4-wave blocks
    (100, 2048, EPI_SILU, True),                  # 640 x 1, the only paired block that tiles 100 rows
    (102, 2048, EPI_SILU, True),                  # no paired block tiles: 256 x 2, N off the block
    (100, 2048, EPI_SILU, False),                 # ... and the SiLU form without the norm
    (4096, 4096, EPI_BF16, False),                # down, pair form: 1024 x 1, two units
    (2048, 6144, EPI_BF16, False),                # 512 x 1, an odd unit count
    (3072, 2048, EPI_BF16, False),                # 768 x 1
    (2560, 2048, EPI_BF16, False),                # 640 x 1
    (102, 2048, EPI_BF16, False),                 # 256 x 1, N off the block
    (4096, 2048, COMBINE, False),                 # down + combine: 1024 threads, a wave streams its row of both experts
    (2048, 6144, COMBINE, False),                 # an odd unit count
    (100, 4096, COMBINE, False),                  # N off the block
    (64, 14336, COMBINE, False),                  # Mixtral's K: the two x rows take 57 KB of LDS
]
IDS = [f"{n}x{k}-{f if f == COMBINE else 'epi%d' % f}{'-norm' if nm else ''}" for n, k, f, nm in SHAPES]

ROW_X, ROW_X1 = 20, 21  # rows with exactly MAX_EXC and MAX_EXC + 1 exceptions
RAW_EXPERT = 1          # the only expert with a (planted) raw row

# top-2 ids per token count, every list one launch: expert 0, expert E - 1, the raw row's expert in either slot
# order, and the same expert in both tokens
ID_SETS = {
    1: [[[0, 3]], [[3, 1]], [[1, 0]]],
    2: [[[1, 3], [3, 1]], [[0, 1], [0, 2]]],
}


def _equal_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8),
                                                                    b.contiguous().view(torch.uint8))


def _plan(N, K):
    """{(expert, row): [k, ...]} of the planted exceptions. k = 512 q + 8 lane + element."""
    last = K - 2048  # the last unit
    spread = [(i * K) // (X + 1) + 3 * i for i in range(X + 1)]
    return {
        (0, 0): [0, K - 1],                              # first weight; lane 63, chunk 3, element 7 of the last unit
        (1, 1): [8 * 5 + 1, 8 * 5 + 6],                  # two in one 8-weight chunk of one lane
        (2, 2): [512 + 8 * 3 + 2, 512 + 8 * 40 + 7],     # two in one wave chunk, different lanes
        (3, 3): [1024 + 8 * 10, 1536 + 8 * 10 + 3],      # one in each of two consecutive chunks
        (0, 4): [last + 100],                            # the last unit
        (2, 10): [777],                                  # one row of a two-row wave (pair form: rows 10, 11) ...
        (3, 12): [300], (3, 13): [300 + 512],            # ... both rows of one (pair form: rows 12, 13)
        (1, 12): [300 + 1024],                           # ... and both slots of a combine wave (experts 1 and 3, row 12)
        (0, ROW_X): spread[:X],
        (RAW_EXPERT, ROW_X1): spread,                    # raw: the combine streams bf16 for row 21 of both experts
        (E - 1, N - 1): [K // 2 + 1],                    # the last row of the last expert
    }


@functools.lru_cache(maxsize=None)
def _weights(N, K):
    """(W [E, N, K], its expert twin) on the GPU."""
    g = torch.Generator(device="cuda").manual_seed(N * 31 + K)
    W = (torch.randn(E, N, K, generator=g, device="cuda") * K ** -0.5).to(torch.bfloat16)
    plan = _plan(N, K)
    for er in ((0, ROW_X), (RAW_EXPERT, ROW_X1)):  # one exponent: no exceptions of their own
        W[er] = ((1 + 0.9 * torch.rand(K, generator=g, device="cuda")) * K ** -0.5).to(torch.bfloat16)
    tiny = [0.0, -0.0, 1e-30, -3e-33]
    for (e, r), ks in plan.items():
        for i, k in enumerate(ks):
            W[e, r, k] = tiny[i % 4]
    pw = wpack.pack12_experts(W)
    assert isinstance(pw, wpack.PackedExperts12) and (pw.E, pw.rows, pw.K) == (E, N, K)
    rec = pw.records().cpu().to(torch.int64) & 0xFFFFFFFF
    base, cnt = rec[:, 0] & 0xFF, (rec[:, 0] >> 8) & 0xFF
    for (e, n), ks in plan.items():
        r = e * N + n
        if (e, n) == (RAW_EXPERT, ROW_X1):
            assert int(base[r]) == wpack.RAW and int(cnt[r]) == 0
            continue
        assert int(base[r]) != wpack.RAW
        assert int(cnt[r]) == X if n == ROW_X else len(ks) <= int(cnt[r]) <= X
        listed = set((rec[r, 1:1 + int(cnt[r])] & 0xFFFF).tolist())
        assert set(ks) <= listed, (e, n, ks, listed)
    assert 1 <= pw.raw_rows <= 1 + N * E // 100  # the planted one; Gaussian rows almost never have more than X exceptions
    assert pw.raw_share <= wpack.MAX_RAW_SHARE
    others = (base.view(E, N) == wpack.RAW).sum(dim=1)
    assert int(others[RAW_EXPERT]) >= 1
    return W, pw


class _Case:
    """One (shape, T): ``run(ids, Wp)`` launches into fresh outputs and returns them."""

    def __init__(self, N, K, form, norm, T):
        self.N, self.K, self.form, self.T = N, K, form, T
        self.W, self.pw = _weights(N, K)
        g = torch.Generator(device="cuda").manual_seed(T * 7 + K)
        rows = T if form == EPI_SILU else 2 * T  # gate_up reads the token's hidden row, down the pair's activation
        self.x = torch.randn(rows, K, generator=g, device="cuda").to(torch.bfloat16)
        self.nw = (1.0 + 0.1 * torch.randn(K, generator=g, device="cuda")).to(torch.bfloat16) if norm else None
        self.ids = torch.zeros(T, 2, dtype=torch.int32, device="cuda")
        if form == COMBINE:
            self.w = torch.rand(T, 2, generator=g, device="cuda", dtype=torch.float32)
            self.h0 = torch.randn(T, N, generator=g, device="cuda").to(torch.bfloat16)
            self.out = torch.empty_like(self.h0)
        else:
            self.out = torch.zeros(2 * T, N // 2 if form == EPI_SILU else N, dtype=torch.bfloat16, device="cuda")

    def fill(self):
        if self.form == COMBINE:
            self.out.copy_(self.h0)
        else:
            self.out.fill_(-7.0)

    def launch(self, Wp):
        if self.form == COMBINE:
            ops.moe_down_combine(self.x, self.W, self.ids, self.w, self.out, self.N, self.K, Wp=Wp)
        elif self.form == EPI_SILU:
            ops.moe_gemv(self.x, self.W, self.ids, 2, self.out, self.N, self.K, EPI_SILU, norm_w=self.nw, Wp=Wp)
        else:
            ops.moe_gemv(self.x, self.W, self.ids, 1, self.out, self.N, self.K, EPI_BF16, Wp=Wp)

    def run(self, ids, Wp):
        self.ids.copy_(torch.tensor(ids, dtype=torch.int32))
        self.fill()
        self.launch(Wp)
        torch.cuda.synchronize()
        return self.out.clone()

    def packed_kernel_launched(self):
        """The packed entry itself on this shape: True when it launched a packed kernel (False: this geometry
        has none and ``ops`` launches the bf16 one)."""
        st, p = torch.cuda.current_stream().cuda_stream, lambda t: t.data_ptr() if t is not None else 0
        self.fill()
        if self.form == COMBINE:
            return kernels().moe_down_combine_p12(self.T, p(self.x), self.x.stride(0), p(self.W), p(self.pw.planes),
                                                  p(self.pw.hdr), p(self.ids), p(self.w), p(self.out),
                                                  self.out.stride(0), self.N, self.K, 2, st)
        silu = self.form == EPI_SILU
        return kernels().moe_gemv_p12(2 * self.T, p(self.x), self.x.stride(0), p(self.nw), 1e-5, p(self.W),
                                      p(self.pw.planes), p(self.pw.hdr), p(self.ids), 2 if silu else 1, p(self.out),
                                      self.out.stride(0), self.N, self.K, self.form, st)


@pytest.mark.parametrize("T", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_packed12_moe_gemv_bits(cuda, shape, T):
    N, K, form, norm = shape
    c = _Case(N, K, form, norm, T)
    sets = ID_SETS[T]
    want = [c.run(ids, None) for ids in sets]
    assert all(bool((w.float() != -7.0).all()) and bool(w.float().abs().sum() > 0) for w in want)
    assert c.packed_kernel_launched()  # every geometry of these shapes has its packed kernel
    torch.cuda.synchronize()
    # repeated launches (the combine from the same initial h)
    for ids, w in zip(sets, want):
        for _ in range(3):
            got = c.run(ids, c.pw)
            assert _equal_bits(got, w), f"ids {ids}: max |diff| {(got.float() - w.float()).abs().max().item()}"
    # one graph, captured on the first ids, replayed after the ids tensor was rewritten in place
    c.ids.copy_(torch.tensor(sets[0], dtype=torch.int32))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c.launch(c.pw)  # warm-up outside capture
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            c.launch(c.pw)
    torch.cuda.current_stream().wait_stream(s)
    for ids, w in list(zip(sets, want))[::-1]:
        c.ids.copy_(torch.tensor(ids, dtype=torch.int32))
        c.fill()
        graph.replay()
        torch.cuda.synchronize()
        assert _equal_bits(c.out, w), f"replay on ids {ids}"


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[11]], ids=[IDS[1], IDS[11]])
def test_a_pair_of_another_ranks_expert_is_left_untouched(cuda, shape):
    N, K, form, norm = shape
    c = _Case(N, K, form, norm, 2)
    for ids in ([[-1, 2], [1, -1]], [[3, -1], [-1, -1]]):
        want, got = c.run(ids, None), c.run(ids, c.pw)
        assert _equal_bits(got, want)
        for p, e in enumerate(sum(ids, [])):
            assert bool((got[p].float() == -7.0).all()) == (e < 0)


@pytest.mark.parametrize("N,K", [(100, 2048), (64, 6144)])
def test_hip_packer_writes_the_reference_expert_twin(cuda, N, K):
    W, pw = _weights(N, K)
    Wc = W.cpu()
    ref = wpack.pack12_experts(Wc)  # on the CPU: pack12_reference of the [E * N, K] view
    assert pw.raw_rows == ref.raw_rows >= 1 and pw.exceptions == ref.exceptions > 0
    assert torch.equal(pw.hdr.cpu(), ref.hdr) and torch.equal(pw.planes.cpu(), ref.planes)
    each = [wpack.pack12_reference(Wc[e]) for e in range(E)]
    assert torch.equal(pw.planes.cpu(), torch.cat([p.planes for p in each]))
    assert torch.equal(pw.hdr.cpu(), torch.cat([p.hdr for p in each]))
    assert pw.nbytes() == wpack.packed12_nbytes(E * N, K)
    assert _equal_bits(wpack.unpack12_reference(pw, W.view(E * N, K)).cpu(), Wc.view(E * N, K))
    assert isinstance(wpack.pack_best(W), wpack.PackedExperts12)


def test_packed_expert_entries_reject_what_they_do_not_cover(cuda):
    N, K = 100, 2048
    W, pw = _weights(N, K)
    c = _Case(N, K, EPI_BF16, False, 2)
    ids = [[1, 3], [3, 1]]
    want = c.run(ids, None)
    # a twin of another stack's shape, or three tokens: the bf16 launch, the same bits
    _, other = _weights(64, 6144)
    assert _equal_bits(c.run(ids, other), want)
    x3 = torch.randn(6, K, device=cuda).to(torch.bfloat16)
    ids3 = torch.tensor([[0, 1], [2, 3], [1, 0]], dtype=torch.int32, device=cuda)
    y = [torch.zeros(6, N, dtype=torch.bfloat16, device=cuda) for _ in range(2)]
    ops.moe_gemv(x3, W, ids3, 1, y[0], N, K, EPI_BF16, Wp=pw)
    ops.moe_gemv(x3, W, ids3, 1, y[1], N, K, EPI_BF16)
    assert _equal_bits(y[0], y[1])
    st, p = torch.cuda.current_stream().cuda_stream, lambda t: t.data_ptr()
    # no packed kernel for the norm prologue with the plain bf16 epilogue: nothing launched, reported as such
    c.fill()
    nw = torch.ones(K, dtype=torch.bfloat16, device=cuda)
    assert kernels().moe_gemv_p12(4, p(c.x), K, p(nw), 1e-5, p(W), p(pw.planes), p(pw.hdr), p(c.ids), 1, p(c.out), N,
                                  N, K, EPI_BF16, st) is False
    torch.cuda.synchronize()
    assert bool((c.out.float() == -7.0).all())
    with pytest.raises(RuntimeError):  # no records
        kernels().moe_gemv_p12(4, p(c.x), K, 0, 1e-5, p(W), p(pw.planes), 0, p(c.ids), 1, p(c.out), N, N, K, EPI_BF16, st)
    with pytest.raises(RuntimeError):  # K off the unit
        kernels().moe_gemv_p12(4, p(c.x), K, 0, 1e-5, p(W), p(pw.planes), p(pw.hdr), p(c.ids), 1, p(c.out), N, N, 1024,
                               EPI_BF16, st)
    w = torch.ones(2, 3, device=cuda)
    with pytest.raises(RuntimeError):  # top-3
        kernels().moe_down_combine_p12(2, p(c.x), K, p(W), p(pw.planes), p(pw.hdr), p(c.ids), p(w), p(c.out), N, N, K,
                                       3, st)
    with pytest.raises(ValueError):
        wpack.pack12_experts(torch.zeros(2, 4, 1024, dtype=torch.bfloat16, device=cuda))
    torch.cuda.synchronize()
