"""Every instantiated geometry of the decode GEMV once (the lists of csrc/kernels/gemv_geom.h), at the smallest
shape that selects it: the bf16 launch against the oracle, the 12- and 13-bit launches equal to it bit for bit.
Each case asserts its geometry through ``ops.gemv_plan``, so it cannot quietly test another one."""

import pytest
import torch

from llm_consensus_amd import ops
from llm_consensus_amd.ops import (EPI_AR, EPI_BF16, EPI_COMBINE, EPI_RESADD, EPI_ROPE, EPI_SILU, GEMV_AR, GEMV_DENSE,
                                   GEMV_MOE_COMBINE, GEMV_MOE_PAIR, WF_BF16, WF_P12, WF_P13, oracle, wpack)
from llm_consensus_amd.utils.native import kernels
from test_kernels_gpu import _rope_setup, close

pytestmark = pytest.mark.gpu

BF = torch.bfloat16

# geometry -> (N, K, epilogue, rows the list has it for)
DENSE = {
    (256, 1, 8): (64, 2048, EPI_BF16, 4),
    (256, 2, 4): (36, 2048, EPI_SILU, 4),
    (512, 1, 4): (2048, 2048, EPI_BF16, 4),
    (640, 1, 4): (2050, 2048, EPI_BF16, 4),
    (768, 1, 4): (2562, 2048, EPI_BF16, 4),
    (1024, 1, 4): (3074, 2048, EPI_BF16, 4),
    (896, 1, 4): (2072, 2048, EPI_SILU, 4),
    (640, 1, 8): (2560, 8192, EPI_BF16, 2),
    (1024, 1, 8): (4096, 8192, EPI_BF16, 2),
    (768, 2, 4): (6144, 2048, EPI_ROPE, 2),
    (896, 2, 4): (7168, 2048, EPI_SILU, 2),
    (1024, 2, 4): (8192, 2048, EPI_SILU, 2),
}
AR = {
    (256, 1, 8): (64, 2048),
    (512, 1, 4): (2048, 2048),
    (640, 1, 4): (2050, 2048),
    (768, 1, 4): (2562, 2048),
    (1024, 1, 4): (3074, 2048),
    (640, 1, 8): (2560, 8192),
    (1024, 1, 8): (4096, 8192),
}
E = 4  # experts
MOE = {  # geometry -> (N, K, the epilogues the list has it for)
    (1024, 1, 4): (4096, 2048, (EPI_SILU, EPI_BF16)),
    (768, 1, 4): (3072, 2048, (EPI_SILU, EPI_BF16)),
    (640, 1, 4): (2560, 2048, (EPI_SILU, EPI_BF16)),
    (512, 1, 4): (2048, 2048, (EPI_SILU, EPI_BF16)),
    (256, 1, 4): (1536, 2048, (EPI_SILU, EPI_BF16)),
    (1024, 2, 4): (8192, 2048, (EPI_SILU,)),
    (896, 2, 4): (7168, 2048, (EPI_SILU,)),
    (896, 1, 4): (3584, 2048, (EPI_SILU,)),
    (256, 2, 4): (102, 2048, (EPI_SILU,)),
}


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8),
                                                                    b.contiguous().view(torch.uint8))


def _weights(N, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(N, K, generator=g, device="cuda") * K ** -0.5).to(BF)


def _planned(op, M, N, K, epi, geom, wf=WF_BF16, unroll=None):
    want = geom[:2] + (geom[2] if unroll is None else unroll, True)
    assert ops.gemv_plan(op, M, N, K, epi, wf) == want, (op, M, N, K, epi, wf)


@pytest.mark.parametrize("geom,M", [(g, M) for g in sorted(DENSE) for M in (1, 2, 3) if M <= DENSE[g][3]])
def test_dense_geometry(cuda, geom, M):
    N, K, epi, _ = DENSE[geom]
    if M == 3:
        K += 8  # off the MFMA form's 128-k tiles: three rows on the VALU form (bf16 only)
    _planned(GEMV_DENSE, M, N, K, epi, geom)
    torch.manual_seed(M * 7 + N + K + epi)
    x = torch.randn(M, K, device="cuda").to(BF)
    W = _weights(N, K, N + K)
    twins = []
    if M <= 2:
        p12, p13 = wpack.pack12(W), wpack.pack(W)
        assert p12.raw_share <= wpack.MAX_RAW_SHARE and p13.raw_share <= wpack.MAX_RAW_SHARE
        _planned(GEMV_DENSE, M, N, K, epi, geom, WF_P12,
                 4 if (M == 2 and geom == (1024, 1, 8) and epi == EPI_ROPE) else None)
        _planned(GEMV_DENSE, M, N, K, epi, geom, WF_P13)
        twins = [p12, p13]
    if epi == EPI_ROPE:
        nh, nkv, D = 32, 8, 128
        assert N == (nh + 2 * nkv) * D
        cos_t, sin_t, _, pos, slots, kc, vc = _rope_setup(nh, nkv, D, M)
        nw = torch.randn(K, device="cuda").to(BF)

        def run(Wp):
            kd, vd = kc.cuda(), vc.cuda()
            qd = torch.zeros(M, nh * D, dtype=BF, device="cuda")
            ops.qkv_rope(x, W, nw, 1e-5, qd, kd, vd, pos.cuda(), slots.cuda(), cos_t.cuda(), sin_t.cuda(), nh, nkv, D,
                         64, Wp=Wp)
            torch.cuda.synchronize()
            return qd, kd, vd

        got = run(None)
        kc_ref, vc_ref = kc.clone(), vc.clone()
        q_ref = torch.zeros(M, nh * D, dtype=BF)
        qkv = oracle.linear(x.cpu(), W.cpu(), 0, None, nw.cpu(), 1e-5)
        oracle.rope_kv_write(qkv, pos, cos_t, sin_t, kc_ref, vc_ref, slots, nh, nkv, D, 64, q_ref)
        for a, b in zip(got, (q_ref, kc_ref, vc_ref)):
            close(a, b, 3e-2)
        for Wp in twins:
            assert all(_bits(a, b) for a, b in zip(run(Wp), got)), type(Wp).__name__
        return
    y = ops.gemv(x, W, epi)
    close(y, oracle.linear(x.cpu(), W.cpu(), epi, None), 2e-2)
    for Wp in twins:
        assert _bits(ops.linear(x, W, epi, Wp=Wp), y), type(Wp).__name__


@pytest.fixture(scope="module")
def one_rank():
    """A fused all-reduce buffer of a group of one: the launch exchanges with nobody and h += W . x."""
    from llm_consensus_amd.parallel.custom_ar import FUSED_CAP

    if not torch.cuda.is_available():  # set up before the function-scoped `cuda` fixture
        pytest.skip("no GPU")
    k = kernels()
    own = k.car_alloc(FUSED_CAP)
    host, host_dev = k.car_host_alloc()
    yield own, host_dev, FUSED_CAP
    torch.cuda.synchronize()
    k.car_free(own)
    k.car_host_free(host)


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("geom", sorted(AR))
def test_fused_allreduce_geometry(cuda, one_rank, geom, M):
    N, K = AR[geom]
    own, host_dev, cap = one_rank
    _planned(GEMV_AR, M, N, K, EPI_AR, geom)
    # packed EPI_AR: two rows on 16 waves run 4 loads per lane
    _planned(GEMV_AR, M, N, K, EPI_AR, geom, WF_P12, 4 if (M == 2 and geom == (1024, 1, 8)) else None)
    torch.manual_seed(M + N + K)
    x = torch.randn(M, K, device="cuda").to(BF)
    h0 = torch.randn(M, N, device="cuda").to(BF)
    W = _weights(N, K, N + K + 1)
    pw = wpack.pack12(W)
    assert pw.raw_share <= wpack.MAX_RAW_SHARE
    k, st, p = kernels(), torch.cuda.current_stream().cuda_stream, lambda t: t.data_ptr()
    hb, hp = h0.clone(), h0.clone()
    k.gemv_ar(M, p(x), x.stride(0), p(W), p(hb), hb.stride(0), N, K, [own], host_dev, 0, 1, cap, st)
    launched = k.gemv_ar_p12(M, p(x), x.stride(0), p(W), p(pw.planes), p(pw.hdr), p(hp), hp.stride(0), N, K, [own],
                             host_dev, 0, 1, cap, st)
    torch.cuda.synchronize()
    assert launched  # not the -8 fall-back
    close(hb, oracle.linear(x.cpu(), W.cpu(), EPI_RESADD, h0.cpu().clone()), 2e-2)
    assert _bits(hp, hb)


def _moe_case(N, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    W = (torch.randn(E, N, K, generator=g, device="cuda") * K ** -0.5).to(BF)
    pw = wpack.pack12_experts(W)
    assert pw.raw_share <= wpack.MAX_RAW_SHARE
    return W, pw, torch.tensor([[3, 1]], dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("geom,epi", [(g, e) for g in sorted(MOE) for e in MOE[g][2]])
def test_moe_pair_geometry(cuda, geom, epi):
    N, K, _ = MOE[geom]
    _planned(GEMV_MOE_PAIR, 1, N, K, epi, geom)
    _planned(GEMV_MOE_PAIR, 1, N, K, epi, geom, WF_P12)
    W, pw, ids = _moe_case(N, K, N + K + epi)
    silu = epi == EPI_SILU
    torch.manual_seed(N + epi)
    # gate_up reads the token's hidden row through the norm prologue, down the pair's activation
    x = torch.randn(1 if silu else 2, K, device="cuda").to(BF)
    nw = (1.0 + 0.1 * torch.randn(K, device="cuda")).to(BF) if silu else None

    def run(Wp):
        out = torch.full((2, N // 2 if silu else N), -7.0, dtype=BF, device="cuda")
        ops.moe_gemv(x, W, ids, 2 if silu else 1, out, N, K, epi, norm_w=nw, Wp=Wp)
        torch.cuda.synchronize()
        return out

    y = run(None)
    for pair, e in enumerate(ids[0].tolist()):
        xr = x[0 if silu else pair].cpu().unsqueeze(0)
        ref = oracle.linear(xr, W[e].cpu(), epi, None, nw.cpu() if silu else None, 1e-5)
        close(y[pair:pair + 1], ref, 3e-2 if silu else 2e-2)
    assert _bits(run(pw), y)


def test_moe_combine_geometry(cuda):
    N, K, geom = 4096, 2048, (1024, 2, 4)
    _planned(GEMV_MOE_COMBINE, 2, N, K, EPI_COMBINE, geom)
    _planned(GEMV_MOE_COMBINE, 2, N, K, EPI_COMBINE, geom, WF_P12)
    W, pw, ids = _moe_case(N, K, 5)
    torch.manual_seed(6)
    act = torch.randn(2, K, device="cuda").to(BF)
    w = torch.rand(1, 2, device="cuda", dtype=torch.float32)
    h0 = torch.randn(1, N, device="cuda").to(BF)

    def run(Wp):
        h = h0.clone()
        ops.moe_down_combine(act, W, ids, w, h, N, K, Wp=Wp)
        torch.cuda.synchronize()
        return h

    y = run(None)
    ref = h0.float().cpu()
    for j, e in enumerate(ids[0].tolist()):
        ref = ref + float(w[0, j]) * (act[j].float().cpu() @ W[e].float().cpu().t())
    close(y, ref, 2e-2)
    assert _bits(run(pw), y)
