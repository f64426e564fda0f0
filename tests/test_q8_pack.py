"""The 8-bit (OCP e4m3fn) weight stream of kernels G1q / G1sq on the host: sjd_amd.ops.quantize_e4m3 (where all the loss is) and
ops.pack_weight_q8 / PackedQ8 (a permutation).  The error bounds follow from the format -- 3 mantissa bits, round to nearest even:
half an ulp is 2^-4 relative for normal codes (|w| / scale >= 2^-6), half the denormal spacing 2^-9 otherwise -- not from what the code
gives.  CPU only (the GPU side is tests/test_gpu_q8.py)."""
import numpy as np
import pytest
import torch

import sjd_amd.ops as ops

FP8 = torch.float8_e4m3fn


def seeded_matrix():
    """[96, 80] bf16 with a zero column, a column whose amax is exactly 448 * 2^-3, a column of 1e-6-sized values and a few 37.0 outliers
    (a `column` is an output column of the projection = a row of the weight)"""
    g = torch.Generator().manual_seed(1234)
    w = (torch.randn(96, 80, generator=g) * 0.05)
    w[7] = 0.0
    w[11] = torch.randn(80, generator=g).clamp(-1, 1) * 20.0
    w[11, 3] = 56.0                                              # 448 * 2^-3
    w[20] = torch.randn(80, generator=g) * 1e-6
    w[33, 5] = w[64, 79] = w[95, 0] = 37.0
    w[40, 2] = -0.0
    return w.to(torch.bfloat16)


def formula(w):
    """the issue's definition, restated with torch ops in float64"""
    wd = w.double()
    amax = wd.abs().amax(dim=1)
    scale = torch.where(amax > 0, torch.exp2(torch.ceil(torch.log2(amax / 448.0))), torch.ones_like(amax))
    q = (wd / scale[:, None]).float().to(FP8).view(torch.uint8)
    return q, scale.float()


def test_quantize_e4m3_formula_and_round_trip():
    w = seeded_matrix()
    q, scale = ops.quantize_e4m3(w)
    assert q.dtype == torch.uint8 and q.shape == w.shape and scale.dtype == torch.float32 and scale.shape == (96,)
    m, _ = torch.frexp(scale)
    assert bool((m == 0.5).all())                                # every scale is a power of two
    assert scale[7] == 1.0 and scale[11] == 0.125
    qf, sf = formula(w)
    assert torch.equal(scale, sf) and torch.equal(q, qf)
    assert not bool(((q & 0x7F) == 0x7F).any())                  # no NaN codes
    assert int((q[11] & 0x7F).max()) == 0x7E                     # the 448 code itself is reached
    assert q[40, 2] == 0x80                                      # -0.0 keeps its sign
    deq = q.view(FP8).float() * scale[:, None]
    assert torch.equal(deq.to(torch.bfloat16).float(), deq)      # q * scale is a bf16 number


def test_quantize_e4m3_error_bound():
    w = seeded_matrix()
    q, scale = ops.quantize_e4m3(w)
    wf = w.float()
    deq = q.view(FP8).float() * scale[:, None]
    err, s = (wf - deq).abs().double(), scale[:, None].double().expand_as(wf)
    normal = (wf.abs().double() / s) >= 2.0 ** -6
    assert bool(normal.any()) and bool((~normal).any())
    assert bool((err[normal] <= 2.0 ** -4 * wf.abs().double()[normal]).all())
    assert bool((err[~normal] <= s[~normal] * 2.0 ** -10).all())


def kernel_read(pq):
    """PackedQ8 -> e4m3 codes [N, K], walking the buffer with the address arithmetic of g1q_skinny_gemm (csrc/sjd_gemm_q8.h): a chunk starts at
    byte k0 * N; pair p of unit (c, t) at first + p * rsb, lane l reads 16 bytes at l * 16 = {k-step 2p, k-step 2p + 1}; the half record of an
    odd unit is 64 x 8 bytes behind the pairs"""
    N, K, KC, T = pq.N, pq.K, pq.KC, pq.N // 32
    data = pq.data.cpu().numpy()
    q = np.zeros((N, K), dtype=np.uint8)
    for k0 in range(0, K, KC):
        steps = min(KC, K - k0) // 16
        npf = steps // 2
        cb = k0 * N
        rsb = (T if pq.step_major else 1) * 1024
        for t in range(T):
            first = cb + (t * 1024 if pq.step_major else t * steps * 512)
            half = cb + (npf * T * 1024 + t * 512 if pq.step_major else t * steps * 512 + npf * 1024)
            for lane in range(64):
                n, kk = 32 * t + (lane & 31), k0 + 8 * (lane >> 5)
                for p in range(npf):
                    b = data[first + p * rsb + lane * 16: first + p * rsb + lane * 16 + 16]
                    q[n, kk + 32 * p: kk + 32 * p + 8] = b[:8]
                    q[n, kk + 32 * p + 16: kk + 32 * p + 24] = b[8:]
                if steps & 1:
                    q[n, kk + 16 * (steps - 1): kk + 16 * (steps - 1) + 8] = data[half + lane * 8: half + lane * 8 + 8]
    return torch.from_numpy(q)


@pytest.mark.parametrize("N,K,KC,step_major,gateup", [(96, 48, 32, False, False), (64, 528, 128, True, False), (128, 512, 256, True, True),
                                                      (64, 48, 32, True, False)])
def test_pack_weight_q8_layout(N, K, KC, step_major, gateup):
    g = torch.Generator().manual_seed(N + K)
    w = (torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-12, 3, (N, 1), generator=g).float())).to(torch.bfloat16)
    w[5] = 0.0
    q, scale = ops.quantize_e4m3(w)
    deq = (q.view(FP8).float() * scale[:, None]).to(torch.bfloat16)
    pq = ops.pack_weight_q8(w, KC, step_major, gateup=gateup)
    assert isinstance(pq, ops.PackedQ8) and (pq.N, pq.K, pq.KC, pq.step_major) == (N, K, KC, step_major)
    assert pq.nbytes() == N * K + 4 * N == pq.data.numel() and pq.numel() == N * K and pq.data.dtype == torch.uint8 and pq.data.is_contiguous()
    assert (N * K) % 512 == 0 and torch.equal(pq.data[N * K:].view(torch.float32), scale)
    assert pq.dequant().dtype == torch.bfloat16
    assert torch.equal(pq.dequant().view(torch.int16), deq.view(torch.int16))          # bit for bit (the sign of -0.0 included)
    assert torch.equal(kernel_read(pq), q)                                             # ... and where the kernel looks for every byte
    st = pq.stats
    wf = w.float()
    assert st["rel_rms_error"] == pytest.approx(float((wf - deq.float()).pow(2).mean().sqrt() / wf.pow(2).mean().sqrt()), rel=1e-5)
    assert 0 < st["rel_rms_error"] < 2.0 ** -4                   # every element is within half an ulp of 3 mantissa bits, or tiny
    assert st["scale_exp_min"] == int(torch.log2(scale).min()) and st["scale_exp_max"] == int(torch.log2(scale).max())


def test_pack_weight_q8_record_order_is_pack_weight():
    """one byte per weight in pack_weight's (chunk, tile, k-step, lane, element) order: with an even step count per chunk, un-pairing the k-steps
    gives pack_weight of the codes"""
    g = torch.Generator().manual_seed(5)
    w = torch.randn(64, 128, generator=g).to(torch.bfloat16)
    q, _ = ops.quantize_e4m3(w)
    for sm in (False, True):
        pq = ops.pack_weight_q8(w, 64, sm)
        ref = ops.pack_weight(q, 64, sm)                          # uint8 stream, records of 512 bytes
        body = pq.data[:64 * 128]
        if sm:
            got = body.reshape(2, 2, 2, 64, 2, 8).permute(0, 1, 4, 2, 3, 5)      # [c, p, t, lane, ks, j] -> [c, p, ks, t, lane, j]
        else:
            got = body.reshape(2, 2, 2, 64, 2, 8).permute(0, 1, 2, 4, 3, 5)      # [c, t, p, lane, ks, j] -> [c, t, p, ks, lane, j]
        assert torch.equal(got.reshape(-1), ref)


def test_scale_exponent_is_clamped_so_that_no_dequantised_value_is_a_bf16_denormal():
    """columns whose amax is below 448 * 2^-117 keep the scale 2^-117 (the formula would go on down): the smallest code magnitude 2^-9 times the
    scale is then 2^-126, the smallest NORMAL bf16 number; values below half of that quantise to zero"""
    w = torch.zeros(32, 32)
    w[0, 0], w[0, 1] = 2.0 ** -112, -2.0 ** -126         # amax 2^-112 < 448 * 2^-117 = 1.75 * 2^-109
    w[1, 0] = 2.0 ** -130                                # below half the smallest code at the clamped scale
    w[2, 0] = 448 * 2.0 ** -117                          # exactly at the clamp: the formula and the clamp agree
    w[3, 0] = 2.0 ** -100                                # above it: the formula
    w = w.to(torch.bfloat16)
    assert float(w[1, 0]) == 2.0 ** -130                 # (a bf16 denormal on the input side)
    q, scale = ops.quantize_e4m3(w)
    assert ops.Q8_MIN_SCALE_EXP == -117
    assert scale[0] == 2.0 ** -117 and scale[1] == 2.0 ** -117 and scale[2] == 2.0 ** -117 and scale[3] == 2.0 ** -108 and scale[4] == 1.0
    deq = q.view(FP8).float() * scale[:, None]
    assert deq[0, 0] == 2.0 ** -112 and deq[0, 1] == -2.0 ** -126 and deq[1, 0] == 0 and deq[2, 0] == 448 * 2.0 ** -117
    nz = deq[deq != 0].abs()
    assert float(nz.min()) >= 2.0 ** -126                # every nonzero dequantised value is a normal bf16 number
    assert torch.equal(deq.to(torch.bfloat16).float(), deq)
    assert torch.equal(ops.pack_weight_q8(w, 32).dequant().float(), deq)


def test_step_major_packing_is_the_same_bytes_under_any_chunking_of_whole_pairs():
    """what lets a 33..64-row window read a gate|up packed in two K halves in chunks half as long (PackedQ8.reads_as, ChameleonBackbone._q8_chunk)"""
    g = torch.Generator().manual_seed(9)
    w = torch.randn(64, 256, generator=g).to(torch.bfloat16)
    a, b, c = ops.pack_weight_q8(w, 128, True), ops.pack_weight_q8(w, 64, True), ops.pack_weight_q8(w, 96, True)
    assert torch.equal(a.data, b.data) and torch.equal(a.data, c.data)
    assert a.reads_as(64) and a.reads_as(96) and a.reads_as(128) and not a.reads_as(48)
    t = ops.pack_weight_q8(w, 128, False)
    assert not torch.equal(t.data, ops.pack_weight_q8(w, 64, False).data) and t.reads_as(128) and not t.reads_as(64)
    assert torch.equal(ops.pack_weight(w, 128, True), ops.pack_weight(w, 64, True))          # the 16-bit stream of the twin has the same property
    odd = ops.pack_weight_q8(w[:, :240], 128, True)                                            # K not a multiple of 32: a half record somewhere
    assert not odd.reads_as(64) and odd.reads_as(128)


def test_q8_refusals():
    w = torch.randn(32, 32)
    with pytest.raises(ValueError, match="bf16"):
        ops.quantize_e4m3(w.to(torch.float16))
    with pytest.raises(ValueError, match="bf16"):
        ops.pack_weight_q8(w.to(torch.float16), 32)
    bad = w.to(torch.bfloat16)
    bad[0, 0] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        ops.quantize_e4m3(bad)
    assert ops.gateup_silu_ok(32, 128, 1024, 512, packed_q8=True) and not ops.gateup_silu_ok(33, 128, 1024, 512, packed_q8=True)
    assert not ops.gateup_silu_ok(32, 128, 1024, 256, packed_q8=True)
