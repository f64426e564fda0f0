"""CPU: the 6-bit weight format of kernels G1q6 / G1sq6 -- ops.quantize_e2m3 (where ALL the loss of the format is) and ops.pack_weight_q6 /
ops.PackedQ6 (a permutation and a bit packing, checked by reading the packed bytes back).  The GPU side has no tolerance (tests/test_gpu_q6.py); the
quantiser's error bound here is derived from the e2m3 grid, not measured:
    the grid is {0 .. 1.875 in steps of 0.125, 2 .. 3.75 in steps of 0.25, 4 .. 7.5 in steps of 0.5} * scale and amax <= 7.5 * scale, so
    round-to-nearest is off by at most half a step: <= scale / 16 where |w| <= 2 scale, <= scale / 8 <= |w| / 16 where 2 scale <= |w|,
    <= scale / 4 <= |w| / 16 where 4 scale <= |w|.  Hence |w - deq| <= max(scale, |w|) / 16 for every element.
A scale block is (column n, 64-k record R, lane half h) = the weights at k = 64 R + 16 u + 8 h + j (u = 0..3, j = 0..7): scale_exp[n, 2 R + h]."""
import pytest
import torch

import sjd_amd.ops as ops

G = ops.Q4_GRANULE
GRID = torch.tensor([i * 0.125 for i in range(16)] + [2 + i * 0.25 for i in range(8)] + [4 + i * 0.5 for i in range(8)])


def gaussian(N, K, seed, sigma=1.0):
    return (torch.randn(N, K, generator=torch.Generator().manual_seed(seed)) * sigma).to(torch.bfloat16)


def block_of(k):
    """scale_exp column of weight column k"""
    return 2 * (k // 64) + (k % 16) // 8


BLOCK_COL = torch.tensor([block_of(k) for k in range(4096)])


def many_binades(N, K, seed):
    """every scale block of a row at its own magnitude, 2^-30 .. 2^10"""
    g = torch.Generator().manual_seed(seed)
    mag = torch.exp2(torch.randint(-30, 11, (N, K // 32), generator=g).float())[:, BLOCK_COL[:K]]
    return (torch.randn(N, K, generator=g) * mag).to(torch.bfloat16)


def scale_of(se, K):
    """fp32 [N, K]: every weight's scale"""
    return torch.exp2(se.float() - 127)[:, BLOCK_COL[:K]]


def reference_dequant(codes, se):
    return torch.where((codes & 32) != 0, -1.0, 1.0) * GRID[(codes & 31).long()] * scale_of(se, codes.shape[1])


def test_the_grid_is_e2m3s_32_magnitudes():
    assert GRID.tolist() == sorted(set(GRID.tolist())) and len(GRID) == 32 and float(GRID[-1]) == 7.5
    row = torch.zeros(64)
    pos = [k for k in range(64) if block_of(k) == 0]    # block (R 0, h 0) is k = 0..7, 16..23, 32..39, 48..55
    neg = [k for k in range(64) if block_of(k) == 1]
    assert pos == [16 * u + j for u in range(4) for j in range(8)] and neg == [k + 8 for k in pos]
    row[pos] = GRID
    row[neg] = -GRID
    codes, se = ops.quantize_e2m3(row[None].repeat(32, 1).to(torch.bfloat16))
    assert se[0].tolist() == [127, 127]                 # 7.5 is in both blocks
    assert codes[0, pos].tolist() == list(range(32)) and codes[0, neg].tolist() == list(range(32, 64))          # sign << 5 | exponent << 3 | mantissa
    deq = ops.dequantize_e2m3(codes, se)
    assert torch.equal(deq[0].float(), row) and int(deq[0, neg[0]].view(torch.int16)) == -32768          # -0 keeps its sign
    for c in range(64):                                 # the code's fields: sign, 2 exponent bits (bias 1), 3 mantissa bits
        e, m = (c >> 3) & 3, c & 7
        mag = m * 0.125 if e == 0 else (1 + m / 8) * 2.0 ** (e - 1)
        assert float(GRID[c & 31]) == mag


def test_ties_round_to_the_even_code_at_every_midpoint():
    mids = (GRID[:-1] + GRID[1:]) / 2                   # 31 midpoints, all bf16 numbers
    assert torch.equal(mids.to(torch.bfloat16).float(), mids)
    want = torch.tensor([i if i % 2 == 0 else i + 1 for i in range(31)])
    for e in (-20, 0, 9):
        s = 2.0 ** e
        row = torch.zeros(128)
        for h in (0, 1):                                # 31 ties and the block's 7.5 (which pins its scale at s), positive and negative: four blocks
            for sign, R in ((1.0, 0), (-1.0, 1)):
                ks = [64 * R + 16 * u + 8 * h + j for u in range(4) for j in range(8)]
                row[ks[:31]] = sign * mids * s
                row[ks[31]] = 7.5 * s
        codes, se = ops.quantize_e2m3(row[None].repeat(32, 1).to(torch.bfloat16))
        assert se[0].tolist() == [127 + e] * 4
        for h in (0, 1):
            for sign, R in ((0, 0), (32, 1)):
                ks = [64 * R + 16 * u + 8 * h + j for u in range(4) for j in range(8)]
                assert torch.equal(codes[0, ks[:31]].long(), want + sign), (e, h, R)
    # a value just under a binade's end rounds onto the next binade's first code
    row = torch.zeros(64)
    row[0], row[1], row[2], row[3] = 7.5, 1.96875, 3.9375, 1.9296875
    codes, _ = ops.quantize_e2m3(row[None].repeat(32, 1).to(torch.bfloat16))
    assert codes[0, :4].tolist() == [31, 16, 24, 15]


@pytest.mark.parametrize("make", [gaussian, many_binades])
def test_scales_are_powers_of_two_that_cover_the_block_and_the_bound_holds(make):
    N, K = 64, 512
    w = make(N, K, 3)
    codes, se = ops.quantize_e2m3(w)
    assert codes.shape == (N, K) and codes.dtype == torch.uint8 and se.shape == (N, K // 32) and se.dtype == torch.uint8 and int(codes.max()) < 64
    wf = w.float()
    scale = scale_of(se, K)
    amax = torch.zeros(N, K // 32).scatter_reduce(1, BLOCK_COL[:K][None].expand(N, K), wf.abs(), "amax")
    s_blk = torch.exp2(se.float() - 127)
    assert bool((amax <= 7.5 * s_blk).all())                                  # nothing saturates
    assert bool(((amax > 3.75 * s_blk) | (amax == 0) | (se == 127 + ops.Q6_MIN_SCALE_EXP)).all())          # ... and it is the SMALLEST such power of two
    deq = reference_dequant(codes, se)
    got = ops.dequantize_e2m3(codes, se)
    assert got.dtype == torch.bfloat16 and torch.equal(got.float(), deq)      # code * scale is exactly a bf16 number
    assert torch.equal(deq, deq.to(torch.bfloat16).float())
    err = (wf - deq).abs()
    assert bool((err <= torch.maximum(scale, wf.abs()) / 16).all()), float((err / torch.maximum(scale, wf.abs())).max())
    assert float(err.max()) > 0
    if make is many_binades:
        assert int(se.max()) - int(se.min()) >= 24 and len(set(se[0].tolist())) > 6


def test_outliers_zero_blocks_and_the_exponent_limits():
    w = gaussian(32, 256, 5, 0.02).float()
    for b in range(8):                                   # one outlier per block of row 0: forty times the rest
        w[0, [k for k in range(256) if block_of(k) == b][b]] = 0.9 * (-1) ** b
    w[1] = 0.0
    w[2, :] = 0.0
    w[2, 64:128] = 2.0 ** -133                           # bf16 denormal blocks: the scale is floored at 2^-123, everything rounds to zero
    w[3, :] = 0.0
    w[3, 0] = 2.0 ** -126                                # the smallest normal: 0.125 * 2^-123 exactly
    w[4, :] = 0.0
    w[4, 13] = -7.5 * 2.0 ** 125                         # the largest magnitude the format holds (k = 13: block h = 1 of record 0)
    w[5, 7] = -0.0
    w = w.to(torch.bfloat16)
    codes, se = ops.quantize_e2m3(w)
    deq = ops.dequantize_e2m3(codes, se)
    assert torch.equal(deq.float(), deq.to(torch.bfloat16).float()) and torch.equal(deq.float(), reference_dequant(codes, se))
    wf, scale = w.float(), scale_of(se, 256)
    assert bool(((wf - deq.float()).abs() <= torch.maximum(scale, wf.abs()) / 16).all())
    assert bool((wf.abs() <= 7.5 * scale).all())
    assert torch.equal(deq[0].float()[wf[0].abs() == 0.9], wf[0][wf[0].abs() == 0.9].sign() * 0.875)          # 0.9 = 7.2 * 2^-3 -> code 7 * 2^-3
    assert se[1].tolist() == [127] * 8 and bool((codes[1] == 0).all())          # zero blocks: scale 1
    assert se[2, 2:4].tolist() == [127 + ops.Q6_MIN_SCALE_EXP] * 2 == [4, 4] and bool((codes[2] == 0).all())
    assert int(se[3, 0]) == 4 and int(codes[3, 0]) == 1
    assert int(se[4, 1]) == 127 + ops.Q6_MAX_SCALE_EXP == 252 and int(codes[4, 13]) == 63 and int(se[4, 0]) == 127
    assert int(codes[5, 7]) == 32                                             # -0 keeps its sign
    assert torch.equal(deq[3:5].view(torch.int16), w[3:5].view(torch.int16)) and int(deq[5, 7].view(torch.int16)) == -32768
    nz = deq.float().abs()[deq.float() != 0]
    assert bool((nz >= 2.0 ** -126).all())                                    # no bf16 denormals come out
    big = torch.zeros(32, 128, dtype=torch.bfloat16)
    big[0, 0] = 1.9921875 * 2.0 ** 127                   # above 7.5 * 2^125 = 1.875 * 2^127
    with pytest.raises(ValueError, match="2\\^125"):
        ops.quantize_e2m3(big)
    with pytest.raises(ValueError, match="bf16"):
        ops.quantize_e2m3(torch.zeros(32, 128, dtype=torch.float16))
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.quantize_e2m3(torch.zeros(32, 96, dtype=torch.bfloat16))


@pytest.mark.parametrize("n,k", [(0, 0), (3, 8), (5, 17), (7, 63), (9, 64), (31, 250), (2, 41)])
def test_one_weight_moves_the_scale_of_its_block_and_no_other(n, k):
    w = gaussian(32, 256, 7, 0.02)
    _, se0 = ops.quantize_e2m3(w)
    w2 = w.clone()
    w2[n, k] = 100.0
    _, se1 = ops.quantize_e2m3(w2)
    changed = (se0 != se1).nonzero().tolist()
    assert changed == [[n, 2 * (k // 64) + (k % 16) // 8]]


PACK_CASES = [(32, G, G, False), (96, 3 * G, 2 * G, False), (96, 3 * G, 2 * G, True),          # a ragged last chunk of one granule
              (64, 1024, 256, True), (160, 512, 512, False), (64, 2560, 2560, True)]


@pytest.mark.parametrize("N,K,KC,step_major", PACK_CASES)
def test_the_packed_buffer_reads_back_as_codes_times_scale(N, K, KC, step_major):
    w = many_binades(N, K, N + K)
    codes, se = ops.quantize_e2m3(w)
    pq = ops.pack_weight_q6(w, KC, step_major)
    assert isinstance(pq, ops.PackedQ6) and isinstance(pq, ops._PackedQuant)
    assert pq.data.dtype == torch.uint8 and pq.nbytes() == pq.data.numel() == N * K * 3 // 4 + N * K // 32
    assert (pq.N, pq.K, pq.KC, pq.step_major, pq.numel()) == (N, K, KC, step_major, N * K)
    assert torch.equal(pq.codes(), codes) and torch.equal(pq.scale_exp(), se)
    assert torch.equal(pq.dequant().float(), reference_dequant(codes, se))
    assert 0 < pq.stats["rel_rms_error"] < 0.06 and pq.stats["scale_exp_min"] == int(se.min()) - 127 and pq.stats["scale_exp_max"] == int(se.max()) - 127
    # the documented byte order, spot-checked without the inverse permutation: unit (chunk 0, tile t), record R, lane l = 32 h + r
    t, R, r, h = N // 32 - 1, 1, 5, 1
    T = N // 32
    rec = (R * T + t) if step_major else t * (min(KC, K) // 64) + R
    lane = 32 * h + r
    raw = torch.cat([pq.data[rec * 1536 + lane * 16:][:16], pq.data[rec * 1536 + 1024 + lane * 8:][:8]])
    bits = sum(int(b) << (8 * i) for i, b in enumerate(raw.tolist()))
    for u in range(4):
        for j in range(8):
            assert (bits >> (6 * (8 * u + j))) & 63 == int(codes[32 * t + r, 64 * R + 16 * u + 8 * h + j])
    sc0 = N * K * 3 // 4
    grp = t if step_major else t * (min(KC, K) // 128)          # trip 0 of tile t: [trip][tile] or [tile][trip]
    assert torch.equal(pq.data[sc0 + grp * 128 + 4 * r:][:4], se[32 * t + r, :4])          # bytes: record 0 half 0, half 1, record 1 half 0, half 1


def test_gateup_packing_and_the_halved_chunk():
    w = many_binades(128, 1024, 9)                          # [Wg; Wu], I = 64
    for sm in (False, True):
        pq = ops.pack_weight_q6(w, 512, sm, gateup=True)
        assert torch.equal(pq.data, ops.pack_weight_q6(w, 512, sm).data)          # (the flag only asserts the two-K-halves shape)
        assert torch.equal(pq.dequant().float(), reference_dequant(*ops.quantize_e2m3(w)))
    sm_pq = ops.pack_weight_q6(w, 512, True)
    assert sm_pq.reads_as(512) and sm_pq.reads_as(256) and sm_pq.reads_as(128) and not sm_pq.reads_as(192)
    assert torch.equal(sm_pq.data, ops.pack_weight_q6(w, 256, True).data)          # the same bytes under a halved chunk
    tm_pq = ops.pack_weight_q6(w, 512, False)
    assert tm_pq.reads_as(512) and not tm_pq.reads_as(256)
    assert not torch.equal(tm_pq.data, ops.pack_weight_q6(w, 256, False).data)


@pytest.mark.parametrize("K,KC", [(192, 128), (256, 192), (256, 64), (64, 64), (1024, 1000)])
def test_the_packer_refuses_what_is_not_whole_granules(K, KC):
    with pytest.raises(ValueError, match="multiples of 128"):
        ops.pack_weight_q6(gaussian(32, K, 1), KC)


def test_the_packer_and_prefill_refusals():
    with pytest.raises(ValueError, match="bf16"):
        ops.pack_weight_q6(torch.zeros(32, 128, dtype=torch.float16), 128)
    pq = ops.pack_weight_q6(gaussian(32, 128, 2), 128)
    with pytest.raises(ValueError, match="no prefill kernel"):
        ops.prefill_gemm(torch.zeros(4, 128, dtype=torch.bfloat16), pq, 32, 128)


def test_the_error_figure_is_e4m3s_class():
    """bf16 Gaussian weights, sigma 0.02, 512 x 4096: 2.82 % (computed on the CPU when the format was proposed), against 2.66 % for e4m3 with a column
    scale and 11.8 % for MXFP4"""
    w = gaussian(512, 4096, 1234, 0.02)
    e6 = ops.pack_weight_q6(w, 2048, True).stats["rel_rms_error"]
    e4 = ops.pack_weight_q4(w, 2048, True).stats["rel_rms_error"]
    print(f"rel_rms_error: e2m3 {e6:.5f}, mxfp4 {e4:.5f}")
    assert abs(e6 - 0.0282) <= 0.002, e6
    assert e6 < e4 / 3, (e6, e4)
