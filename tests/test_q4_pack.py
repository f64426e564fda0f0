"""CPU: the MXFP4 weight format of kernels G1q4 / G1sq4 -- ops.quantize_mxfp4 (where ALL the loss of the format is), ops.pack_weight_q4 /
ops.PackedQ4 (a permutation, checked by reading the packed bytes back) and the launch-shape sets that go with it.  The GPU side has no tolerance
(tests/test_gpu_q4.py); the quantiser's error bound here is derived from the e2m1 grid, not measured:
    the grid is {0, 0.5, 1, 1.5, 2, 3, 4, 6} * scale -- step 0.5 up to 2, 1 up to 4, 2 up to 6 -- and amax <= 6 * scale, so round-to-nearest is off by
    at most half a step: <= scale / 4 where |w| <= 2 scale, <= scale / 2 <= |w| / 4 where 2 scale <= |w|, <= scale <= |w| / 4 where 4 scale <= |w|.
    Hence |w - deq| <= max(scale, |w|) / 4 for every element."""
import pytest
import torch

import sjd_amd.launch_shapes as LS
import sjd_amd.ops as ops

G = ops.Q4_GRANULE
GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def gaussian(N, K, seed):
    return torch.randn(N, K, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16)


def many_binades(N, K, seed):
    """every block of 32 of a row at its own magnitude, 2^-30 .. 2^10: the scales of one row spread over forty binades"""
    g = torch.Generator().manual_seed(seed)
    mag = torch.exp2(torch.randint(-30, 11, (N, K // 32), generator=g).float()).repeat_interleave(32, dim=1)
    return (torch.randn(N, K, generator=g) * mag).to(torch.bfloat16)


def split(codes, se):
    """(nibbles [N, K], scale [N, K] fp32)"""
    N, K = codes.shape[0], 2 * codes.shape[1]
    nib = torch.stack([codes & 0xF, codes >> 4], dim=2).reshape(N, K)
    return nib, torch.exp2(se.float() - 127).repeat_interleave(32, dim=1)


def reference_dequant(codes, se):
    nib, scale = split(codes, se)
    return torch.where((nib & 8) != 0, -1.0, 1.0) * GRID[(nib & 7).long()] * scale


@pytest.mark.parametrize("make", [gaussian, many_binades])
def test_scales_are_powers_of_two_that_cover_the_block_and_the_bound_holds(make):
    w = make(64, 512, 3)
    codes, se = ops.quantize_mxfp4(w)
    assert codes.shape == (64, 256) and codes.dtype == torch.uint8 and se.shape == (64, 16) and se.dtype == torch.uint8
    wf = w.float()
    _, scale = split(codes, se)
    amax = wf.reshape(64, 16, 32).abs().amax(dim=2)
    s_blk = torch.exp2(se.float() - 127)
    assert bool((amax <= 6 * s_blk).all())                                    # nothing saturates
    assert bool(((amax > 3 * s_blk) | (amax == 0) | (se == 127 + ops.Q4_MIN_SCALE_EXP)).all())          # ... and it is the SMALLEST such power of two
    deq = reference_dequant(codes, se)
    assert torch.equal(ops.dequantize_mxfp4(codes, se).float(), deq)          # code * scale is exactly a bf16 number
    err = (wf - deq).abs()
    assert bool((err <= torch.maximum(scale, wf.abs()) / 4).all()), float((err / torch.maximum(scale, wf.abs())).max())
    assert float(err.max()) > 0
    if make is many_binades:
        assert int(se.max()) - int(se.min()) >= 24 and len(set(se[0].tolist())) > 6


def test_zero_blocks_tiny_blocks_and_the_exponent_limits():
    w = torch.zeros(32, 128)
    w[1, 32:64] = 2.0 ** -133                          # a bf16 denormal block: the scale is floored at 2^-125, everything rounds to zero
    w[2, 0] = 2.0 ** -126                              # the smallest normal: 0.5 * 2^-125 exactly
    w[3, 5] = -6 * 2.0 ** 125                          # the largest magnitude the format holds
    w[4, 7] = -0.0
    w = w.to(torch.bfloat16)
    codes, se = ops.quantize_mxfp4(w)
    assert int(se[0, 0]) == 127 and bool((codes[0] == 0).all())               # a zero block: scale 1
    assert int(se[1, 1]) == 127 + ops.Q4_MIN_SCALE_EXP == 2 and bool((codes[1] == 0).all())
    assert int(se[2, 0]) == 2 and int(codes[2, 0]) == 0x01
    assert int(se[3, 0]) == 127 + ops.Q4_MAX_SCALE_EXP == 252 and int(codes[3, 2]) == 0xF0          # element 5: the high nibble of byte 2, code -6
    assert int(codes[4, 3]) == 0x80                                           # -0 keeps its sign
    deq = ops.dequantize_mxfp4(codes, se)
    assert torch.equal(deq[2:5].view(torch.int16), w[2:5].view(torch.int16))
    nz = deq.float().abs()[deq.float() != 0]
    assert bool((nz >= 2.0 ** -126).all())                                    # no bf16 denormals come out
    big = torch.zeros(32, 128, dtype=torch.bfloat16)
    big[0, 0] = 1.75 * 2.0 ** 127                      # above 6 * 2^125 = 1.5 * 2^127
    with pytest.raises(ValueError, match="2\\^125"):
        ops.quantize_mxfp4(big)
    with pytest.raises(ValueError, match="bf16"):
        ops.quantize_mxfp4(torch.zeros(32, 128, dtype=torch.float16))


def test_ties_round_to_the_even_code():
    for e in (-20, 0, 9):
        s = 2.0 ** e
        row = torch.zeros(32)
        ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
        row[:7] = torch.tensor(ties) * s
        row[7:14] = -torch.tensor(ties) * s
        row[14] = 6 * s                                 # pins the block's scale at s
        codes, se = ops.quantize_mxfp4(row[None].repeat(32, 1).to(torch.bfloat16))
        assert int(se[0, 0]) == 127 + e
        deq = ops.dequantize_mxfp4(codes, se)[0].float() / s
        want = torch.tensor([0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0])              # codes 0, 2, 2, 4, 4, 6, 6: the even neighbour
        assert torch.equal(deq[:7], want) and torch.equal(deq[7:14], -want)
        nib, _ = split(codes, se)
        assert nib[0, :7].tolist() == [0, 2, 2, 4, 4, 6, 6] and nib[0, 7:14].tolist() == [8, 10, 10, 12, 12, 14, 14]


PACK_CASES = [(32, G, G, False), (96, 3 * G, 2 * G, False), (96, 3 * G, 2 * G, True),          # a ragged last chunk of one granule
              (64, 1024, 256, True), (160, 512, 512, False),                                   # N = 160: a partial last workgroup at 2, 3, 4 .. tiles each
              (64, 2560, 2560, True)]


@pytest.mark.parametrize("N,K,KC,step_major", PACK_CASES)
def test_the_packed_buffer_reads_back_as_codes_times_scale(N, K, KC, step_major):
    w = many_binades(N, K, N + K)
    codes, se = ops.quantize_mxfp4(w)
    pq = ops.pack_weight_q4(w, KC, step_major)
    assert pq.data.dtype == torch.uint8 and pq.nbytes() == pq.data.numel() == N * K // 2 + N * K // 32
    assert (pq.N, pq.K, pq.KC, pq.step_major, pq.numel()) == (N, K, KC, step_major, N * K)
    assert torch.equal(pq.codes(), codes) and torch.equal(pq.scale_exp(), se)
    assert torch.equal(pq.dequant().float(), reference_dequant(codes, se))
    assert 0 < pq.stats["rel_rms_error"] < 0.25 and pq.stats["scale_exp_min"] == int(se.min()) - 127 and pq.stats["scale_exp_max"] == int(se.max()) - 127
    # the documented byte order, spot-checked without the inverse permutation: unit (chunk 0, tile t), record R, lane l = 32 h + r, k-step i of the record
    t, R, r, h, i = N // 32 - 1, 0, 5, 1, 2
    T = N // 32
    rec = (R * T + t) if step_major else t * (min(KC, K) // 64) + R
    got = pq.data[rec * 1024 + (32 * h + r) * 16 + 4 * i:][:4]
    k = 16 * (4 * R + i) + 8 * h
    assert torch.equal(got, codes[32 * t + r, k // 2:k // 2 + 4])
    sc0 = N * K // 2
    grp = t if step_major else t * (min(KC, K) // 128)          # trip 0 of tile t: [trip][tile] or [tile][trip]
    assert torch.equal(pq.data[sc0 + grp * 128 + 4 * r:][:4], se[32 * t + r, :4])


def test_gateup_packing_and_the_halved_chunk():
    w = many_binades(128, 1024, 9)                          # [Wg; Wu], I = 64
    for sm in (False, True):
        pq = ops.pack_weight_q4(w, 512, sm, gateup=True)
        assert torch.equal(pq.data, ops.pack_weight_q4(w, 512, sm).data)          # (the flag only asserts the two-K-halves shape)
        assert torch.equal(pq.dequant().float(), reference_dequant(*ops.quantize_mxfp4(w)))
    sm_pq = ops.pack_weight_q4(w, 512, True)
    assert sm_pq.reads_as(512) and sm_pq.reads_as(256) and sm_pq.reads_as(128) and not sm_pq.reads_as(192)
    assert torch.equal(sm_pq.data, ops.pack_weight_q4(w, 256, True).data)          # the same bytes under a halved chunk
    tm_pq = ops.pack_weight_q4(w, 512, False)
    assert tm_pq.reads_as(512) and not tm_pq.reads_as(256)
    assert not torch.equal(tm_pq.data, ops.pack_weight_q4(w, 256, False).data)


@pytest.mark.parametrize("K,KC", [(192, 128), (256, 192), (256, 64), (64, 64), (1024, 1000)])
def test_the_packer_refuses_what_is_not_whole_granules(K, KC):
    with pytest.raises(ValueError, match="multiples of 128"):
        ops.pack_weight_q4(gaussian(32, K, 1), KC)


@pytest.mark.parametrize("cfg,dims", [
    (LS.G1_CFG_Q4, dict(qkv=(3 * 4096, 4096), o=(4096, 4096), gate_up=(2 * 11008, 4096), down=(4096, 11008))),           # Lumina-mGPT 7B
    (LS.G1_CFG_EMU3_Q4, dict(qkv=(6144, 4096), o=(4096, 4096), gate_up=(2 * 14336, 4096), down=(4096, 14336)))])         # Emu3-Gen 8B
def test_the_launch_shape_sets_fit_the_format(cfg, dims):
    assert G == LS.Q4_GRANULE == 128 and LS.q4_chunk_errors(cfg, dims) == []
    for name, (KC, tiles, sm) in cfg.items():
        K = dims[name][1]
        assert K % G == 0 and KC % G == 0 and KC <= LS.CHUNK_CAP_32ROW == 2560
        for T in (32, 33, 64):
            kc = LS.chunk_for_rows(name, cfg[name], T, K, "mxfp4", 64)
            assert LS.CHUNK_CAP_64ROW == 1280 and kc % G == 0 and kc <= (2560 if T <= 32 else 1280)
            assert kc == KC or sm                              # a halved chunk reads a step-major packing only
            assert kc == LS.chunk_for_rows(name, cfg[name], T, K, "mxfp4_as_bf16", 64)
    hid, inter = dims["gate_up"][1], dims["gate_up"][0] // 2
    fused32 = LS.gateup_silu_ok(32, inter, hid, cfg["gate_up"][0], packed_q8=True)
    assert fused32 == (2 * cfg["gate_up"][0] == hid)           # Lumina: two K halves of 2048 -> G1sq4; Emu3's chunks of 1024 -> G1q4 + F3
    assert not LS.gateup_silu_ok(33, inter, hid, cfg["gate_up"][0], packed_q8=True)
    assert LS.default_shapes(torch.bfloat16, None, None, False, cfg is LS.G1_CFG_EMU3_Q4, True, "mxfp4", None, 65536)[0] == cfg
    assert LS.default_shapes(torch.bfloat16, None, None, False, cfg is LS.G1_CFG_EMU3_Q4, True, "mxfp4_as_bf16", 64, 65536)[0] == cfg
    assert LS.q4_chunk_errors(dict(cfg, qkv=(1000, 6, True)), dims) == [("qkv", "granule")]
    assert LS.q4_chunk_errors(dict(cfg, qkv=(4096, 6, True)), dims) == [("qkv", "chunk")]
    assert LS.q4_chunk_errors(dict(cfg, down=(1408, 8, True)), dims) == [("down", "halved")]          # 704 is no multiple of 128
    assert LS.q4_chunk_errors(dict(cfg, gate_up=(2048, 8, False)), dims) == [("gate_up", "halved")]   # tile-major: no halved chunk reads it
