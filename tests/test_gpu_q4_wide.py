"""GPU: kernel G1wq4 -- the MXFP4 form of G1w (csrc/sjd_gemm_wide.h, Q && WIDE) behind SJD_G1_W4_MXFP4 at 65..256 rows.  Nothing here has a
tolerance: the kernel rebuilds the bf16 MFMA operand code * scale bit for bit (g1q4_operand) and runs G1w's MFMA sequence, so every plane is
compared BIT FOR BIT with the uncompressed kernel on pack_weight(PackedQ4.dequant())."""
import ctypes

import pytest
import torch

from tests.test_gpu_q4 import BAD_ARG, UNSUPPORTED, W4, W8, q4_weight

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from tests.conftest import poison_device_memory
    poison_device_memory(total_gib=1)          # the planes come from torch.empty: an unwritten element must not read as zero
    return "cuda:0"


G1WQ4_CASES = [(65, 96, 128, 128, 3, False),             # first row past 64; one trip = one ring: the prologue's loads are all there is
               (96, 192, 384, 256, 6, True),             # two tiles per wave, ragged last chunk (one trip)
               (128, 160, 1408, 1408, 4, True),          # eleven trips, a workgroup with missing tiles
               (128, 64, 256, 128, 2, False),            # four row tiles x two tiles
               (129, 256, 512, 256, 8, True),            # XCD map (fewer than eight workgroups: its tail branch), two chunks
               (160, 288, 1024, 128, 3, False),          # eight chunks: whole rounds of eight workgroups
               (200, 128, 2048, 128, 2, True),           # sixteen chunks
               (256, 512, 1152, 384, 8, True),           # three chunks: plain map, the register-heaviest form
               (130, 288, 512, 128, 2, True)]            # XCD map with four chunks and a tail of four workgroups


@pytest.mark.parametrize("M,N,K,KC,tiles,step_major", G1WQ4_CASES)
def test_g1wq4_planes_are_g1w_on_the_dequantised_weight(dev, M, N, K, KC, tiles, step_major):
    import sjd_amd.ops as ops
    w = q4_weight(N, K, N + K + M, dev)
    pq = ops.pack_weight_q4(w, KC, step_major)
    wp = ops.pack_weight(pq.dequant(), KC, step_major)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(M)).to(torch.bfloat16).to(dev)
    ref = ops.skinny_gemm(x, wp, N, K, KC, tiles, step_major).data
    got = ops.skinny_gemm(x, pq, N, K, KC, tiles, step_major).data
    torch.cuda.synchronize()
    assert got.shape == ref.shape == ((K + KC - 1) // KC, 32 * ((M + 31) // 32), N)
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), (got - ref).abs().max()          # the whole planes, padding rows included
    assert float(ref.abs().max()) > 0
    if M % 32:
        assert float(got[:, M:].abs().max()) == 0
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ops.skinny_gemm(x, pq, N, K, KC, tiles, step_major)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        cap = ops.skinny_gemm(x, pq, N, K, KC, tiles, step_major).data
    cap.fill_(float("nan"))
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap.view(torch.int32), ref.view(torch.int32))


def test_g1wq4_column_window(dev):
    import sjd_amd.ops as ops
    M, NP, K, KC, c0, nc = 160, 512, 512, 256, 64, 352
    w = q4_weight(NP, K, 78, dev)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(4)).to(torch.bfloat16).to(dev)
    for sm, tiles in ((True, 4), (False, 6)):
        pq = ops.pack_weight_q4(w, KC, sm)
        full = ops.skinny_gemm(x, pq, NP, K, KC, tiles, sm).data
        ref = ops.skinny_gemm_cols(x, ops.pack_weight(pq.dequant(), KC, sm), NP, K, KC, c0, nc, tiles, sm).data
        got = ops.skinny_gemm_cols(x, pq, NP, K, KC, c0, nc, tiles, sm).data          # (tile0 = 2; the scales still sit at byte N_packed * K / 2)
        torch.cuda.synchronize()
        assert got.shape == (2, 160, nc) and torch.equal(got.view(torch.int32), full[:, :, c0:c0 + nc].contiguous().view(torch.int32))
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32)) and float(ref.abs().max()) > 0


def test_c_boundary_refusals_above_64_rows(dev):
    """with the bit set, what G1wq4 does not serve comes back as SJD_ERR_UNSUPPORTED before any launch"""
    import sjd_amd._lib as L
    lib = L.load()
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
    p = ctypes.c_void_p(buf.data_ptr())
    bf = L.DTYPE_BF16 | W4
    # sjd_skinny_gemm(x, w_packed, out, M, N, K, KC, waves, step_major, dtype, stream)
    for waves in (1, 5, 16):
        assert lib.sjd_skinny_gemm(p, p, p, 65, 32, 128, 128, waves, 0, bf, None) == UNSUPPORTED
        assert lib.sjd_skinny_gemm_cols(p, p, p, 65, 32, 128, 128, waves, 0, bf, 64, 0, None) == UNSUPPORTED
    assert lib.sjd_skinny_gemm(p, p, p, 70, 64, 128, 128, 2, 0, bf, None) == UNSUPPORTED              # three row tiles x two tiles: no G1w form
    assert lib.sjd_skinny_gemm(p, p, p, 70, 64, 192, 128, 3, 0, bf, None) == UNSUPPORTED              # K = 192: half a trip
    assert lib.sjd_skinny_gemm(p, p, p, 70, 64, 256, 64, 3, 0, bf, None) == UNSUPPORTED               # KC = 64
    assert lib.sjd_skinny_gemm_cols(p, p, p, 200, 32, 256, 64, 4, 1, bf, 64, 0, None) == UNSUPPORTED
    assert lib.sjd_skinny_gemm(p, p, p, 70, 64, 128, 128, 3, 0, L.DTYPE_F16 | W4, None) == UNSUPPORTED  # fp16
    assert lib.sjd_skinny_gemm_cols(p, p, p, 256, 32, 128, 128, 4, 0, L.DTYPE_F16 | W4, 64, 0, None) == UNSUPPORTED
    assert lib.sjd_skinny_gemm(p, p, p, 70, 64, 128, 128, 3, 0, bf | W8, None) == BAD_ARG             # both weight streams at once
    assert lib.sjd_skinny_gemm_cols(p, p, p, 256, 32, 128, 128, 4, 0, bf | W8, 64, 0, None) == BAD_ARG
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0
