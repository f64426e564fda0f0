"""fp16 windows of 129..256 rows, on the host: enable_fused (asked with untuned_fp16=True: the launch shapes were swept in bf16), SJDBatchEngine and
LlamaGenSolver.slots_for accept fp16 at 256 rows as they accept bf16; rows above 256 are still refused with the limit named, and what was packed for
128 rows behaves as before."""
import pytest
import torch

import sjd_amd.backbones as BB
import sjd_amd.ops as ops
from sjd_amd.engine_batch import SJDBatchEngine
from sjd_amd.llamagen_solver import LlamaGenSolver
from tests.helpers import make_llamagen

TINY = dict(dim=128, n_layer=2, n_head=2, vocab_size=16384, block_size=64, cls_token_num=1, model_type="c2i", num_classes=1000)


def _fp16(max_rows=256):
    return make_llamagen(TINY, 3, 0.25, None, dtype=torch.float16).enable_fused(ops, gemm="sjd", max_rows=max_rows, untuned_fp16=True)


def test_enable_fused_accepts_fp16_at_256_rows():
    cls = BB.LlamaGenBackbone
    h, b = _fp16(), make_llamagen(TINY, 3, 0.25, None, dtype=torch.bfloat16).enable_fused(ops, gemm="sjd", max_rows=256)
    assert h.G1_CFG == b.G1_CFG == cls.G1_CFG_LLAMAGEN_256ROW and tuple(h.HEAD_CFG) == tuple(b.HEAD_CFG) == cls.HEAD_CFG_256ROW
    assert h.max_rows == h._fused_rows == 256 and h._packed[0]["qkv"].dtype == torch.float16 and h._packed_head.dtype == torch.float16
    with pytest.raises(ValueError, match="max_rows is 64, 128 or 256"):
        make_llamagen(TINY, 3, 0.25, None, dtype=torch.float16).enable_fused(ops, gemm="sjd", max_rows=512, untuned_fp16=True)
    with pytest.raises(ValueError, match="untuned_fp16=True"):          # the plain call keeps its refusal and names the way in
        make_llamagen(TINY, 3, 0.25, None, dtype=torch.float16).enable_fused(ops, gemm="sjd", max_rows=256)


def test_batch_engine_accepts_fp16_at_256_rows(monkeypatch):
    h = _fp16()
    # (the guards sit in front of every device allocation: stop the constructor right behind them)
    class _Passed(Exception):
        pass

    def stop(*a, **k):
        raise _Passed
    monkeypatch.setattr(ops, "BlobArray", stop)
    for n_prompts in (5, 8):                                        # 160 and 256 rows
        with pytest.raises(_Passed):
            SJDBatchEngine(h, 16384, "cpu", n_prompts)
    with pytest.raises(ValueError, match="at most 256 rows"):
        SJDBatchEngine(h, 16384, "cpu", 9)                          # 288 rows
    with pytest.raises(ValueError, match=r"= 160.*max_rows=256, untuned_fp16=True"):
        SJDBatchEngine(_fp16(128), 16384, "cpu", 5)                 # packed for 128 rows: the packing rule, and the call that lifts it


def test_slots_for_gives_fp16_eight_slots():
    h = _fp16()
    h.max_num_new_tokens = 16
    s = LlamaGenSolver(h, 1000, 1.0)
    assert s.slots_for(20, 2) == 8 and s.slots_for(20, 1) == 16 and s.slots_for(5, 2) == 5
    h.max_num_new_tokens = 32
    assert s.slots_for(20, 2) == 4                                  # 4 x 2 x 32 = 256 rows
    h128 = _fp16(128)                                               # packed for 128 rows: decodes with the slots it had before
    h128.max_num_new_tokens = 16
    assert LlamaGenSolver(h128, 1000, 1.0).slots_for(20, 2) == 4


def test_wrappers_refuse_mixed_16bit_types_on_the_host():
    import sjd_amd._lib as L
    x = torch.zeros(160, 64, dtype=torch.float16)
    wp = ops.pack_weight(torch.zeros(32, 64, dtype=torch.bfloat16), 64, True)
    with pytest.raises(L.SjdLibraryError, match="packed from"):
        ops.skinny_gemm(x, wp, 32, 64, 64, waves=4, step_major=True)
    with pytest.raises(L.SjdLibraryError, match="packed from"):
        ops.skinny_gemm_cols(x, wp, 32, 64, 64, 0, 32, waves=4, step_major=True)
