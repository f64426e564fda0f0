"""Several LlamaGen prompts per forward, on the host: the refusals of SJDBatchEngine and LlamaGenSolver.generate with their messages, the
launch-shape set chosen by enable_fused(max_rows=...), sample(generator=...), the library's version / mode constants and the example's
arguments."""
import importlib.util
import os
import re

import pytest
import torch

import sjd_amd._lib as L
import sjd_amd.backbones as BB
import sjd_amd.ops as ops
from sjd_amd.engine import WindowSpec
from sjd_amd.engine_batch import SJDBatchEngine
from sjd_amd.llamagen_solver import LlamaGenSolver, sample
from tests.helpers import make_llamagen

TINY = dict(dim=128, n_layer=2, n_head=2, vocab_size=16384, block_size=64, cls_token_num=1, model_type="c2i", num_classes=1000)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_max_rows_chooses_the_shape_set():
    cls = BB.LlamaGenBackbone
    base = make_llamagen(TINY, 3, 0.25, None, dtype=torch.bfloat16).enable_fused(ops, gemm="sjd")
    same = make_llamagen(TINY, 3, 0.25, None, dtype=torch.bfloat16).enable_fused(ops, gemm="sjd", max_rows=64)
    assert base.G1_CFG == cls.G1_CFG_LLAMAGEN and base.HEAD_CFG == cls.HEAD_CFG and "HEAD_CFG" not in base.__dict__ and base.max_rows == 64
    for a, b in zip(base._packed, same._packed):                     # the default packs exactly what max_rows=64 packs (and what it packed before)
        assert all(torch.equal(a[k], b[k]) for k in a)
    assert torch.equal(base._packed_head, same._packed_head)
    for rows in (128, 256):
        m = make_llamagen(TINY, 3, 0.25, None, dtype=torch.bfloat16).enable_fused(ops, gemm="sjd", max_rows=rows)
        want, head = getattr(cls, f"G1_CFG_LLAMAGEN_{rows}ROW"), getattr(cls, f"HEAD_CFG_{rows}ROW")
        assert m.G1_CFG == want and tuple(m.HEAD_CFG) == head and m.max_rows == rows
        assert all(c[1] in cls.G1_WIDE_TILES for c in list(want.values()) + [head])        # column-tile counts kernel G1w takes
        assert all(-(-k // c[0]) <= 8 for c, k in ((want["qkv"], 1280), (want["o"], 1280), (want["gate_up"], 1280), (want["down"], 3584), (head, 1280)))
        fold = (m._fused[0].float() * m.layers[0].ffn_norm.weight.float()[None, :]).to(torch.bfloat16)
        assert torch.equal(m._packed[0]["gate_up"], ops.pack_weight(fold, want["gate_up"][0], want["gate_up"][2]))
    with pytest.raises(ValueError, match="max_rows is 64, 128 or 256"):
        make_llamagen(TINY, 3, 0.25, None, dtype=torch.bfloat16).enable_fused(ops, gemm="sjd", max_rows=96)
    with pytest.raises(ValueError, match="fp16 windows of at most 128 rows"):
        make_llamagen(TINY, 3, 0.25, None, dtype=torch.float16).enable_fused(ops, gemm="sjd", max_rows=256)


def test_forward_window_row_limit_follows_max_rows(monkeypatch):
    m = make_llamagen(TINY, 3, 0.25, None, dtype=torch.bfloat16).enable_fused(ops, gemm="sjd", max_rows=128)
    took = []
    monkeypatch.setattr(m, "_forward_window_g1", lambda *a, **k: took.append("g1"))
    monkeypatch.setattr(m, "forward_embeds", lambda *a, **k: took.append("aten"))
    for rows in (64, 128, 144):
        m.forward_window(torch.zeros(rows // 16, 16, dtype=torch.long), None, 0, None)
    assert took == ["g1", "g1", "aten"]


def test_batch_engine_guards():
    m = make_llamagen(TINY, 3, 0.25, None, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match=r"enable_fused\(ops, gemm='sjd', max_rows="):
        SJDBatchEngine(m, 16384, "cpu", 2)                                               # not fused
    m.enable_fused(ops, gemm="sjd")
    with pytest.raises(ValueError, match=r"max_rows=64 rows.*= 96.*max_rows=128"):
        SJDBatchEngine(m, 16384, "cpu", 3)                                               # packed for 64 rows, 3 x 2 x 16 = 96
    m8 = make_llamagen(TINY, 3, 0.25, None, dtype=torch.bfloat16).enable_fused(ops, gemm="sjd", max_rows=128)
    with pytest.raises(ValueError, match=r"= 160.*max_rows=256"):
        SJDBatchEngine(m8, 16384, "cpu", 5)
    h = make_llamagen(TINY, 3, 0.25, None, dtype=torch.float16).enable_fused(ops, gemm="sjd", max_rows=128)
    with pytest.raises(ValueError, match="fp16 windows of at most 128 rows"):
        SJDBatchEngine(h, 16384, "cpu", 5)
    with pytest.raises(ValueError, match="at most 256 rows"):
        SJDBatchEngine(m8, 16384, "cpu", 9)                                              # (the 256-row limit as before)


def test_window_spec_conditioning_fields_default_to_none():
    s = WindowSpec(first_tokens=None, first_positions=None, key_start=torch.zeros(2, dtype=torch.int32), pos_offset=torch.zeros(2, dtype=torch.long))
    assert s.cond_embeds is None and s.cond_sampling is None and s.kv_base == 0


def test_sample_generator_argument():
    lg = torch.randn(3, 2, 500, generator=torch.Generator().manual_seed(1))
    torch.manual_seed(11)
    want = torch.multinomial(torch.softmax(lg[:, -1, :].clone(), -1), 1)
    torch.manual_seed(11)
    a, pa = sample(lg.clone(), top_k=0, top_p=1.0)
    torch.manual_seed(11)
    b, pb = sample(lg.clone(), top_k=0, top_p=1.0, generator=None)
    assert torch.equal(a, want) and torch.equal(a, b) and torch.equal(pa, pb)            # default: today's global-generator draw, bit for bit
    g = torch.Generator().manual_seed(5)
    st = torch.get_rng_state()
    c, _ = sample(lg.clone(), top_k=50, top_p=0.9, generator=g)
    assert torch.equal(torch.get_rng_state(), st)                                        # the global generator is left alone
    d, _ = sample(lg.clone(), top_k=50, top_p=0.9, generator=torch.Generator().manual_seed(5))
    assert torch.equal(c, d)
    e, _ = sample(lg.clone(), sample_logits=False, generator=g)
    assert torch.equal(e, lg[:, -1, :].argmax(-1, keepdim=True))


def test_solver_refusals_for_several_prompts():
    m = make_llamagen(TINY, 3, 0.25, None, dtype=torch.bfloat16)
    m.do_cfg, m.guidance_scale, m.max_num_new_tokens = True, 4.0, 16
    cond = torch.tensor([1, 2, 3])
    with pytest.raises(ValueError, match=r"3 prompts runs on the fused HIP path only.*enable_fused.*one prompt per call"):
        LlamaGenSolver(m, 1000, 1.0).generate(cond, 64, None, cfg_scale=4.0)
    m.enable_fused(ops, gemm="sjd", max_rows=128)
    with pytest.raises(ValueError, match=r"noise_device='cpu'.*one prompt per call"):
        LlamaGenSolver(m, 1000, 1.0, noise_device="cpu").generate(cond, 64, None, cfg_scale=4.0)
    with pytest.raises(ValueError, match="must match do_cfg"):
        LlamaGenSolver(m, 1000, 1.0).generate(cond, 64, None, cfg_scale=1.0)
    s = LlamaGenSolver(m, 1000, 1.0)
    assert s.prompts_per_forward is None and s.slots_for(5, 2) == 5 and s.slots_for(20, 2) == 8 and s.slots_for(20, 1) == 16
    assert LlamaGenSolver(m, 1000, 1.0, prompts_per_forward=2).slots_for(5, 2) == 2
    h = make_llamagen(TINY, 3, 0.25, None, dtype=torch.float16)
    h.max_num_new_tokens = 16
    assert LlamaGenSolver(h, 1000, 1.0).slots_for(20, 2) == 4                            # fp16: 128 rows


def test_lib_version_and_mode_constants():
    hdr = open(os.path.join(ROOT, "include", "sjd_hip.h")).read()
    assert int(re.search(r"#define SJD_VERSION (\d+)", hdr).group(1)) == 104
    assert L.load().sjd_version() == 104
    assert L.F2_ROPE_TABLE == int(re.search(r"#define SJD_F2_ROPE_TABLE (0x[0-9a-f]+)", hdr).group(1), 16) == 0x200
    assert "64 < B*n <= 256" in hdr


def test_example_arguments():
    spec = importlib.util.spec_from_file_location("llamagen_c2i_example", os.path.join(ROOT, "examples", "llamagen_c2i.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    a = ex.parse_args([])
    assert a.class_id == [207] and a.prompts_per_forward is None and ex.out_paths("s.png", a.class_id) == ["s.png"]
    a = ex.parse_args(["--fused", "--class-id", "207", "1", "980", "--out", "g.png"])
    assert a.class_id == [207, 1, 980] and ex.out_paths(a.out, a.class_id) == ["g_207.png", "g_1.png", "g_980.png"]
    assert ex.out_paths("g.png", [5, 5]) == ["g_5_0.png", "g_5_1.png"]
    with pytest.raises(SystemExit):
        ex.parse_args(["--class-id", "1", "2"])                                          # several labels need --fused
