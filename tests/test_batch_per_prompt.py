"""CPU: the host side of per-prompt guidance scales / sampler settings in the several-prompt engine -- which SJDConfig fields may differ
between the prompts of one decode_many, the refusals, LlamaGenSolver.generate's per-prompt arguments, the new export's declaration."""
import ctypes
import dataclasses
import os
import re

import pytest
import torch

from tests.conftest import ROOT


def _cfgs(n, **kw):
    from sjd_amd.engine import SJDConfig
    return [SJDConfig(guidance_scale=3.0 + j, seed=10 * j, **kw) for j in range(n)]


def test_one_config_or_one_per_prompt():
    from sjd_amd.engine import SJDConfig
    from sjd_amd.engine_batch import per_prompt_configs
    one = SJDConfig(guidance_scale=4.0, seed=5)
    assert per_prompt_configs(one, 3) == (one, None)                       # today's call: nothing per prompt
    shared, cfgs = per_prompt_configs([one], 1)                            # one prompt, its config in a list: the same config
    assert shared is one and cfgs == [one]
    shared, cfgs = per_prompt_configs(tuple(_cfgs(4)), 4)
    assert [c.guidance_scale for c in cfgs] == [3.0, 4.0, 5.0, 6.0] and [c.seed for c in cfgs] == [0, 10, 20, 30] and shared is cfgs[0]
    # do_cfg may differ as long as "CFG on" does not: (do_cfg, scale 3) and (do_cfg, scale 4) are both on
    per_prompt_configs([SJDConfig(do_cfg=True, guidance_scale=3.0), SJDConfig(do_cfg=True, guidance_scale=4.0)], 2)
    per_prompt_configs([SJDConfig(do_cfg=False, guidance_scale=3.0), SJDConfig(do_cfg=True, guidance_scale=1.0)], 2)     # both off
    for bad_n in (3, 5):
        with pytest.raises(ValueError, match=f"4 configs for {bad_n} prompts"):
            per_prompt_configs(_cfgs(4), bad_n)
    with pytest.raises(ValueError, match="config of prompt 1 is dict"):
        per_prompt_configs([one, {}], 2)


@pytest.mark.parametrize("field,other", [("max_num_new_tokens", 8), ("prefix_token_sampler_scheme", "jacobi"), ("multi_token_init_scheme", "repeat_horizon"),
                                         ("do_sample", False), ("noise_device", "cpu"), ("max_length", 77), ("eos_token_ids", (3,)),
                                         ("jacobi_loop_interval_r", 9), ("img_vocab_n", 16)])
def test_fields_that_must_agree_are_named(field, other):
    from sjd_amd.engine_batch import per_prompt_configs
    cfgs = _cfgs(4)
    cfgs[2] = dataclasses.replace(cfgs[2], **{field: other})
    with pytest.raises(ValueError, match=rf"SJDConfig\.{field} must agree .* prompt 0 has .* prompt 2 has ") as e:
        per_prompt_configs(cfgs, 4)
    assert repr(other) in str(e.value)


def test_every_config_field_is_per_prompt_or_must_agree():
    """a field added to SJDConfig later is shared until someone decides otherwise"""
    from sjd_amd.engine import SJDConfig
    from sjd_amd import engine_batch as EB
    names = {f.name for f in dataclasses.fields(SJDConfig)}
    assert set(EB._PER_PROMPT_FIELDS) == {"guidance_scale", "seed", "do_cfg"} and set(EB._PER_PROMPT_FIELDS) <= names
    for need in ("max_num_new_tokens", "prefix_token_sampler_scheme", "multi_token_init_scheme", "do_sample", "noise_device"):
        assert need in names - set(EB._PER_PROMPT_FIELDS)


def test_cfg_on_must_agree():
    from sjd_amd.engine import SJDConfig
    from sjd_amd.engine_batch import per_prompt_configs
    with pytest.raises(ValueError, match=r"do_cfg and guidance_scale != 1.*prompt 0 and False for prompt 1"):
        per_prompt_configs([SJDConfig(guidance_scale=3.0), SJDConfig(guidance_scale=1.0)], 2)
    with pytest.raises(ValueError, match=r"do_cfg and guidance_scale != 1.*for prompt 2"):
        per_prompt_configs([SJDConfig(), SJDConfig(guidance_scale=2.0), SJDConfig(do_cfg=False)], 3)


def _bare_engine(**attrs):
    """the engine's host side without a device (decode_many validates its configs before it touches one)"""
    from sjd_amd.engine_batch import SJDBatchEngine
    eng = SJDBatchEngine.__new__(SJDBatchEngine)
    eng.P, eng.nb, eng.Lmax, eng.slot_launches, eng.head_partials, eng._guidance, eng._mixed_guidance = 2, 2, 16, True, True, 3.0, False
    for k, v in attrs.items():
        setattr(eng, k, v)
    return eng


def test_decode_many_validates_before_any_launch():
    eng = _bare_engine()
    with pytest.raises(ValueError, match=r"SJDConfig\.do_sample must agree"):
        eng.decode_many([[], []], [None, None], [None, None], [dataclasses.replace(c, do_sample=bool(j)) for j, c in enumerate(_cfgs(2))])
    with pytest.raises(ValueError, match="3 configs for 2 prompts"):
        eng.decode_many([[], []], [None, None], [None, None], _cfgs(3))


def test_mixed_scales_are_refused_on_dense_logits():
    """the cut line, known before anything runs: the K2 that reads dense logits bakes one scalar into its graphs"""
    eng = _bare_engine(head_partials=False)
    with pytest.raises(ValueError, match="different guidance scales.*dense logits"):
        eng.decode_many([[], []], [None, None], [None, None], _cfgs(2))
    assert eng._mixed_guidance


def test_mixed_scales_are_refused_on_per_slot_k2_over_a_narrow_head():
    """... and known at the first window forward: one K2 launch per slot (SJD_SLOT_LAUNCHES=0) over a head too narrow for K2a; _sample_body refuses
    before it launches anything"""
    import sjd_amd.ops as ops
    narrow = ops.HeadOut(ops.Partials(torch.zeros(1, 32, 8192), 1, 8192), 0, 16, torch.bfloat16)
    assert ops.head_slots_ok(narrow)
    eng = _bare_engine(_mixed_guidance=True, hook=None, slot_launches=False)
    with pytest.raises(ValueError, match="different guidance scales.*SJD_SLOT_LAUNCHES=0"):
        eng._sample_body(0, narrow, None)
    with pytest.raises(ValueError, match="different guidance scales"):
        eng._sample_body(0, torch.zeros(4, 16, 8192), None)                 # dense logits
    eng._mixed_guidance = False
    eng._refuse_mixed_guidance_per_slot()                                   # one scale: nothing to refuse
    assert eng._guidance_key() == 3.0                                      # ... and the graph keys of a single config
    eng._mixed_guidance = True
    assert eng._guidance_key() == "per-slot array"


def test_solver_per_prompt_values():
    from sjd_amd.llamagen_solver import per_prompt_values
    assert per_prompt_values("cfg_scale", 4.0, 5) is None and per_prompt_values("top_k", 1000, 1) is None
    assert per_prompt_values("top_p", None, 3) is None and per_prompt_values("cfg_scale", torch.tensor(4.0), 3) is None
    assert per_prompt_values("cfg_scale", [1.5, 3, 4], 3) == [1.5, 3, 4]
    assert per_prompt_values("cfg_scale", torch.tensor([1.5, 3.0, 7.5]), 3) == [1.5, 3.0, 7.5]
    import numpy as np
    assert per_prompt_values("top_k", np.array([100, 200]), 2) == [100, 200]
    with pytest.raises(ValueError, match="temperature has 2 values for 3 prompts"):
        per_prompt_values("temperature", (1.0, 0.9), 3)
    with pytest.raises(ValueError, match="top_k was given as a sequence of 1 values, but generate\\(\\) got one prompt"):
        per_prompt_values("top_k", [1000], 1)


class _NoModel:
    model_type, num_classes, _ops, do_cfg, guidance_scale, max_num_new_tokens = "c2i", 1000, object(), True, 4.0, 16


def test_solver_generate_refuses_bad_sequences():
    from sjd_amd.llamagen_solver import LlamaGenSolver
    solver = LlamaGenSolver(_NoModel(), 1000, 1.0)
    five, one = torch.tensor([1, 2, 3, 4, 5]), torch.tensor([7])
    for kw in (dict(cfg_scale=[4.0]), dict(cfg_scale=4.0, top_k=[1000]), dict(cfg_scale=4.0, temperature=torch.tensor([1.0])), dict(cfg_scale=4.0, top_p=(0.9,))):
        with pytest.raises(ValueError, match="got one prompt"):
            solver.generate(one, 64, None, **kw)
    with pytest.raises(ValueError, match="cfg_scale has 4 values for 5 prompts"):
        solver.generate(five, 64, None, cfg_scale=[1.5, 3, 4, 7.5])
    with pytest.raises(ValueError, match="top_p has 6 values for 5 prompts"):
        solver.generate(five, 64, None, cfg_scale=4.0, top_p=[0.9] * 6)
    with pytest.raises(ValueError, match="cfg_scale 1.0 of prompt 3 .* CFG-on or CFG-off as a whole"):
        solver.generate(five, 64, None, cfg_scale=[1.5, 3, 4, 1.0, 2])


def test_solver_processors_per_prompt():
    from sjd_amd.llamagen_solver import LlamaGenSolver
    from sjd_amd.scheduler.logit_processor_3dim import grammar_from_processors
    solver = LlamaGenSolver(_NoModel(), 1000, 0.95)
    g = grammar_from_processors(list(solver.create_logits_processor()), prompt_len=1, max_length=64, vocab_size=16384)
    assert (g.top_k, g.top_p, g.temperature) == (1000, 0.95, 1.0)
    g = grammar_from_processors(list(solver.create_logits_processor(top_k=300, top_p=0.8, temperature=0.7)), prompt_len=1, max_length=64, vocab_size=16384)
    assert (g.top_k, g.top_p, g.temperature) == (300, 0.8, 0.7)
    r = g.window_rules(2)[0]
    assert r.top_k == 300 and abs(r.temperature - 0.7) < 1e-7 and abs(r.top_p_thr - 0.2) < 1e-6


def test_new_export_is_declared():
    import sjd_amd._lib as L
    if not os.path.exists(L.SO_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = L.load()
    name = "sjd_logits_to_probs_sample_part_slots_g"
    hdr = open(os.path.join(ROOT, "include", "sjd_hip.h")).read()
    assert re.search(rf"^int {name}\(const sjd_head_partials \*head, const float \*guidance, int max_rows, int V,", hdr, re.M)
    assert name in L.EXPORTS and len(L.EXPORTS) == len(set(L.EXPORTS)) <= 45
    vp = ctypes.c_void_p
    assert getattr(lib, name).argtypes == [ctypes.POINTER(L.HeadPartials), vp, ctypes.c_int32, ctypes.c_int32, vp, vp, vp, vp, ctypes.POINTER(L.Slots), vp]
    assert re.search(r"#define SJD_VERSION 104\b", hdr)
    # argument checks run before any launch: no array, a misaligned array, then the checks of the scalar entry point (no head)
    assert getattr(lib, name)(None, None, 16, 100, None, None, None, None, None, None) == -1
    hp, sl = L.HeadPartials(), L.Slots()
    assert getattr(lib, name)(ctypes.byref(hp), vp(6), 16, 100, None, None, None, None, ctypes.byref(sl), None) == -1
    assert getattr(lib, name)(ctypes.byref(hp), vp(8), 16, 100, None, None, None, None, ctypes.byref(sl), None) == -1
    k2a = "sjd_head_combine_g"                                                # the feature's second export
    assert k2a in L.EXPORTS and re.search(rf"^int {k2a}\(const sjd_head_partials \*head, const float \*guidance", hdr, re.M)
    assert getattr(lib, k2a).argtypes == [ctypes.POINTER(L.HeadPartials), vp, ctypes.c_int32, ctypes.c_int32, vp, vp, vp]
    assert getattr(lib, k2a)(ctypes.byref(hp), None, 16, 100, None, None, None) == -1
    assert getattr(lib, k2a)(ctypes.byref(hp), vp(8), 16, 100, None, None, None) == -1


def test_example_takes_a_scale_per_class_id():
    import importlib.util
    spec = importlib.util.spec_from_file_location("llamagen_c2i_example_pp", os.path.join(ROOT, "examples", "llamagen_c2i.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    assert ex.parse_args([]).cfg_scale == 4.0 and ex.parse_args(["--cfg-scale", "3"]).cfg_scale == 3.0
    a = ex.parse_args(["--fused", "--class-id", "207", "1", "980", "417", "--cfg-scale", "1.5", "3", "4", "7.5"])
    assert a.class_id == [207, 1, 980, 417] and a.cfg_scale == [1.5, 3.0, 4.0, 7.5]
    assert ex.parse_args(["--fused", "--class-id", "207", "1", "--cfg-scale", "3"]).cfg_scale == 3.0
    for bad in (["--fused", "--class-id", "207", "1", "980", "--cfg-scale", "1.5", "3"], ["--cfg-scale", "1.5", "3"]):
        with pytest.raises(SystemExit):
            ex.parse_args(bad)
