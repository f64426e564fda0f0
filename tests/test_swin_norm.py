"""Swin-norm Chameleon backbones (the 30B-class form: ChameleonSwinDecoderLayer, QK-norm gains in model_parallel_size shards) on the CPU:
the eager forward against the reference's logits, the whole SJD loop of the CPU oracle against the reference's loop, checkpoint loading
and argument validation.  Fixtures: tests/golden/make_golden_swin.py."""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import sjd_amd.backbones as BB
import sjd_amd.synthetic as synthetic
from oracle.attention_ref import OracleWindowAttention


def swin_args(config):
    keys = {k: v for k, v in config.items() if k in BB.ChameleonArgs.__dataclass_fields__}
    return BB.ChameleonArgs(qk_norm=True, **keys)


def make_swin(config, weight_seed, embed_token_scale, attn, dtype=torch.float32, device="cpu"):
    model = BB.ChameleonBackbone(swin_args(config), attn=attn).eval()
    synthetic.fill_state_dict(model, seed=weight_seed, embed_token_scale=embed_token_scale)
    return model.to(device=device, dtype=dtype)


def _load(golden_dir, name):
    d = np.load(os.path.join(golden_dir, name))
    return d, json.loads(str(d["meta"]))


def test_swin_backbone_holds_sharded_qk_norms(golden_dir):
    d, m = _load(golden_dir, "fwd_chameleon_swin.npz")
    model = make_swin(m["config"], m["weight_seed"], m["embed_token_scale"], None)
    assert model.args.swin_norm and model.args.model_parallel_size == 2
    sd = model.state_dict()
    assert tuple(sd["model.layers.0.self_attn.q_norm.weight"].shape) == (2, 16)
    assert tuple(sd["model.layers.0.self_attn.k_norm.bias"].shape) == (2, 16)
    # row r of the gain serves heads [r * H / mp, (r + 1) * H / mp): heads 0, 1 -> row 0, heads 2, 3 -> row 1 (q); one k head per row
    qn = model.model.layers[0].self_attn.q_norm
    x = torch.randn(1, 1, 4, 16)
    y = qn(x)
    base = torch.nn.functional.layer_norm(x, (16,), eps=1e-5)
    for h, r in ((0, 0), (1, 0), (2, 1), (3, 1)):
        assert torch.allclose(y[0, 0, h], base[0, 0, h] * qn.weight[r] + qn.bias[r])


@torch.no_grad()
def test_swin_eager_forward_matches_reference_logits(golden_dir):
    """the eager fp32 forward in the swin order reproduces the reference's logits within 1e-5: a 7-token prefix, then a 5-token window on the
    cache, both batch rows"""
    d, m = _load(golden_dir, "fwd_chameleon_swin.npz")
    model = make_swin(m["config"], m["weight_seed"], m["embed_token_scale"], OracleWindowAttention())
    tokens, ref = torch.from_numpy(d["tokens"]), torch.from_numpy(d["logits"])
    B, L = tokens.shape
    P = m["prefix"]
    model.setup_cache(batch=B, s_max=32)
    ks = torch.zeros(B, dtype=torch.int32)
    pos = torch.arange(L)[None].repeat(B, 1)
    l1 = model.forward_window(tokens[:, :P], pos[:, :P], 0, ks)
    l2 = model.forward_window(tokens[:, P:], pos[:, P:], P, ks)
    got = torch.cat([l1, l2], dim=1)
    assert got.shape == ref.shape
    err = (got - ref).abs().max().item()
    assert err <= 1e-5, err
    # the pre-norm arithmetic on the same weights is a different model: the fixture would catch a silent fall-back
    pre = make_swin({**m["config"], "swin_norm": False}, m["weight_seed"], m["embed_token_scale"], OracleWindowAttention())
    pre.setup_cache(batch=B, s_max=32)
    assert (pre.forward_window(tokens, pos, 0, ks) - ref).abs().max().item() > 1e-2


def test_swin_oracle_loop_matches_reference_loop(golden_dir):
    """the CPU oracle loop over the eager swin backbone reproduces the reference's SJD loops token for token (sampled, greedy, plain Jacobi)"""
    from oracle import loop as OL
    from oracle import sjd_oracle as O
    from tests.helpers import lumina_forward_fn
    d, meta = _load(golden_dir, "loop_lumina_swin.npz")
    assert [m["jacobi"]["prefix_token_sampler_scheme"] for m in meta] == ["speculative_jacobi", "speculative_jacobi", "jacobi"]
    assert [m["do_sample"] for m in meta] == [True, False, True]
    for m in meta:
        name, jac = m["name"], m["jacobi"]
        model = make_swin(m["config"], m["weight_seed"], m["embed_token_scale"], OracleWindowAttention())
        prompt = d[f"{name}.prompt"][0].tolist()
        fwd = lumina_forward_fn(model, len(prompt), m["max_len"] + 32)
        cfg = OL.LoopConfig(jacobi_loop_interval_l=jac["jacobi_loop_interval_l"], jacobi_loop_interval_r=jac["jacobi_loop_interval_r"],
                            max_num_new_tokens=jac["max_num_new_tokens"], guidance_scale=jac["guidance_scale"], seed=jac["seed"],
                            do_cfg=jac["do_cfg"], prefix_token_sampler_scheme=jac["prefix_token_sampler_scheme"], max_length=m["max_len"],
                            eos_token_ids=(8196,), do_sample=m["do_sample"])
        seq, tr = OL.run(prompt, fwd, lambda c, n: O.lumina_rules(c, n, 2000, 10), cfg, m["config"]["vocab_size"], no_cfg_fn=O.lumina_force_no_cfg)
        assert seq == d[f"{name}.sequence"][0].tolist(), name
        assert tr.matched == d[f"{name}.matched"].tolist(), name


@pytest.mark.parametrize("H,Hkv,mp", [(4, 2, 3), (4, 2, 4), (6, 4, 3), (4, 4, 0)])
def test_invalid_model_parallel_size_raises(H, Hkv, mp):
    args = BB.ChameleonArgs(vocab_size=64, hidden_size=16 * H, intermediate_size=64, num_hidden_layers=1, num_attention_heads=H,
                            num_key_value_heads=Hkv, model_parallel_size=mp, swin_norm=True)
    with pytest.raises(ValueError, match="model_parallel_size"):
        BB.ChameleonBackbone(args)


def test_load_builds_swin_backbone_from_checkpoint_dir(tmp_path, golden_dir):
    """FlexARInferenceSolver._load reads swin_norm and model_parallel_size from config.json: the [mp, D] norm tensors of a swin checkpoint
    load, and the loaded backbone computes the swin forward"""
    from safetensors.torch import save_file
    from sjd_amd.inference_solver import FlexARInferenceSolver
    d, m = _load(golden_dir, "fwd_chameleon_swin.npz")
    src = make_swin(m["config"], m["weight_seed"], m["embed_token_scale"], None)
    cfg = dict(m["config"], model_type="chameleon")
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    save_file({k: v.contiguous() for k, v in src.state_dict().items()}, str(tmp_path / "model.safetensors"))
    model = FlexARInferenceSolver._load(str(tmp_path))
    assert model.args.swin_norm is True and model.args.model_parallel_size == 2
    assert tuple(model.model.layers[1].self_attn.k_norm.weight.shape) == (2, 16)
    for k, v in src.state_dict().items():
        assert torch.equal(model.state_dict()[k], v), k
    model.attn = OracleWindowAttention()
    model.setup_cache(batch=2, s_max=32)
    tokens = torch.from_numpy(d["tokens"])
    got = model.forward_window(tokens, torch.arange(tokens.shape[1])[None].repeat(2, 1), 0, torch.zeros(2, dtype=torch.int32))
    assert (got - torch.from_numpy(d["logits"])).abs().max().item() <= 1e-5
    # a pre-norm checkpoint directory (no swin keys) still loads as before
    (tmp_path / "config.json").write_text(json.dumps({k: v for k, v in cfg.items() if k not in ("swin_norm", "model_parallel_size")}))
    with pytest.raises(RuntimeError, match="size mismatch"):
        FlexARInferenceSolver._load(str(tmp_path))          # [2, D] norms into a model_parallel_size=1 backbone


def test_chameleon_30b_preset_shapes():
    a = BB.CHAMELEON_30B
    assert a.swin_norm and a.qk_norm and a.num_attention_heads % a.model_parallel_size == 0 and a.num_key_value_heads % a.model_parallel_size == 0
    with torch.device("meta"):
        model = BB.ChameleonBackbone(dataclasses.replace(a, num_hidden_layers=1))
    D = a.hidden_size // a.num_attention_heads
    at = model.model.layers[0].self_attn
    assert tuple(at.q_norm.weight.shape) == (a.model_parallel_size, D) and tuple(at.k_norm.weight.shape) == (a.model_parallel_size, D)
    assert tuple(at.k_proj.weight.shape) == (a.num_key_value_heads * D, a.hidden_size)
    per_layer = sum(p.numel() for p in model.model.layers[0].parameters())
    total = per_layer * a.num_hidden_layers + 2 * a.vocab_size * a.hidden_size + a.hidden_size
    assert 60e9 < 2 * total < 75e9          # bf16 bytes of the whole model: the "about 67 GB" the 288 GB card holds


def test_swin_backbone_refuses_batch_engine_and_fp8_cache():
    from sjd_amd import ops
    from sjd_amd.engine_batch import SJDBatchEngine
    model = make_swin(dict(vocab_size=64, hidden_size=64, intermediate_size=64, num_hidden_layers=1, num_attention_heads=4,
                           num_key_value_heads=2, model_parallel_size=2, swin_norm=True), 1, 1.0, None)
    with pytest.raises(ValueError, match="swin-norm"):
        SJDBatchEngine(model, 64, "cpu", n_prompts=2)
    with pytest.raises(ValueError, match="fp8"):
        model.setup_cache(batch=2, s_max=32, dtype=ops.FP8)
