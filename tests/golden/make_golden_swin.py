#!/usr/bin/env python3
"""Generate the swin-norm Chameleon fixtures by IMPORTING THE REFERENCE in this container (CPU), as make_golden.py does.

Run:  python tests/golden/make_golden_swin.py          (writes the two files below)

The reference's ChameleonModel builds ChameleonSwinDecoderLayer when config.swin_norm is true (the RMSNorm after each sublayer) and stores
the QK-norm gain / bias as [model_parallel_size, head_dim] -- the form of the 30B-class checkpoints.  Tiny configurations of that form,
with grouped-query attention and model_parallel_size=2, per-key synthetic weights (sjd_amd.synthetic.fill_state_dict):

  fwd_chameleon_swin.npz   the reference's fp32 logits of whole token sequences (use_cache=False); the tests replay them as a prefix
                           forward plus a window forward on the cache
  loop_lumina_swin.npz     the reference's whole SJD loop on the same form: the run table of make_golden.gen_loop_lumina -- one sampled run,
                           one greedy run (GenerationConfig(do_sample=False)), one plain-Jacobi run

Only inputs (seeds, small integer arrays) and the reference's outputs are written; nothing at test time imports this script.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (installs the reference shims; its sys.path rules apply)

from transformers import GenerationConfig  # noqa: E402
from transformers.generation.logits_process import LogitsProcessorList  # noqa: E402
from transformers.generation.stopping_criteria import StoppingCriteriaList, EosTokenCriteria, MaxLengthCriteria  # noqa: E402

VQ = dict(embed_dim=32, num_embeddings=64, double_latent=False, latent_channels=32, resolution=32, in_channels=3, base_channels=32,
          channel_multiplier=[1, 1], num_res_blocks=1, attn_resolutions=None, dropout=0.0, attn_type="vanilla")


def _model(cfg_kw, ets, seed=23):
    from model.chameleon import ChameleonForConditionalGeneration, ChameleonConfig
    cfg = ChameleonConfig(**cfg_kw, attn_implementation="sdpa")
    cfg.rope_scaling = None
    model = ChameleonForConditionalGeneration(cfg).eval()
    assert type(model.model.layers[0]).__name__ == "ChameleonSwinDecoderLayer"
    assert tuple(model.model.layers[0].self_attn.q_norm.weight.shape) == (cfg_kw["model_parallel_size"], cfg_kw["hidden_size"] // cfg_kw["num_attention_heads"])
    MG.synthetic.fill_state_dict(model, seed=seed, skip_prefixes=("model.vqmodel.",), embed_token_scale=ets)
    return model


def gen_fwd():
    """fp32 logits of two token sequences of 12 (a 512-word vocabulary keeps the file small)"""
    cfg_kw = dict(vocab_size=512, hidden_size=64, intermediate_size=128, num_hidden_layers=3, num_attention_heads=4, num_key_value_heads=2,
                  model_parallel_size=2, swin_norm=True, max_position_embeddings=512, rms_norm_eps=1e-5, rope_theta=10000.0,
                  mask_image_logits=False, vocabulary_map={"<image>": 500}, vq_config=VQ)
    model = _model(cfg_kw, 1.0, seed=31)
    g = torch.Generator().manual_seed(5)
    tokens = torch.randint(4, 500, (2, 12), generator=g)
    logits = model(input_ids=tokens, use_cache=False).logits.float()
    meta = dict(config={k: v for k, v in cfg_kw.items() if k != "vq_config"}, weight_seed=31, embed_token_scale=1.0, prefix=7)
    np.savez_compressed(os.path.join(HERE, "fwd_chameleon_swin.npz"), tokens=tokens.numpy(), logits=logits.numpy(), meta=np.array(json.dumps(meta)))
    print("fwd_chameleon_swin", tuple(logits.shape), "argmax", logits[0, -1].argmax().item())


def gen_loop():
    out, meta = {}, []
    # (name, scheme, do_sample, seed, hg, wg, window, l, r, P, embed_token_scale) -- the rows of make_golden.gen_loop_lumina
    runs = [("spec_s3", "speculative_jacobi", True, 3, 4, 4, 16, 3, 8 * 9 - 10, 12, 0.25),
            ("greedy_s6_w8", "speculative_jacobi", False, 6, 3, 5, 8, 3, 6 * 11 - 6, 20, 0.5),
            ("jacobi_s3", "jacobi", True, 3, 4, 4, 16, 3, 8 * 9 - 10, 12, 0.25)]
    for name, scheme, do_sample, seed, hg, wg, window, l, r, P, ets in runs:
        V = 9216
        cfg_kw = dict(vocab_size=V, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                      model_parallel_size=2, swin_norm=True, max_position_embeddings=512, rms_norm_eps=1e-5, rope_theta=10000.0,
                      mask_image_logits=False, vocabulary_map={"<image>": 8711}, vq_config=VQ)
        model = _model(cfg_kw, ets)
        jac = dict(jacobi_loop_interval_l=l, jacobi_loop_interval_r=r, max_num_new_tokens=window, guidance_scale=3.0,
                   seed=seed, multi_token_init_scheme="random", do_cfg=True, image_top_k=2000, text_top_k=10,
                   prefix_token_sampler_scheme=scheme, use_chameleon_tokenizer=False)
        model.__class__ = type("M", (MG.CompatMixin, MG.JL.renew_sampler(model.__class__)), {})
        model._init_new_params(**jac)
        model.img_vocab = torch.arange(4, 8196)
        model.model.__class__ = MG.JL.renew_backbone(model.model.__class__)
        procs = LogitsProcessorList([
            MG.LP.MultiTokensVLLogitsProcessor(image_start_token_id=8197, image_end_token_id=8196, image_next_line_token_id=8803, patch_size=32,
                                               voc_size=V),
            MG.LP.MultiTokensInterleavedTopKLogitsWarper(image_top_k=2000, text_top_k=10, image_start_token_id=8197, image_end_token_id=8196)])
        prompt = torch.cat([MG.synthetic.synthetic_prompt(P - 3, seed, lo=8900, hi=9200), torch.tensor([[8197, 8804 + hg, 8804 + wg]])], dim=1)
        n_img = (2 * wg + 1) * 2 * hg
        max_len = P + n_img + 1 + 4
        stopping = StoppingCriteriaList([EosTokenCriteria([8196]), MaxLengthCriteria(max_len)])
        gc = GenerationConfig(max_length=max_len, do_sample=do_sample, temperature=1.0, top_k=None)
        gc._pad_token_tensor = torch.tensor(0)
        tr = MG.Tracer()
        tr.install()
        try:
            seq = model._sample(input_ids=prompt, logits_processor=procs, stopping_criteria=stopping, generation_config=gc, synced_gpus=False,
                                streamer=None, attention_mask=torch.ones_like(prompt), past_key_values=MG.LegacyCache(), use_cache=True)
        finally:
            tr.remove()
        out[f"{name}.prompt"] = prompt.numpy()
        out[f"{name}.sequence"] = seq.numpy()
        tr.pack(name, out)
        meta.append(dict(name=name, config={k: v for k, v in cfg_kw.items() if k != "vq_config"}, weight_seed=23, embed_token_scale=ets,
                         jacobi=jac, do_sample=do_sample, P=P, hg=hg, wg=wg, max_len=max_len, nfe=len(tr.matched)))
        print("loop_lumina_swin", name, "generated", seq.shape[1] - P, "NFE", len(tr.matched))
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(HERE, "loop_lumina_swin.npz"), **out)


if __name__ == "__main__":
    which = sys.argv[1:] or ["fwd", "loop"]
    if "fwd" in which:
        gen_fwd()
    if "loop" in which:
        gen_loop()
