#!/usr/bin/env python3
"""End-to-end class-conditional LlamaGen generation with Speculative Jacobi Decoding on one MI355X: the flow of the reference's
test_llamagen.py (model registry -> renew_llamagen / renew_sampler -> LlamaGenSolver.generate -> VQ decode -> image file), with the
reference's import lines.  The VQ decoder goes into generate(vq_model=): it returns the pixels next to the ids, and with several labels
every image is decoded on a side stream as soon as its label's tokens are complete, under the window forwards of the others.
Checkpoints: pass --gpt-ckpt / --vq-ckpt (the reference's files load unchanged: same state-dict keys);
without them both networks get synthetic weights, which exercises every step but of course draws noise.

    python examples/llamagen_c2i.py --class-id 207 --out sample.png
    python examples/llamagen_c2i.py --fused --class-id 207 1 980 417 --out grid.png      # four images per forward: grid_207.png, grid_1.png, ...
    python examples/llamagen_c2i.py --fused --gpt-model GPT-3B --image-size 384 --class-id 207 1 980 417      # GPT-3B too (heads of 100 stored 128 wide)
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from llamagen.llamagen import GPT_models  # noqa: E402                                  (test_llamagen.py:19)
from llamagen.llamagen_solver import LlamaGenSolver, renew_llamagen  # noqa: E402       (test_llamagen.py:20)
from llamagen.tokenizer.tokenizer_image.vq_model import VQ_models  # noqa: E402         (test_llamagen.py:17)
from scheduler.jacobi_iteration_lumina_mgpt import renew_sampler  # noqa: E402          (test_llamagen.py:21)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpt-model", default="GPT-B", choices=list(GPT_models))
    ap.add_argument("--gpt-ckpt", default=None)
    ap.add_argument("--vq-model", default="VQ-16", choices=list(VQ_models))
    ap.add_argument("--vq-ckpt", default=None)
    ap.add_argument("--image-size", type=int, default=256)
    ap.add_argument("--class-id", type=int, nargs="+", default=[207],
                    help="one ImageNet class, or several: they share the window forwards (needs --fused) and one PNG is written per label")
    ap.add_argument("--prompts-per-forward", type=int, default=None, help="several labels: how many share a forward (default: what 256 rows hold)")
    ap.add_argument("--cfg-scale", type=float, nargs="+", default=[4.0],
                    help="classifier-free guidance scale: one value, or one per --class-id (the labels still share their window forwards)")
    ap.add_argument("--top-k", type=int, default=1000)
    ap.add_argument("--top-p", type=float, default=1.0)
    ap.add_argument("--window", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--fused", action="store_true", help="draft windows on the hand-written HIP path (LlamaGenBackbone.enable_fused)")
    ap.add_argument("--weights", default=None, choices=["e4m3", "mxfp4"],
                    help="with --fused: stream the layer projections from QUANTISED weights (LOSSY, opt-in; image quality on a real checkpoint is not measured)")
    ap.add_argument("--compress", action="store_true",
                    help="with --fused: stream the layer projections and the output head from the LOSSLESS 12-bit copy (about 0.78 of the bytes, the same tokens; "
                         "at most 128 window rows per forward)")
    ap.add_argument("--lenience", type=float, default=1.0,
                    help="accept a draft with min(1, LENIENCE * p / q) in the verify step (LOSSY, opt-in; 1 is the exact rule; >= 1 and exactly a bf16 value, "
                         "e.g. 1.25, 1.5, 2, 4; more tokens per step, image quality on a real checkpoint is not measured)")
    ap.add_argument("--scheme", default="speculative_jacobi", choices=["speculative_jacobi", "jacobi", "coupled_jacobi"],
                    help="the verify step: speculative_jacobi (default); jacobi (token equality, per-iteration noise); coupled_jacobi (token equality, "
                         "sampling noise keyed by the token's position: lossless, and the image of a --seed does not depend on --window or on the "
                         "labels sharing a forward)")
    ap.add_argument("--out", default="sample.png")
    a = ap.parse_args(argv)
    try:
        from sjd_amd.engine import lenience_field
        lenience_field(a.lenience, a.scheme)
    except ValueError as e:
        ap.error(f"--lenience: {e}")
    if a.weights and not a.fused:
        ap.error("--weights packs the weights of the fused HIP path: add --fused")
    if a.compress and not a.fused:
        ap.error("--compress packs the weights of the fused HIP path: add --fused")
    if a.compress and a.weights:
        ap.error("--compress (lossless 12-bit) and --weights (a quantised copy) are two streams: one per packed copy")
    if a.compress and (a.prompts_per_forward or len(a.class_id)) * 2 * a.window > 128:
        ap.error(f"--compress serves at most 128 window rows per forward: --prompts-per-forward {max(1, 128 // (2 * a.window))} or fewer at --window {a.window}")
    if len(a.class_id) > 1 and not a.fused:
        ap.error("several --class-id labels are decoded together on the fused HIP path: add --fused")
    if len(a.cfg_scale) not in (1, len(a.class_id)):
        ap.error(f"--cfg-scale takes one value or one per --class-id ({len(a.class_id)}), got {len(a.cfg_scale)}")
    if len(a.cfg_scale) == 1 or len(a.class_id) == 1:
        a.cfg_scale = a.cfg_scale[0]                                                     # a number: every prompt's scale, as ever
    return a


def out_paths(out, class_ids):
    """one label: `out` itself; several: <stem>_<label><ext> per label (a repeated label gets its index as well)"""
    if len(class_ids) == 1:
        return [out]
    stem, ext = os.path.splitext(out)
    return [f"{stem}_{c}{ext}" if class_ids.count(c) == 1 else f"{stem}_{c}_{i}{ext}" for i, c in enumerate(class_ids)]


def main():
    a = parse_args()
    dev = torch.device("cuda:0")
    import sjd_amd.ops as ops
    import sjd_amd.synthetic as synthetic
    latent = a.image_size // (16 if a.vq_model == "VQ-16" else 8)

    vq = VQ_models[a.vq_model](codebook_size=16384, codebook_embed_dim=8).to(dev).eval()
    if a.vq_ckpt:
        vq.load_state_dict(torch.load(a.vq_ckpt, map_location="cpu")["model"])
    else:
        synthetic.fill_state_dict_conv(vq, seed=1)

    gpt = GPT_models[a.gpt_model](block_size=latent ** 2, cls_token_num=1, model_type="c2i", num_classes=1000).to(dev, torch.bfloat16).eval()
    gpt.attn = ops.HipWindowAttention()
    if a.gpt_ckpt:
        ck = torch.load(a.gpt_ckpt, map_location="cpu")
        gpt.load_state_dict(ck.get("model", ck), strict=False)
    else:
        synthetic.fill_state_dict_device(gpt, seed=0, embed_token_scale=0.5)
    if a.fused:
        rows = (a.prompts_per_forward or len(a.class_id)) * 2 * a.window          # prompts x CFG pair x window rows per forward
        # (GPT-3B's 32 heads are 100 wide: the kernels store them 128 wide with zero pad columns, which the backbone does on request only)
        # (... and several labels per forward on the padded model need its own swept launch shapes: padded_batch, no effect on the other models)
        gpt.enable_fused(ops, gemm="sjd", max_rows=64 if rows <= 64 else (128 if rows <= 128 else 256), pad_head_dim=gpt.head_dim == 100,
                         padded_batch=rows > 64, weights=a.weights, compress=a.compress)
        if a.compress:
            st = gpt.compress_stats
            print(f"--compress: lossless 12-bit copy, {st['bytes_packed'] / st['bytes_raw']:.3f} of the 16-bit bytes ({st['raw_units']} of {st.get('units', 0)} units verbatim)")
        if a.weights:
            print(f"--weights {a.weights}: LOSSY, rel. RMS error of the packed projections {gpt.compress_stats['rel_rms_error']:.4f}")
    one_scale = a.cfg_scale if isinstance(a.cfg_scale, float) else a.cfg_scale[0]        # (a scale per label: this one only says "CFG on")
    jac = dict(jacobi_loop_interval_l=1, jacobi_loop_interval_r=latent ** 2 - a.window - 2, max_num_new_tokens=a.window,
               guidance_scale=one_scale, seed=a.seed, multi_token_init_scheme="random", do_cfg=True, image_top_k=a.top_k,
               text_top_k=10, prefix_token_sampler_scheme=a.scheme)
    gpt.__class__ = renew_llamagen(gpt.__class__)
    gpt._init_new_params(**jac)
    gpt.__class__ = renew_sampler(gpt.__class__)
    gpt._init_new_params(**jac)

    solver = LlamaGenSolver(model=gpt, image_top_k=a.top_k, image_top_p=a.top_p, prompts_per_forward=a.prompts_per_forward, lenience=a.lenience)
    if a.lenience != 1.0:
        print(f"--lenience {a.lenience}: LOSSY verify step, drafts accepted with min(1, {a.lenience} * p / q)")
    torch.manual_seed(a.seed)
    t0 = time.time()
    index_sample, images = solver.generate(torch.tensor(a.class_id, device=dev), latent ** 2, None, cfg_scale=a.cfg_scale, temperature=1.0,
                                           top_k=a.top_k, top_p=a.top_p, sample_logits=True, vq_model=vq, qzshape=(8, latent, latent))
    torch.cuda.synchronize()
    dt = time.time() - t0
    stats = gpt.last_sjd_stats if isinstance(gpt.last_sjd_stats, list) else [gpt.last_sjd_stats]
    n_tok = index_sample.numel()
    for c, st in zip(a.class_id, stats):
        print(f"class {c}: {index_sample.shape[1]} image tokens in {st.nfe} forward passes ({index_sample.shape[1] / max(st.nfe, 1):.2f} tokens/step)")
    print(f"{n_tok} image tokens and {len(images)} decoded images in {dt:.2f} s ({n_tok / dt:.0f} tokens/s)")

    from PIL import Image
    for img, path in zip(images, out_paths(a.out, a.class_id)):                          # uint8 [H, W, 3]   (test_llamagen.py:182-183)
        Image.fromarray(img.cpu().numpy()).save(path)
        print(f"wrote {path} ({img.shape[1]}x{img.shape[0]})")


if __name__ == "__main__":
    main()
