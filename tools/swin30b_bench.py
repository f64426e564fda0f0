#!/usr/bin/env python3
"""The 30B-class swin-norm Chameleon (backbones.CHAMELEON_30B) on one MI355X.

  --sweep   G1 launch shapes of its four projections at a 32-row window (window 16, CFG), uncompressed and 12-bit stream: us per launch
            from a hipGraph of back-to-back launches over enough weight copies that each streams from HBM.  One JSON line per shape;
            the fastest per projection is what G1_CFG_30B / G1_CFG_30B_Z hold.
  --step    ms per SJD step of the whole preset (synthetic weights drawn on the device, window 16, CFG, bf16) on the 12-bit stream and on
            the uncompressed packing (each packed once, before its timed decode), plus the projections' algorithmic bytes per step.
"""
import argparse
import dataclasses
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import sjd_amd.backbones as BB  # noqa: E402
import sjd_amd.ops as ops  # noqa: E402


def _graph_us(fn, n):
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        fn(0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(n):
            fn(i)
    g.replay()
    torch.cuda.synchronize()
    res = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        res.append(e0.elapsed_time(e1) * 1e3 / n)
    return min(res)


def sweep(args):
    a = BB.CHAMELEON_30B
    D = a.hidden_size // a.num_attention_heads
    shapes = dict(qkv=((a.num_attention_heads + 2 * a.num_key_value_heads) * D, a.hidden_size), o=(a.hidden_size, a.num_attention_heads * D),
                  gate_up=(2 * a.intermediate_size, a.hidden_size), down=(a.hidden_size, a.intermediate_size))
    dev = torch.device("cuda:0")
    M = args.rows
    g = torch.Generator(device=dev).manual_seed(1)
    best = {}
    for name, (N, K) in shapes.items():
        if args.only and name not in args.only.split(","):
            continue
        copies = max(2, -(-768 * 2**20 // (N * K * 2)))        # > 0.75 GB in flight: past the 256 MB Infinity Cache
        ws = [(torch.randn(N, K, generator=g, device=dev) / K ** 0.5).to(torch.bfloat16) for _ in range(copies)]
        x = torch.randn(M, K, generator=g, device=dev).to(torch.bfloat16)
        for kc in (512, 768, 1024, 1280, 1536, 1792, 2048, 2560):
            if kc > K or (M <= 32 and kc > 2560):
                continue
            for sm in (True, False):
                for z in (False, True):
                    packed = [ops.pack_weight_z(w, kc, sm) if z else ops.pack_weight(w, kc, sm) for w in ws]
                    if any(p is None for p in packed):
                        continue
                    for waves in (4, 6, 8):
                        try:
                            us = _graph_us(lambda i: ops.skinny_gemm(x, packed[i % copies], N, K, kc, waves, sm), 4 * copies)
                        except Exception as e:          # a launch shape the kernel declines
                            print(json.dumps(dict(proj=name, kc=kc, waves=waves, step_major=sm, z=z, error=str(e)[:80])), flush=True)
                            continue
                        nbytes = packed[0].nbytes() if z else N * K * 2
                        rec = dict(proj=name, N=N, K=K, rows=M, kc=kc, waves=waves, step_major=sm, z=z, us=round(us, 2),
                                   tbps_alg=round(N * K * 2 / us / 1e6, 3), tbps_packed=round(nbytes / us / 1e6, 3))
                        print(json.dumps(rec), flush=True)
                        key = (name, z)
                        if key not in best or us < best[key]["us"]:
                            best[key] = rec
                    del packed
        del ws
        torch.cuda.empty_cache()
    for (name, z), r in sorted(best.items()):
        print(json.dumps(dict(best=name, z=z, cfg=[r["kc"], r["waves"], r["step_major"]], us=r["us"], tbps_alg=r["tbps_alg"])), flush=True)


def step(args):
    from sjd_amd.engine import SJDEngine, SJDConfig
    from sjd_amd.frontends import lumina_window_spec, lumina_prompt
    from sjd_amd.grammar import LuminaGrammar
    import sjd_amd.synthetic as synthetic
    dev = torch.device("cuda:0")
    margs = dataclasses.replace(BB.CHAMELEON_30B, num_hidden_layers=args.layers)
    t0 = time.time()
    with torch.device(dev):
        model = BB.ChameleonBackbone(margs, attn=ops.HipWindowAttention()).to(torch.bfloat16).eval()
    synthetic.fill_state_dict_device(model, seed=0, embed_token_scale=0.7)
    torch.cuda.synchronize()
    out = dict(model="chameleon30b", layers=args.layers, window=16, cfg=True, dtype="bf16", weights_gb=round(sum(p.numel() for p in model.parameters()) * 2 / 1e9, 2),
               fill_s=round(time.time() - t0, 1), runs=[])
    window, grid, P = 16, 48, args.prompt
    prompt = lumina_prompt(P, grid, grid, seed=3)
    spec = lumina_window_spec(prompt, dev)
    for compress in (True, False):
        t0 = time.time()
        if "G1_CFG" in model.__dict__:
            del model.G1_CFG
        model.enable_fused(ops, gemm="sjd", compress=compress)
        torch.cuda.synchronize()
        pack_s = time.time() - t0
        proj_bytes = sum((p.nbytes() if isinstance(p, ops.PackedZ) else p.numel() * p.element_size()) for lay in model._packed for p in lay.values())
        proj_alg = sum(p.numel() * p.element_size() for lay in model.model.layers
                       for p in (lay.self_attn.q_proj.weight, lay.self_attn.k_proj.weight, lay.self_attn.v_proj.weight, lay.self_attn.o_proj.weight,
                                 lay.mlp.gate_proj.weight, lay.mlp.up_proj.weight, lay.mlp.down_proj.weight))
        model.setup_cache(batch=2, s_max=((P + (args.steps + args.warmup + 4) * window + 64 + 31) // 32) * 32)
        eng = SJDEngine(model, margs.vocab_size, dev, max_window=window, use_graph=True)
        cfg = SJDConfig(jacobi_loop_interval_l=0, jacobi_loop_interval_r=grid * grid + grid - 13, max_num_new_tokens=window, guidance_scale=3.0,
                        seed=3, max_length=P + grid * (grid + 1) + 1, eos_token_ids=(8196,))
        seq, st = eng.decode(prompt, spec, LuminaGrammar(2000, 10), cfg, warmup_iters=args.warmup, timed_iters=args.steps,
                             on_timed_start=torch.cuda.synchronize, on_timed_end=torch.cuda.synchronize)
        ms = 1e3 * st.seconds / max(1, st.timed_nfe)
        run = dict(packing="12-bit" if compress else "uncompressed", pack_s=round(pack_s, 1), ms_per_step=round(ms, 3), timed_steps=st.timed_nfe,
                   tokens_per_step=round(st.tokens / max(1, st.timed_nfe), 2), proj_gb_packed=round(proj_bytes / 1e9, 2),
                   proj_gb_alg=round(proj_alg / 1e9, 2), compress_stats={k: v for k, v in model.compress_stats.items() if not isinstance(v, dict)},
                   g1_cfg=model.G1_CFG)
        out["runs"].append(run)
        print(json.dumps(run), flush=True)
        del eng
        model._packed = []
        model.cache = None
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--only", default="")
    ap.add_argument("--layers", type=int, default=BB.CHAMELEON_30B.num_hidden_layers)
    ap.add_argument("--prompt", type=int, default=300)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.sweep:
        sweep(args)
    if args.step:
        step(args)


if __name__ == "__main__":
    main()
