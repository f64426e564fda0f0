#!/usr/bin/env python3
"""The 30B-class swin-norm Chameleon (backbones.CHAMELEON_30B) on one MI355X.

  --sweep   G1 launch shapes of its four projections at a 32-row window (window 16, CFG), uncompressed and 12-bit stream: us per launch
            from a hipGraph of back-to-back launches over enough weight copies that each streams from HBM.  One JSON line per shape;
            the fastest per projection is what G1_CFG_30B / G1_CFG_30B_Z hold.
  --step    ms per SJD step of the whole preset (synthetic weights drawn on the device, window 16, CFG, bf16) on the 12-bit stream and on
            the uncompressed packing (each packed once, before its timed decode), plus the projections' algorithmic bytes per step.
  --step --quant   the quantised streams (enable_fused(weights=..., swin_quant=True): LOSSY, opt-in) against the 12-bit stream with the protocol of
            tools/q8_bench.py --step: one process, one device, ONE set of 16-bit parameters, the legs 12-bit / e4m3 / mxfp4 (fused gate|up) / mxfp4
            (gate|up as G1q4 + F3, the same packed copy) alternating, --rounds timed rounds after an untimed one, the timed region at the mean KV
            length.  Per leg: ms per step (every round, the median), packed bytes per step, the projections' launch times at 32 rows and their
            fraction of the HBM peak on stored bytes; and whether the fused launch beats the unfused leg by more than that leg's spread.
"""
import argparse
import copy
import dataclasses
import json
import os
import statistics
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


PEAK = 8.0e12          # HBM bytes per second of one MI355X


def _spread(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), rounds=[round(t, 4) for t in v])


def _launch_us(model, rows, dev, rounds, fused):
    """us per launch of the four projections of `model` at `rows` window rows as its window forward runs them, over the layers' own packed copies"""
    a = model.args
    H, Hkv, D, hid, inter = model.n_heads, model.n_kv_heads, model.head_dim, a.hidden_size, a.intermediate_size
    out = {}
    for name, (N, K) in dict(qkv=((H + 2 * Hkv) * D, hid), o=(hid, H * D), gate_up=(2 * inter, hid), down=(hid, inter)).items():
        _, waves, sm = model.G1_CFG[name]
        KC = model._q8_chunk(name, rows, K)
        pk = [d[name] for d in model._packed]
        x = torch.randn(rows, K, device=dev).to(torch.bfloat16)
        one = name == "gate_up" and fused and isinstance(pk[0], ops.PackedQ4) and ops.gateup_silu_chunked_ok(rows, inter, hid, pk[0].KC)
        if one:
            run = lambda i: ops.gateup_silu(x, pk[i % len(pk)], inter, hid, sm)
        elif name == "gate_up":
            run = lambda i: ops.silu_mul(ops.skinny_gemm(x, pk[i % len(pk)], N, K, KC, waves, sm), rows=rows, dtype=x.dtype)
        else:
            run = lambda i: ops.skinny_gemm(x, pk[i % len(pk)], N, K, KC, waves, sm)
        us = [_graph_us(run, len(pk)) for _ in range(rounds)]
        size = pk[0].nbytes() if not isinstance(pk[0], torch.Tensor) else pk[0].numel() * pk[0].element_size()
        out[name] = dict(cfg=[KC, waves, int(sm)], launch="fused gate|up + SiLU" if one else ("projection + F3" if name == "gate_up" else "projection"),
                         us=_spread(us), stored_bytes=size, frac_of_8TBps_on_stored_bytes=round(size / (statistics.median(us) * 1e-6) / PEAK, 4))
    tot = sum(v["us"]["median"] for v in out.values())
    out["sum"] = dict(us=round(tot, 2), proj_ms_per_step=round(tot * len(model._packed) / 1e3, 3),
                      frac_of_8TBps_on_stored_bytes=round(sum(v["stored_bytes"] for v in out.values() if "stored_bytes" in v) / (tot * 1e-6) / PEAK, 4))
    return out


def step_quant(args):
    from sjd_amd.engine import SJDEngine, SJDConfig
    from sjd_amd.frontends import lumina_window_spec, lumina_prompt
    from sjd_amd.grammar import LuminaGrammar
    import sjd_amd.synthetic as synthetic
    dev = torch.device("cuda:0")
    margs = dataclasses.replace(BB.CHAMELEON_30B, num_hidden_layers=args.layers)
    with torch.device(dev):
        base = BB.ChameleonBackbone(margs, attn=None).to(torch.bfloat16).eval()
    synthetic.fill_state_dict_device(base, seed=0, embed_token_scale=0.7)
    torch.cuda.synchronize()
    window, grid, P = 16, 48, args.prompt
    n_img = grid * (grid + 1)
    prompt = lumina_prompt(P, grid, grid, seed=3)
    spec = lumina_window_spec(prompt, dev)
    cfg = SJDConfig(jacobi_loop_interval_l=0, jacobi_loop_interval_r=grid * grid + grid - 13, max_num_new_tokens=window, guidance_scale=3.0,
                    seed=3, max_length=P + n_img + 1, eos_token_ids=(8196,))
    lead = int(P + n_img // 2 - (args.steps / 2.0 + args.warmup))          # the timed region sits at the mean KV length (about one token per step)
    legs = {}

    def leg(tag, src, **kw):
        m = copy.copy(src)          # the same modules: one set of 16-bit parameters; packed copy, launch shapes, attention state and cache are the leg's own
        m.attn = ops.HipWindowAttention()
        m.gateup_route = {}
        if kw is not None and "fused" not in kw:
            m.__dict__.pop("G1_CFG", None)
            t0 = time.time()
            m.enable_fused(ops, gemm="sjd", **kw)
            torch.cuda.synchronize()
            pack_s = round(time.time() - t0, 1)
            for other in [base] + [lg["model"] for lg in legs.values()]:
                other._fused = m._fused          # (enable_fused re-points the shared parameters at fresh q|k|v / gate|up tensors: drop the old ones)
        else:
            m.gateup_fused, pack_s = kw["fused"], 0.0
        m.setup_cache(batch=2, s_max=((P + n_img + 2 * window + 64 + 31) // 32) * 32)
        if "fused" not in kw:
            m.gateup_route = {}          # (enable_fused made a new one; the unfused twin leg gets its own above)
        legs[tag] = dict(model=m, eng=SJDEngine(m, margs.vocab_size, dev, max_window=window, use_graph=True), ms=[], kv=[], tok=[], pack_s=pack_s)

    leg("z12", base, compress=True)
    leg("e4m3", base, weights="e4m3", swin_quant=True)
    leg("mxfp4", base, weights="mxfp4", swin_quant=True)
    legs["mxfp4"]["model"].gateup_fused = True
    leg("mxfp4_unfused", legs["mxfp4"]["model"], fused=False)
    tags = tuple(legs)
    sync = torch.cuda.synchronize
    for rnd in range(args.rounds + 1):          # round 0 is untimed practice: every hipGraph of the decode is captured in it
        for tag in tags:
            lg = legs[tag]
            _, st = lg["eng"].decode(prompt, spec, LuminaGrammar(2000, 10), cfg, warmup_iters=args.warmup, timed_iters=args.steps,
                                     on_timed_start=sync, on_timed_end=sync, lead_in_kv=lead)
            if rnd:
                lg["ms"].append(st.seconds / max(st.timed_nfe, 1) * 1e3)
                lg["kv"].append([st.kv_len_start, st.kv_len])
                lg["tok"].append(round(st.tokens / max(st.timed_nfe, 1), 3))
    rec = dict(device=torch.cuda.get_device_name(0), peak_TBps=PEAK / 1e12,
               workload=f"Chameleon-30B architecture (swin-norm, {args.layers} layers, synthetic weights), 1 prompt of {P} tokens, {grid}x{grid} image tokens, "
                        "draft window 16, CFG 3.0 (32 rows per forward), bf16, 16-bit KV cache",
               steps=args.steps, warmup=args.warmup, rounds=args.rounds, lead_in_kv=lead,
               order="alternating " + ", ".join(tags) + " per round after one untimed round; one process, one device, one set of 16-bit parameters",
               launch_shapes="UNTUNED: G1_CFG_30B_Q8 / G1_CFG_30B_Q4 are G1_CFG_30B_Z's values; no launch-shape sweep was run on either quantised stream",
               per_launch_method="one hipGraph of one launch per layer's packed copy, replayed three times, the fastest taken; median / min / max over the rounds")
    for tag, lg in legs.items():
        m = lg["model"]
        fused = tag == "mxfp4"
        rec[tag] = dict(weights=m.weights, gate_up_at_32_rows=m.gateup_route.get(2 * window) if m.weights else "g1z + f3", pack_s=lg["pack_s"],
                        G1_CFG={k: list(v) for k, v in m.G1_CFG.items()}, ms_per_step=_spread(lg["ms"]), kv_len=lg["kv"], tokens_per_step=lg["tok"],
                        packed_bytes_per_step=m.packed_bytes(head=False), compress_stats={k: v for k, v in m.compress_stats.items() if not isinstance(v, dict)},
                        per_launch_32_rows=_launch_us(m, 2 * window, dev, args.rounds, fused))
    f, u, z = rec["mxfp4"]["ms_per_step"], rec["mxfp4_unfused"]["ms_per_step"], rec["z12"]["ms_per_step"]
    rec["fused_minus_unfused_ms"] = round(f["median"] - u["median"], 4)
    rec["unfused_leg_spread_between_rounds_ms"] = round(u["max"] - u["min"], 4)
    rec["fused_faster_than_unfused_beyond_spread"] = bool(u["median"] - f["median"] > u["max"] - u["min"])
    rec["largest_spread_between_rounds_ms"] = round(max(rec[t]["ms_per_step"]["max"] - rec[t]["ms_per_step"]["min"] for t in tags), 4)
    for t in tags[1:]:
        rec[f"{t}_minus_z12_ms"] = round(rec[t]["ms_per_step"]["median"] - z["median"], 4)
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(rec, fh, indent=1)
            fh.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--quant", action="store_true", help="--step: the quantised legs (12-bit / e4m3 / mxfp4 fused / mxfp4 unfused), alternating")
    ap.add_argument("--rounds", type=int, default=3)
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
    if args.step and args.quant:
        step_quant(args)
    elif args.step:
        step(args)


if __name__ == "__main__":
    main()
