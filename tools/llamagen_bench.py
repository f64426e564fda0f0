#!/usr/bin/env python3
"""LlamaGen on one MI355X: the ATen window forward against the fused HIP path (LlamaGenBackbone.enable_fused).

  --sweep   G1 launch shapes of the four per-layer projections and the output head of one preset (default GPT-XL) at a --rows-row window
            (default 32: window 16, CFG; 128 / 256: four / eight prompts per forward, column-tile counts of kernel G1w, at most eight planes): us per launch from a hipGraph of back-to-back launches over enough weight copies that each streams from HBM.
            One JSON line per shape; the fastest per projection is what LlamaGenBackbone.G1_CFG_LLAMAGEN / HEAD_CFG hold.
  --ab      ms per SJD step, ATen against fused, for GPT-B c2i 256px, GPT-XL t2i 512px (120 caption rows, left-padded) and GPT-XXL t2i 512px
            on synthetic weights (window 16, CFG, bf16): both legs in the same process on the same weights, timed in alternation over
            --rounds rounds (median reported), captured hipGraphs in both; then one whole image per leg (tokens/s) and the packed bytes one
            fused step streams / step time / 8 TB/s.
  --batch   several prompts per forward (SJDBatchEngine): for the same three configurations ms per SJD step and accepted image tokens/s per GPU
            at 1 (SJDEngine on the default packing: the one-prompt path), 2, 4 and 8 prompts per forward (packed with max_rows 64 / 128 / 256),
            all legs in one process on the same weights, timed in alternation over --rounds rounds (median and the per-round values reported),
            the fraction of 8 TB/s each step streams; then F2's table rotary at 256 rows, GPT-XL shape: four heads per wave against one
            (SJD_F2_ONE_HEAD), us per launch from a hipGraph of back-to-back launches.  --only GPT-3B: the same legs for GPT-3B c2i 384px alone
            (pad_head_dim=True; above one prompt padded_batch=True), without the F2 part.
  --batch --detok   tokens -> pixels of a queue of whole GPT-B c2i 256px images (synthetic weights, a synthetic-weight VQ-16 in fp32) at 1 / 2 / 4 / 8
            prompts per forward (SJDBatchEngine, continuous batching over max(8, 2 x prompts) images): ms per image of the detokenizer alone,
            images/s with the images decoded serially after decode_many, images/s with decode_many(detokenize=) (every image decoded on the
            engine's side stream as its prompt ends).  The two queue legs alternate over --rounds rounds; medians, the per-round values and
            the spread between rounds are reported (profiles/llamagen_detok.json).  Replaces the --batch table: the default output is unchanged.
  --step    the fused step alone (one preset, --steps timed iterations): what the rocprofv3 by-shape table is taken from.
  --fused3b GPT-3B c2i 384px (24 layers, 32 heads of 100 stored 128 wide: enable_fused(pad_head_dim=True)), window 16, CFG, bf16: fused ms per SJD
            step over --rounds rounds (median), the packed bytes a step streams and their fraction of 8 TB/s.  No ATen leg: un-fused GPT-3B does
            not run on K1 (no head_dim-100 instantiation), so there is nothing to alternate with.
  --quant   the lossy weight streams (enable_fused(weights="e4m3" / "mxfp4")): GPT-XL t2i 512px and GPT-3B c2i 384px at --counts (default 1,8) prompts per
            forward, legs 16-bit / e4m3 / mxfp4 alternated over --rounds rounds (median and the rounds), then us per launch of GPT-3B's projections at
            128 / 256 rows on kernels G1w / G1wq / G1wq4 (profiles/llamagen_quant.json).
  --z       the LOSSLESS 12-bit stream (enable_fused(compress=True)): GPT-B c2i 256px, GPT-XL t2i 512px and GPT-3B c2i 384px at --counts (default 1,4)
            prompts per forward, legs 16-bit / 12-bit on the same weights and launch shapes alternated over --rounds rounds (median, min / max, the
            verdict against the larger round-to-round spread, the 16-bit leg against the recorded rounds), then us per launch of G1 against G1z at
            GPT-3B's four shapes, 32 and 128 rows (profiles/llamagen_z.json).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import sjd_amd.backbones as BB  # noqa: E402
import sjd_amd.ops as ops  # noqa: E402

PRESETS = {"GPT-B": (12, 12, 768), "GPT-L": (24, 16, 1024), "GPT-XL": (36, 20, 1280), "GPT-XXL": (48, 24, 1536), "GPT-3B": (24, 32, 3200)}
CONFIGS = [("GPT-B", "c2i", 256), ("GPT-XL", "t2i", 512), ("GPT-XXL", "t2i", 512)]
CONFIG_3B = ("GPT-3B", "c2i", 384)        # head_dim 100: fused only, with pad_head_dim=True (--fused3b)
PEAK_TBPS = 8.0
CAP_PAD = 7            # left-padded caption rows of the t2i runs (key_start)


def _args(preset, model_type, image_size):
    n_layer, n_head, dim = PRESETS[preset]
    latent = image_size // 16
    return BB.LlamaGenArgs(dim=dim, n_layer=n_layer, n_head=n_head, vocab_size=16384, block_size=latent * latent, model_type=model_type,
                           cls_token_num=1 if model_type == "c2i" else 120, num_classes=1000, caption_dim=2048)


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
    a = _args(args.preset, "t2i", 512)
    D = a.dim // a.n_head
    ff = int(2 * (4 * a.dim) / 3)
    inter = ff if ff % a.multiple_of == 0 else ff + a.multiple_of - (ff % a.multiple_of)
    DS = 128 if D == 100 else D           # (a head_dim of 100 is stored 128 wide: the o projection's K is H * 128, zero columns at the pad positions)
    shapes = dict(qkv=(3 * a.n_head * D, a.dim), o=(a.dim, a.n_head * DS), gate_up=(2 * inter, a.dim), down=(a.dim, inter), head=(a.vocab_size, a.dim))
    # split-K chunks: the sets' 128..1280, and for GPT-3B the multiples of 16 that leave at most eight planes of K = 3200 / 4096 / 8704
    kcs = (128, 256, 320, 512, 640, 1280) if D != 100 else (400, 512, 640, 800, 1088, 1280, 1600, 2176)
    dev = torch.device("cuda:0")
    M = args.rows
    max_planes = 8 if (M > 64 or D == 100) else None
    g = torch.Generator(device=dev).manual_seed(1)
    best = {}
    for name, (N, K) in shapes.items():
        copies = max(2, -(-768 * 2**20 // (N * K * 2)))        # > 0.75 GB in flight: past the 256 MB Infinity Cache
        ws = [(torch.randn(N, K, generator=g, device=dev) / K ** 0.5).to(torch.bfloat16) for _ in range(copies)]
        x = torch.randn(M, K, generator=g, device=dev).to(torch.bfloat16)
        for kc in kcs:
            if kc > K or (max_planes and name != "head" and -(-K // kc) > max_planes):       # (the wider sets and GPT-3B: at most eight split-K planes, the limit the 32-row set observes)
                continue
            if kc > (2560 if M <= 32 else 1280) and M <= 64:       # (the staged activation chunk must fit in LDS)
                continue
            for sm in (True, False):
                packed = [ops.pack_weight(w, kc, sm) for w in ws]
                for waves in ((1, 2, 4, 8) if M <= 64 else (2, 3, 4, 6, 8)):       # (above 64 rows: the column-tile counts of kernel G1w)
                    try:
                        if name == "head":
                            fn = lambda i: ops.skinny_gemm_cols(x, packed[i % copies], N, K, kc, 0, N, waves, sm)
                        else:
                            fn = lambda i: ops.skinny_gemm(x, packed[i % copies], N, K, kc, waves, sm)
                        us = _graph_us(fn, 2 * copies)
                    except Exception as e:          # a launch shape the kernel declines
                        print(json.dumps(dict(proj=name, kc=kc, waves=waves, step_major=sm, error=str(e)[:80])), flush=True)
                        continue
                    rec = dict(preset=args.preset, proj=name, N=N, K=K, rows=M, kc=kc, waves=waves, step_major=sm, us=round(us, 2),
                               tbps=round(N * K * 2 / us / 1e6, 3))
                    print(json.dumps(rec), flush=True)
                    if name not in best or us < best[name]["us"]:
                        best[name] = rec
                del packed
        del ws
        torch.cuda.empty_cache()
    for name, r in best.items():
        print(json.dumps(dict(best=name, preset=args.preset, cfg=[r["kc"], r["waves"], r["step_major"]], us=r["us"], tbps=r["tbps"])), flush=True)


DTYPES = dict(bf16=torch.bfloat16, fp16=torch.float16)


def _make(preset, model_type, image_size, dev, dtype=torch.bfloat16):
    import sjd_amd.synthetic as synthetic
    a = _args(preset, model_type, image_size)
    with torch.device(dev):
        m = BB.LlamaGenBackbone(a, attn=ops.HipWindowAttention()).to(dtype).eval()
    synthetic.fill_state_dict_device(m, seed=0, embed_token_scale=0.5)
    return m


class _Leg:
    """one backbone (ATen or fused) with its cache, prefill and engine"""

    def __init__(self, model, window, dev, seed=3):
        from sjd_amd.engine import SJDEngine
        self.m, self.window, self.dev = model, window, dev
        a = model.args
        self.T, self.N = a.cls_token_num, a.block_size
        g = torch.Generator(device=dev).manual_seed(seed)
        if a.model_type == "c2i":
            self.cond = torch.tensor([207, a.num_classes], device=dev)
            self.ks = torch.zeros(2, dtype=torch.int32, device=dev)
        else:
            cap = (torch.randn(1, self.T, a.caption_dim, generator=g, device=dev) * 0.5).to(model.output.weight.dtype)
            self.cond = torch.cat([cap, torch.zeros_like(cap) + model.cls_embedding.uncond_embedding.to(cap.dtype)])
            self.ks = torch.full((2,), CAP_PAD, dtype=torch.int32, device=dev)          # left-padded caption: the first rows are hidden
        self.s_max = ((self.T + self.N + window + 32 + 31) // 32) * 32
        model.setup_cache(batch=2, s_max=self.s_max)
        self.eng = SJDEngine(model, a.vocab_size, dev, max_window=window, use_graph=True)

    def prefill(self):
        m = self.m
        m.attn.params = None
        pos = torch.arange(self.T, device=self.dev)[None].repeat(2, 1)
        lg = m.forward_embeds(m.embed_condition(self.cond), pos, 0, self.ks)
        return int(lg[0, -1].argmax())

    def decode(self, warmup=0, steps=None):
        from sjd_amd.engine import SJDConfig, WindowSpec
        from sjd_amd.grammar import TopKTopPGrammar
        first = self.prefill()
        T, N, w = self.T, self.N, self.window
        cfg = SJDConfig(jacobi_loop_interval_l=1, jacobi_loop_interval_r=N - w - 2, max_num_new_tokens=w, guidance_scale=4.0, seed=3,
                        max_length=N)
        spec = WindowSpec(first_tokens=torch.tensor([[first], [first]], device=self.dev),
                          first_positions=torch.full((2, 1), T, dtype=torch.long, device=self.dev), key_start=self.ks,
                          pos_offset=torch.zeros(2, dtype=torch.long), kv_base=T)
        kw = {} if steps is None else dict(warmup_iters=warmup, timed_iters=steps, on_timed_start=torch.cuda.synchronize,
                                           on_timed_end=torch.cuda.synchronize)
        torch.cuda.synchronize()
        t0 = time.time()
        seq, st = self.eng.decode([first], spec, TopKTopPGrammar(1000, 1.0), cfg, **kw)
        torch.cuda.synchronize()
        return seq, st, time.time() - t0


def ab(args):
    dev = torch.device("cuda:0")
    out = []
    for preset, mt, size in CONFIGS:
        if args.only and preset not in args.only.split(","):
            continue
        aten = _make(preset, mt, size, dev)
        fused = _make(preset, mt, size, dev)
        fused.load_state_dict(aten.state_dict())
        fused.enable_fused(ops, gemm="sjd")
        legs = dict(aten=_Leg(aten, args.window, dev), fused=_Leg(fused, args.window, dev))
        ms = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, leg in legs.items():
                _, st, _ = leg.decode(args.warmup, args.steps)
                ms[k].append(1e3 * st.seconds / max(1, st.timed_nfe))
        whole = {}
        for k, leg in legs.items():
            seq, st, wall = leg.decode()
            whole[k] = dict(tokens=len(seq) - 1, nfe=st.nfe, seconds=round(wall, 3), tokens_per_s=round((len(seq) - 1) / wall, 1))
        med = {k: statistics.median(v) for k, v in ms.items()}
        nbytes = fused.packed_bytes()
        rec = dict(preset=preset, model_type=mt, image_size=size, window=args.window, cfg=True, dtype="bf16",
                   cls_token_num=fused.args.cls_token_num, key_start=int(legs["fused"].ks[0]), layers=fused.n_layers,
                   ms_per_step=dict(aten=round(med["aten"], 3), fused=round(med["fused"], 3)),
                   ms_per_step_rounds={k: [round(x, 3) for x in v] for k, v in ms.items()},
                   speedup=round(med["aten"] / med["fused"], 2), whole_image=whole,
                   packed_gb_per_step=round(nbytes / 1e9, 3),
                   fused_fraction_of_8tbps=round(nbytes / (med["fused"] * 1e-3) / (PEAK_TBPS * 1e12), 3),
                   g1_cfg=fused.G1_CFG, head_cfg=list(fused.HEAD_CFG))
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del legs, aten, fused
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


class _BatchLeg:
    """P prompts per forward on one fused backbone (its own cache and engine); every prompt its own conditioning"""

    def __init__(self, model, P, window, dev):
        from sjd_amd.engine_batch import SJDBatchEngine
        self.m, self.P, self.window, self.dev = model, P, window, dev
        a = model.args
        self.T, self.N = a.cls_token_num, a.block_size
        self.s_max = ((self.T + self.N + window + 32 + 31) // 32) * 32
        model.setup_cache(batch=2 * P, s_max=self.s_max)
        self.eng = SJDBatchEngine(model, a.vocab_size, dev, P, max_window=window, use_graph=True)

    def decode(self, warmup, steps):
        from sjd_amd.engine import SJDConfig, WindowSpec
        from sjd_amd.grammar import TopKTopPGrammar
        m, a, T, N, w, dev = self.m, self.m.args, self.T, self.N, self.window, self.dev
        specs = []
        for j in range(self.P):
            if a.model_type == "c2i":
                cond, ks = torch.tensor([(207 + 101 * j) % 1000, a.num_classes], device=dev), torch.zeros(2, dtype=torch.int32)
            else:
                cap = (torch.randn(1, T, a.caption_dim, generator=torch.Generator().manual_seed(3 + j)) * 0.5).to(dev, m.output.weight.dtype)
                cond = torch.cat([cap, torch.zeros_like(cap) + m.cls_embedding.uncond_embedding.to(cap.dtype)])
                ks = torch.full((2,), CAP_PAD, dtype=torch.int32)
            specs.append(WindowSpec(first_tokens=None, first_positions=None, key_start=ks, pos_offset=torch.zeros(2, dtype=torch.long), kv_base=T,
                                    cond_embeds=m.embed_condition(cond), cond_sampling=dict(cfg_scale=4.0, top_k=1000, top_p=1.0)))
        cfg = SJDConfig(jacobi_loop_interval_l=1, jacobi_loop_interval_r=N - w - 2, max_num_new_tokens=w, guidance_scale=4.0, seed=3, max_length=N)
        self.eng.decode_many([[] for _ in specs], specs, [TopKTopPGrammar(1000, 1.0) for _ in specs], cfg, warmup_iters=warmup, timed_iters=steps,
                             on_timed_start=torch.cuda.synchronize, on_timed_end=torch.cuda.synchronize)
        rs = self.eng.run_stats
        return 1e3 * rs["seconds"] / max(1, rs["timed_iterations"]), rs["tokens"] / rs["seconds"]


def _f2_ab(dev, rows=256, H=20, D=64, hid=1280):
    """F2's table rotary at `rows` rows, GPT-XL shape, planes source: us per launch, four heads per wave against one (SJD_F2_ONE_HEAD)"""
    g = torch.Generator(device=dev).manual_seed(2)
    S, N, n = 1216, 3 * H * D, 16
    B = rows // n
    table = BB._rope_table_extended(BB._rope_2d_table(32, D, 10000, 120).to(dev), S)
    copies = 24
    parts = [ops.Partials(torch.randn(5, rows, N, generator=g, device=dev), 5, N) for _ in range(copies)]       # (K 1280 in chunks of 256)
    kc = torch.zeros(B, H, S, D, dtype=torch.bfloat16, device=dev)
    vc = torch.zeros_like(kc)
    pos = (400 + torch.arange(n, device=dev))[None].repeat(B, 1).reshape(-1).contiguous()
    ss = torch.rand(3, rows, device=dev) * hid
    out = {}
    for name, one_head in (("rows_kernel", False), ("one_head_kernel", True), ("rows_kernel_again", False)):
        fn = lambda i: ops.qknorm_rope_append(parts[i % copies], kc, vc, None, None, None, None, None, pos, B, n, H, H, D, None, 400,
                                              dtype=torch.bfloat16, row_norm=(ss, hid, 1e-5), rope_table=table, one_head=one_head)
        out[name] = round(_graph_us(fn, 4 * copies), 2)
    return dict(shape=dict(rows=rows, H=H, D=D, planes=5), us_per_launch=out)


def batch(args):
    """--dtype bf16 / fp16: one type; both: the legs of both types in every round, alternated (fp16 beside its bf16 twin from one session).
    --counts: prompts per forward to measure (1 = SJDEngine, more = SJDBatchEngine)."""
    dev = torch.device("cuda:0")
    names = ["bf16", "fp16"] if args.dtype == "both" else [args.dtype]
    counts = [int(c) for c in args.counts.split(",")]
    out = dict(configs=[], window=args.window, cfg=True, dtype=args.dtype, rounds=args.rounds, steps=args.steps, warmup=args.warmup)
    only = args.only.split(",") if args.only else []
    for preset, mt, size in CONFIGS + ([CONFIG_3B] if "GPT-3B" in only else []):          # (GPT-3B on request only: the default run is what it was)
        if only and preset not in only:
            continue
        models, legs = {}, {}
        for dn in names:
            base = _make(preset, mt, size, dev, DTYPES[dn])
            for P in counts:
                m = models[dn, P] = base if P == counts[0] else _make(preset, mt, size, dev, DTYPES[dn])
                if m is not base:
                    m.load_state_dict(base.state_dict())
            for P in counts:
                rows = P * 2 * args.window
                models[dn, P].enable_fused(ops, gemm="sjd", max_rows=64 if rows <= 64 else (128 if rows <= 128 else 256), untuned_fp16=True,
                                           pad_head_dim=preset == "GPT-3B", padded_batch=preset == "GPT-3B" and rows > 64)
                legs[dn, P] = _Leg(models[dn, P], args.window, dev) if P == 1 else _BatchLeg(models[dn, P], P, args.window, dev)
        ms, tps = {k: [] for k in legs}, {k: [] for k in legs}
        for _ in range(args.rounds):
            for P in counts:
                for dn in names:
                    leg = legs[dn, P]
                    if P == 1:
                        _, st, _ = leg.decode(args.warmup, args.steps)
                        ms[dn, P].append(1e3 * st.seconds / max(1, st.timed_nfe))
                        tps[dn, P].append(st.tokens / st.seconds)
                    else:
                        a_, b_ = leg.decode(args.warmup, args.steps)
                        ms[dn, P].append(a_)
                        tps[dn, P].append(b_)
        for dn in names:
            med_ms = {P: statistics.median(ms[dn, P]) for P in counts}
            med_tps = {P: statistics.median(tps[dn, P]) for P in counts}
            m0 = models[dn, counts[0]]
            rec = dict(preset=preset, model_type=mt, image_size=size, layers=m0.n_layers, head_dim=m0.head_dim, head_dim_stored=m0.cache.k.shape[-1],
                       ms_per_step={str(P): round(v, 3) for P, v in med_ms.items()},
                       tokens_per_s={str(P): round(v, 1) for P, v in med_tps.items()},
                       ms_per_step_rounds={str(P): [round(x, 3) for x in ms[dn, P]] for P in counts},
                       tokens_per_s_rounds={str(P): [round(x, 1) for x in tps[dn, P]] for P in counts},
                       tokens_per_s_vs_one_prompt={str(P): round(med_tps[P] / med_tps[counts[0]], 2) for P in counts},
                       prompt_steps_per_s_vs_one_prompt={str(P): round(P * med_ms[counts[0]] / (counts[0] * med_ms[P]), 2) for P in counts},
                       packed_gb_per_step={str(P): round(models[dn, P].packed_bytes() / 1e9, 3) for P in counts},
                       fraction_of_8tbps={str(P): round(models[dn, P].packed_bytes() / (med_ms[P] * 1e-3) / (PEAK_TBPS * 1e12), 3) for P in counts},
                       g1_cfg={str(P): [models[dn, P].G1_CFG, list(models[dn, P].HEAD_CFG)] for P in counts})
            if args.dtype == "both":
                rec["dtype"] = dn
            print(json.dumps(rec), flush=True)
            out["configs"].append(rec)
        del legs, models, base
        torch.cuda.empty_cache()
    if args.dtype == "bf16" and only != ["GPT-3B"]:
        out["f2_table_256rows"] = _f2_ab(dev)
        print(json.dumps(out["f2_table_256rows"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


def quant(args):
    """--quant: ms per SJD step from 16-bit, e4m3 and MXFP4 weights (LlamaGenBackbone.enable_fused(weights=...): LOSSY streams, synthetic weights), GPT-XL
    t2i 512px and GPT-3B c2i 384px, --counts prompts per forward (default 1,8); one process, the legs alternated in every round, medians and the rounds.
    Then us per launch of the GPT-3B projections at 128 / 256 rows on kernels G1w / G1wq / G1wq4 (the quantised set's shapes)."""
    dev = torch.device("cuda:0")
    counts = [int(c) for c in (args.counts if args.counts != "1,2,4,8" else "1,8").split(",")]
    streams = [None, "e4m3", "mxfp4"]
    only = args.only.split(",") if args.only else []
    out = dict(configs=[], window=args.window, cfg=True, rounds=args.rounds, steps=args.steps, warmup=args.warmup,
               note="synthetic weights; e4m3 / mxfp4 are LOSSY (rel_rms_error below is all there is to judge them by: image quality is NOT measured); "
                    "the quantised launch shapes are UNTUNED (launch_shapes.LLAMAGEN_QUANT_SETS)")
    for preset, mt, size in (CONFIGS[1], CONFIG_3B):
        if only and preset not in only:
            continue
        base = _make(preset, mt, size, dev)
        models, legs = {}, {}
        for wt in streams:
            for P in counts:
                m = models[wt, P] = _make(preset, mt, size, dev)
                m.load_state_dict(base.state_dict())
                rows = P * 2 * args.window
                m.enable_fused(ops, gemm="sjd", max_rows=64 if rows <= 64 else (128 if rows <= 128 else 256), pad_head_dim=preset == "GPT-3B",
                               padded_batch=preset == "GPT-3B" and rows > 64, weights=wt)
                legs[wt, P] = _Leg(m, args.window, dev) if P == 1 else _BatchLeg(m, P, args.window, dev)
        del base
        ms = {k: [] for k in legs}
        for _ in range(args.rounds):
            for P in counts:
                for wt in streams:
                    if P == 1:
                        _, st, _ = legs[wt, P].decode(args.warmup, args.steps)
                        ms[wt, P].append(1e3 * st.seconds / max(1, st.timed_nfe))
                    else:
                        ms[wt, P].append(legs[wt, P].decode(args.warmup, args.steps)[0])
        for wt in streams:
            med = {P: statistics.median(ms[wt, P]) for P in counts}
            rec = dict(preset=preset, model_type=mt, image_size=size, weights=wt or "bf16", layers=models[wt, counts[0]].n_layers,
                       ms_per_step={str(P): round(v, 3) for P, v in med.items()},
                       ms_per_step_rounds={str(P): [round(x, 3) for x in ms[wt, P]] for P in counts},
                       ms_vs_bf16={str(P): round(med[P] / statistics.median(ms[None, P]), 3) for P in counts},
                       packed_gb_per_step={str(P): round(models[wt, P].packed_bytes() / 1e9, 3) for P in counts},
                       rel_rms_error=models[wt, counts[0]].compress_stats.get("rel_rms_error"),
                       g1_cfg={str(P): models[wt, P].G1_CFG for P in counts})
            print(json.dumps(rec), flush=True)
            out["configs"].append(rec)
        del legs, models
        torch.cuda.empty_cache()
    # per launch: GPT-3B's projections (o reads heads stored 128 wide) on the quantised 256-row set, weights cycled past the Infinity Cache
    cfg = BB.LS.LLAMAGEN_QUANT_SETS[True, 256][0]
    shapes = BB.LS.llamagen_dims(3200, 32, 100, 8704, 128)
    g = torch.Generator(device=dev).manual_seed(1)
    launches = []
    for name, (N, K) in shapes.items():
        kc, tiles, sm = cfg[name]
        copies = max(2, -(-768 * 2**20 // (N * K * 2)))
        ws = [(torch.randn(N, K, generator=g, device=dev) / K ** 0.5).to(torch.bfloat16) for _ in range(copies)]
        packs = dict(G1w=[ops.pack_weight(w, kc, sm) for w in ws], G1wq=[ops.pack_weight_q8(w, kc, sm) for w in ws], G1wq4=[ops.pack_weight_q4(w, kc, sm) for w in ws])
        for M in (128, 256):
            x = torch.randn(M, K, generator=g, device=dev).to(torch.bfloat16)
            us = {kn: round(_graph_us(lambda i: ops.skinny_gemm(x, pk[i % copies], N, K, kc, tiles, sm), 2 * copies), 2) for kn, pk in packs.items()}
            rec = dict(proj=name, N=N, K=K, rows=M, cfg=[kc, tiles, sm], us_per_launch=us)
            print(json.dumps(rec), flush=True)
            launches.append(rec)
        del ws, packs
        torch.cuda.empty_cache()
    out["gpt_3b_launches"] = launches
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


def _recorded_16bit(preset, P):
    """(min, max) ms per step of the 16-bit leg's recorded rounds at P prompts per forward (profiles/llamagen_batch.json, llamagen_3b_batch.json), or None"""
    name = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "llamagen_3b_batch.json" if preset == "GPT-3B" else "llamagen_batch.json")
    try:
        rec = next(c for c in json.load(open(name))["configs"] if c["preset"] == preset)
        return min(rec["ms_per_step_rounds"][str(P)]), max(rec["ms_per_step_rounds"][str(P)])
    except (OSError, KeyError, StopIteration):
        return None


def zstream(args):
    """--z: ms per SJD step from 16-bit weights and from the LOSSLESS 12-bit stream (LlamaGenBackbone.enable_fused(compress=True)) on the same synthetic
    weights and the same launch shapes: GPT-B c2i 256px, GPT-XL t2i 512px and GPT-3B c2i 384px at --counts (default 1,4) prompts per forward; one
    process, the two legs alternated in every round, medians with min / max.  The 12-bit leg counts as faster (or slower) only where the gap exceeds the
    larger of the two legs' round-to-round spreads; the 16-bit leg is held against the rounds recorded in profiles/llamagen_batch.json /
    llamagen_3b_batch.json.  Then us per launch of G1 against G1z at GPT-3B's four shapes (o with the zero pad columns of heads stored 128 wide)."""
    dev = torch.device("cuda:0")
    counts = [int(c) for c in (args.counts if args.counts != "1,2,4,8" else "1,4").split(",")]
    only = args.only.split(",") if args.only else []
    out = dict(configs=[], window=args.window, cfg=True, rounds=args.rounds, steps=args.steps, warmup=args.warmup,
               note="synthetic weights; the 12-bit stream is lossless (bit-identical planes), its launch shapes are the 16-bit ones (UNTUNED: launch_shapes.LLAMAGEN_Z_SETS)")
    for preset, mt, size in (CONFIGS[0], CONFIGS[1], CONFIG_3B):
        if only and preset not in only:
            continue
        base = _make(preset, mt, size, dev)
        models, legs = {}, {}
        for z in (False, True):
            for P in counts:
                m = models[z, P] = _make(preset, mt, size, dev)
                m.load_state_dict(base.state_dict())
                rows = P * 2 * args.window
                m.enable_fused(ops, gemm="sjd", max_rows=64 if rows <= 64 else 128, pad_head_dim=preset == "GPT-3B", padded_batch=preset == "GPT-3B" and rows > 64,
                               compress=z)
                legs[z, P] = _Leg(m, args.window, dev) if P == 1 else _BatchLeg(m, P, args.window, dev)
        del base
        ms = {k: [] for k in legs}
        for _ in range(args.rounds):
            for P in counts:
                for z in (False, True):
                    if P == 1:
                        _, st, _ = legs[z, P].decode(args.warmup, args.steps)
                        ms[z, P].append(1e3 * st.seconds / max(1, st.timed_nfe))
                    else:
                        ms[z, P].append(legs[z, P].decode(args.warmup, args.steps)[0])
        rec = dict(preset=preset, model_type=mt, image_size=size, layers=models[False, counts[0]].n_layers, prompts_per_forward={})
        for P in counts:
            med = {z: statistics.median(ms[z, P]) for z in (False, True)}
            spread = max(max(ms[z, P]) - min(ms[z, P]) for z in (False, True))
            gain = med[False] - med[True]
            was = _recorded_16bit(preset, P)
            st = models[True, P].compress_stats
            rec["prompts_per_forward"][str(P)] = dict(
                ms_per_step={n: dict(median=round(med[z], 3), min=round(min(ms[z, P]), 3), max=round(max(ms[z, P]), 3), rounds=[round(x, 3) for x in ms[z, P]])
                             for n, z in (("bf16", False), ("z12", True))},
                gain_ms=round(gain, 3), larger_round_spread_ms=round(spread, 3),
                verdict="12-bit faster" if gain > spread else "12-bit slower" if -gain > spread else "no difference beyond the round-to-round spread",
                z12_vs_bf16=round(med[True] / med[False], 3),
                packed_gb_per_step=dict(bf16=round(models[False, P].packed_bytes() / 1e9, 3), z12=round(models[True, P].packed_bytes() / 1e9, 3)),
                bytes_packed_over_raw=round(st["bytes_packed"] / st["bytes_raw"], 4), raw_units=st["raw_units"], units=st.get("units"),
                recorded_bf16_rounds_min_max=was,
                bf16_inside_recorded_spread=None if was is None else bool(was[0] <= med[False] <= was[1]),
                g1_cfg=models[True, P].G1_CFG, head_cfg=list(models[True, P].HEAD_CFG))
            if was is not None and not was[0] <= med[False] <= was[1]:
                rec["prompts_per_forward"][str(P)]["box_note"] = (f"the 16-bit leg ({med[False]:.3f} ms) lies outside the recorded rounds {was[0]:.3f}..{was[1]:.3f} ms: "
                                                                  "this box (or its software) is not the one of the recorded profile; compare the two legs of this run only")
        print(json.dumps(rec), flush=True)
        out["configs"].append(rec)
        del legs, models
        torch.cuda.empty_cache()
    # per launch: GPT-3B's projections on the 12-bit set's shapes, 32 and 128 rows, weights cycled past the Infinity Cache
    shapes = BB.LS.llamagen_dims(3200, 32, 100, 8704, 128)
    g = torch.Generator(device=dev).manual_seed(1)
    launches = []
    for name, (N, K) in shapes.items():
        copies = max(2, -(-768 * 2**20 // (N * K * 2)))
        ws = [(torch.randn(N, K, generator=g, device=dev) / K ** 0.5).to(torch.bfloat16) for _ in range(copies)]
        if name == "o":          # heads of 100 stored 128 wide: zero columns at the pad positions (every unit of the 12-bit copy then travels verbatim)
            for w in ws:
                w.view(N, 32, 128)[:, :, 100:] = 0
        for M, pad_rows in ((32, 64), (128, 128)):
            kc, tiles, sm = BB.LS.LLAMAGEN_Z_SETS[True, pad_rows][0][name]
            packs = dict(G1=[ops.pack_weight(w, kc, sm) for w in ws], G1z=[ops.pack_weight_z(w, kc, sm) for w in ws])
            x = torch.randn(M, K, generator=g, device=dev).to(torch.bfloat16)
            us = {kn: round(_graph_us(lambda i: ops.skinny_gemm(x, pk[i % copies], N, K, kc, tiles, sm), 2 * copies), 2) for kn, pk in packs.items()}
            rec = dict(proj=name, N=N, K=K, rows=M, cfg=[kc, tiles, sm], us_per_launch=us, raw_units=packs["G1z"][0].n_raw, units=packs["G1z"][0].stats["units"],
                       bytes_z_over_16bit=round(packs["G1z"][0].nbytes() / (N * K * 2), 4))
            print(json.dumps(rec), flush=True)
            launches.append(rec)
            del packs
        del ws
        torch.cuda.empty_cache()
    out["gpt_3b_launches"] = launches
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


def detok(args):
    from llamagen.tokenizer.tokenizer_image.vq_model import VQ_models
    from sjd_amd.detokenizers import to_uint8
    from sjd_amd.engine import SJDConfig, WindowSpec
    from sjd_amd.engine_batch import SJDBatchEngine
    from sjd_amd.grammar import TopKTopPGrammar
    import sjd_amd.synthetic as synthetic
    dev = torch.device("cuda:0")
    preset, mt, size = CONFIGS[0]
    latent, w = size // 16, args.window
    vq = synthetic.fill_state_dict_conv(VQ_models["VQ-16"](codebook_size=16384, codebook_embed_dim=8).eval(), seed=1).to(dev)
    decode = lambda ids: to_uint8(vq.decode_code(ids[-latent * latent:], (1, 8, latent, latent)))[0]
    counts = [int(c) for c in args.counts.split(",")]
    out = dict(preset=preset, model_type=mt, image_size=size, window=w, cfg=True, dtype="bf16", vq="VQ-16 fp32, synthetic weights", rounds=args.rounds,
               counts={})
    # the detokenizer alone: one image per call on the default stream, nothing else on the device
    ids0 = torch.randint(0, 16384, (latent * latent,), device=dev, generator=torch.Generator(dev).manual_seed(0))
    for _ in range(3):
        decode(ids0)
    alone = []
    for _ in range(args.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(10):
            decode(ids0)
        e1.record()
        torch.cuda.synchronize()
        alone.append(e0.elapsed_time(e1) / 10)
    out["detok_ms_per_image"] = round(statistics.median(alone), 3)
    out["detok_ms_per_image_rounds"] = [round(x, 3) for x in alone]
    print(json.dumps(dict(detok_ms_per_image=out["detok_ms_per_image"], rounds=out["detok_ms_per_image_rounds"])), flush=True)
    base = _make(preset, mt, size, dev)
    for P in counts:
        m = _make(preset, mt, size, dev)
        m.load_state_dict(base.state_dict())
        rows = P * 2 * w
        m.enable_fused(ops, gemm="sjd", max_rows=64 if rows <= 64 else (128 if rows <= 128 else 256))
        T, N = m.args.cls_token_num, m.args.block_size
        m.setup_cache(batch=2 * P, s_max=((T + N + w + 32 + 31) // 32) * 32)
        eng = SJDBatchEngine(m, m.args.vocab_size, dev, P, max_window=w, use_graph=True)
        Q = max(8, 2 * P)
        cfg = SJDConfig(jacobi_loop_interval_l=1, jacobi_loop_interval_r=N - w - 2, max_num_new_tokens=w, guidance_scale=4.0, seed=3, max_length=N)

        def queue(overlap):
            specs = [WindowSpec(first_tokens=None, first_positions=None, key_start=torch.zeros(2, dtype=torch.int32),
                                pos_offset=torch.zeros(2, dtype=torch.long), kv_base=T,
                                cond_embeds=m.embed_condition(torch.tensor([(207 + 101 * j) % 1000, m.args.num_classes], device=dev)),
                                cond_sampling=dict(cfg_scale=4.0, top_k=1000, top_p=1.0)) for j in range(Q)]
            grammars = [TopKTopPGrammar(1000, 1.0) for _ in range(Q)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if overlap:
                res, images = eng.decode_many([[] for _ in specs], specs, grammars, cfg, detokenize=decode)
            else:
                res = eng.decode_many([[] for _ in specs], specs, grammars, cfg)
                images = [decode(torch.tensor(seq, dtype=torch.long, device=dev)) for seq, _ in res]
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert len(images) == Q and all(im.shape == (size, size, 3) for im in images)
            return Q / dt, [seq for seq, _ in res]

        ips = dict(serial=[], overlap=[])
        _, a = queue(False)                      # untimed: graph captures, convolution algorithm search
        _, b = queue(True)
        assert a == b, "the overlapped queue decodes the tokens of the serial one"
        for _ in range(args.rounds):
            for leg in ("serial", "overlap"):
                ips[leg].append(queue(leg == "overlap")[0])
        med = {k: statistics.median(v) for k, v in ips.items()}
        rec = dict(prompts_per_forward=P, images=Q, images_per_s={k: round(v, 2) for k, v in med.items()},
                   images_per_s_rounds={k: [round(x, 2) for x in v] for k, v in ips.items()},
                   spread_between_rounds={k: round((max(v) - min(v)) / med[k], 3) for k, v in ips.items()},
                   overlap_vs_serial=round(med["overlap"] / med["serial"], 3),
                   detok_share_of_serial=round(out["detok_ms_per_image"] * 1e-3 * med["serial"], 3))
        print(json.dumps(rec), flush=True)
        out["counts"][str(P)] = rec
        del eng, m
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


def step(args):
    dev = torch.device("cuda:0")
    preset, mt, size = next(c for c in CONFIGS + [CONFIG_3B] if c[0] == args.preset)
    m = _make(preset, mt, size, dev, DTYPES[args.dtype])
    pad = preset == "GPT-3B"             # (head_dim 100 stored 128 wide; several prompts per forward: its own swept sets, padded_batch=True)
    if args.prompts > 1:
        rows = args.prompts * 2 * args.window
        m.enable_fused(ops, gemm="sjd", max_rows=64 if rows <= 64 else (128 if rows <= 128 else 256), untuned_fp16=True, pad_head_dim=pad,
                       padded_batch=pad and rows > 64)
        ms, tps = _BatchLeg(m, args.prompts, args.window, dev).decode(args.warmup, args.steps)
        print(json.dumps(dict(preset=preset, prompts=args.prompts, ms_per_step=round(ms, 3), tokens_per_s=round(tps, 1))), flush=True)
        return
    m.enable_fused(ops, gemm="sjd", pad_head_dim=pad)
    leg = _Leg(m, args.window, dev)
    _, st, _ = leg.decode(args.warmup, args.steps)
    print(json.dumps(dict(preset=preset, ms_per_step=round(1e3 * st.seconds / max(1, st.timed_nfe), 3), timed_steps=st.timed_nfe)), flush=True)


def fused3b(args):
    dev = torch.device("cuda:0")
    preset, mt, size = CONFIG_3B
    m = _make(preset, mt, size, dev)
    if args.cfg_from:            # launch shapes from the `best` lines of a --sweep output instead of LlamaGenBackbone.G1_CFG_LLAMAGEN_3B (a caller's set wins)
        best = {r["best"]: tuple(r["cfg"]) for r in map(json.loads, open(args.cfg_from)) if "best" in r}
        m.G1_CFG = {k: best[k] for k in ("qkv", "o", "gate_up", "down")}
        m.HEAD_CFG = best["head"]
    m.enable_fused(ops, gemm="sjd", pad_head_dim=True)
    leg = _Leg(m, args.window, dev)
    ms = []
    for _ in range(args.rounds):
        _, st, _ = leg.decode(args.warmup, args.steps)
        ms.append(1e3 * st.seconds / max(1, st.timed_nfe))
    seq, st, wall = leg.decode()
    med, nbytes = statistics.median(ms), m.packed_bytes()
    rec = dict(preset=preset, model_type=mt, image_size=size, window=args.window, cfg=True, dtype="bf16", layers=m.n_layers, head_dim=m.head_dim,
               head_dim_stored=m.cache.k.shape[-1], prompts_per_forward=1, ms_per_step=dict(fused=round(med, 3)),
               ms_per_step_rounds=dict(fused=[round(x, 3) for x in ms]), aten=None,
               aten_note="no ATen leg: un-fused GPT-3B does not run on K1 (head_dim 100 has no instantiation)",
               whole_image=dict(tokens=len(seq) - 1, nfe=st.nfe, seconds=round(wall, 3), tokens_per_s=round((len(seq) - 1) / wall, 1)),
               packed_gb_per_step=round(nbytes / 1e9, 3), fused_fraction_of_8tbps=round(nbytes / (med * 1e-3) / (PEAK_TBPS * 1e12), 3),
               g1_cfg=m.G1_CFG, head_cfg=list(m.HEAD_CFG))
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump([rec], f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--batch", action="store_true")
    ap.add_argument("--fused3b", action="store_true")
    ap.add_argument("--quant", action="store_true", help="16-bit / e4m3 / mxfp4 weight streams (enable_fused(weights=...)), GPT-XL and GPT-3B, 1 and 8 prompts per forward")
    ap.add_argument("--z", action="store_true", help="16-bit against the lossless 12-bit stream (enable_fused(compress=True)): GPT-B, GPT-XL and GPT-3B at 1 and 4 prompts per forward, "
                                                     "then G1 against G1z per launch at GPT-3B's shapes")
    ap.add_argument("--detok", action="store_true", help="--batch: the tokens -> pixels queue (detokenizer alone, serial, overlapped) instead of the step table")
    ap.add_argument("--cfg-from", default="", help="--fused3b: a --sweep output whose `best` lines give the G1 launch shapes")
    ap.add_argument("--prompts", type=int, default=1, help="--step: prompts per forward (SJDBatchEngine above 1)")
    ap.add_argument("--preset", default="GPT-XL", choices=list(PRESETS))
    ap.add_argument("--only", default="")
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--window", type=int, default=16)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "both"], help="--batch / --step: weight type (both: --batch only, legs alternated)")
    ap.add_argument("--counts", default="1,2,4,8", help="--batch: prompts per forward to measure")
    args = ap.parse_args()
    if args.sweep:
        sweep(args)
    if args.ab:
        ab(args)
    if args.batch and args.detok:
        detok(args)
    elif args.batch:
        batch(args)
    if args.step:
        step(args)
    if args.quant:
        quant(args)
    if args.z:
        zstream(args)
    if args.fused3b:
        fused3b(args)


if __name__ == "__main__":
    main()
