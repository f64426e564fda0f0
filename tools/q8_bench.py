#!/usr/bin/env python3
"""The 8-bit (e4m3) weight stream against the uncompressed and the lossless 12-bit one, in ONE process, the legs alternating, three rounds,
median and spread (min .. max over the rounds) per leg.

  --launch  per launch: the four Lumina-7B projection shapes at 32 rows and the Emu3-8B ones at 64, each leg at the launch shape the backbone
            uses for it (G1_CFG / G1_CFG_Z / G1_CFG_Q8 and the _EMU3 sets), launches replayed from a hipGraph over `--copies` weight sets so that
            every launch streams from HBM; gate|up as the backbone runs it (the fused launch where it is served, else the projection + F3).
            Bytes: algorithmic (the bf16 matrix) and stored (what the leg's format holds), and stored bytes / time as a fraction of 8 TB/s.
  --step    per step: Lumina-mGPT-7B 768x768, draft window 16, CFG, bf16 -- the default 12-bit packing (enable_fused as bench.py calls it) against
            enable_fused(weights="e4m3"), two backbones with the same synthetic weights, each decoded through a real lead-in so that the timed
            iterations are centred on the mean KV length (bench.py's method), ms per SJD iteration.

  --batch   several prompts per forward (SJDBatchEngine): the same workload with 2 / 4 / 8 prompts sharing the window forward (64 / 128 / 256 rows) --
            enable_fused(weights="e4m3", max_rows=64 / 128 / 256) against what those row counts run otherwise: the default 12-bit stream at 2 / 4
            prompts (G1_CFG_64ROW / G1_CFG_128ROW), compress=False at 8 (G1_CFG_256ROW) -- and at 4 as well, which is what bench.py runs there.  Per
            prompt count one backbone per leg with the same synthetic
            weights, the timed iterations centred on the mean KV length by a warm-up of whole window iterations; ms per shared window forward, packed
            bytes per step, and us per launch of the four projections as each backbone runs them (its own 32 packed layers in turn, from a hipGraph).

  --mxfp4   adds an MXFP4 leg ("q4": enable_fused(weights="mxfp4"), kernels G1q4 / G1sq4, launch shapes G1_CFG_Q4 / G1_CFG_EMU3_Q4) to --launch and --step:
            the legs then alternate 12-bit / e4m3 / mxfp4 (per launch: bf16 first), and the record compares the mxfp4 leg with the e4m3 leg of the same run.
  --e2m3    adds a 6-bit e2m3 leg ("q6": enable_fused(weights="e2m3"), kernels G1q6 / G1sq6, the MXFP4 launch shapes -- untuned for this stream) to --launch and
            --step, between the e4m3 and the mxfp4 leg: 12-bit / e4m3 / e2m3 / mxfp4; the record compares the e2m3 leg with the e4m3 leg of the same run.

One JSON document on stdout (and in --out)."""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")          # as bench.py: read by the HIP runtime when it is loaded
import torch  # noqa: E402

import sjd_amd._lib as L  # noqa: E402
import sjd_amd.backbones as BB  # noqa: E402
import sjd_amd.ops as ops  # noqa: E402
from g1_bench import timed_graph  # noqa: E402

PEAK = 8.0e12


def spread(xs):
    return dict(median=round(statistics.median(xs), 3), min=round(min(xs), 3), max=round(max(xs), 3), rounds=[round(x, 3) for x in xs])


def launch_legs(a, dev, lib):
    C = BB.ChameleonBackbone
    arch = [("lumina7b", 32, dict(qkv=(12288, 4096), o=(4096, 4096), gate_up=(22016, 4096), down=(4096, 11008)), (C.G1_CFG, C.G1_CFG_Z, C.G1_CFG_Q8, C.G1_CFG_Q4)),
            ("emu3_8b", 64, dict(qkv=(6144, 4096), o=(4096, 4096), gate_up=(28672, 4096), down=(4096, 14336)), (C.G1_CFG_EMU3, C.G1_CFG_EMU3_Z, C.G1_CFG_EMU3_Q8, C.G1_CFG_EMU3_Q4))]
    tags = ("bf16", "z12", "q8") + (("q6",) if a.e2m3 else ()) + (("q4",) if a.mxfp4 else ())
    out = []
    for model, rows, shapes, cfgs in arch:
        for name, (N, K) in shapes.items():
            if a.only and name not in a.only.split(","):
                continue
            x = torch.randn(rows, K, device=dev).to(torch.bfloat16)
            ws = [(torch.randn(N, K, device=dev) / K ** 0.5).to(torch.bfloat16) for _ in range(a.copies)]
            legs = {}
            for tag in tags:
                KC, waves, sm = cfgs[dict(bf16=0, z12=1, q8=2, q6=3, q4=3)[tag]][name]          # (the 6-bit stream runs on the MXFP4 sets)
                gu = name == "gate_up" and 2 * KC == K
                if tag == "bf16":
                    pk = [ops.pack_weight(w, KC, sm) for w in ws]
                    stored = N * K * 2
                elif tag == "z12":
                    pk = [ops.pack_weight_z(w, KC, sm, gateup=gu) for w in ws]
                    stored = pk[0].nbytes()
                elif tag == "q8":
                    pk = [ops.pack_weight_q8(w, KC, sm, gateup=gu) for w in ws]
                    stored = pk[0].nbytes()
                else:
                    pk = [(ops.pack_weight_q6 if tag == "q6" else ops.pack_weight_q4)(w, KC, sm, gateup=gu) for w in ws]
                    stored = pk[0].nbytes()
                fused = gu and ops.gateup_silu_ok(rows, N // 2, K, KC, tag == "z12", tag in ("q8", "q6", "q4"))
                if fused:
                    run = lambda i, pk=pk, sm=sm: ops.gateup_silu(x, pk[i % a.copies], N // 2, K, sm)
                elif name == "gate_up":
                    run = lambda i, pk=pk, KC=KC, waves=waves, sm=sm: ops.silu_mul(ops.skinny_gemm(x, pk[i % a.copies], N, K, KC, waves, sm), rows=rows, dtype=x.dtype)
                else:
                    run = lambda i, pk=pk, KC=KC, waves=waves, sm=sm: ops.skinny_gemm(x, pk[i % a.copies], N, K, KC, waves, sm)
                legs[tag] = dict(run=run, stored=stored, cfg=[KC, waves, int(sm)], launch="fused gate|up + SiLU" if fused else ("projection + F3" if name == "gate_up" else "projection"),
                                 us=[], keep=pk)
            del ws
            for _ in range(a.rounds):                     # alternating: bf16, 12-bit, 8-bit, and round again
                for tag in tags:
                    legs[tag]["us"].append(timed_graph(legs[tag]["run"], a.launches, lib)[1] * 1e3)
            rec = dict(model=model, rows=rows, shape=name, N=N, K=K, algorithmic_bytes=N * K * 2)
            for tag, lg in legs.items():
                s = spread(lg["us"])
                rec[tag] = dict(cfg=lg["cfg"], launch=lg["launch"], us=s, stored_bytes=lg["stored"],
                                frac_of_8TBps_on_stored_bytes=round(lg["stored"] / (s["median"] * 1e-6) / PEAK, 4),
                                frac_of_8TBps_on_algorithmic_bytes=round(N * K * 2 / (s["median"] * 1e-6) / PEAK, 4))
            rec["q8_over_z12"] = round(rec["q8"]["us"]["median"] / rec["z12"]["us"]["median"], 4)
            rec["q8_over_bf16"] = round(rec["q8"]["us"]["median"] / rec["bf16"]["us"]["median"], 4)
            if a.mxfp4:
                rec["q4_over_q8"] = round(rec["q4"]["us"]["median"] / rec["q8"]["us"]["median"], 4)
            if a.e2m3:
                rec["q6_over_q8"] = round(rec["q6"]["us"]["median"] / rec["q8"]["us"]["median"], 4)
            print(json.dumps(rec), flush=True)
            out.append(rec)
            del legs
            torch.cuda.empty_cache()
    return out


def step_legs(a, dev):
    import bench
    from sjd_amd.engine import SJDEngine
    base = bench.parse(["--gpus", "1", "--steps", str(a.steps), "--warmup", str(a.warmup)])
    base.model, base.window, base.prompts_per_gpu, base.n_split = "lumina7b", 16, 1, 0
    legs = {}
    tags = ("z12", "q8") + (("q6",) if a.e2m3 else ()) + (("q4",) if a.mxfp4 else ())
    for tag in tags:
        b = copy.copy(base)
        b.no_fused = tag != "z12"                         # (the q8 / q4 legs call enable_fused themselves, on the same synthetic weights)
        model, margs, attn = bench.build_model(b, dev)
        if tag != "z12":
            model.enable_fused(ops, gemm="sjd", weights=dict(q8="e4m3", q6="e2m3", q4="mxfp4")[tag])
        w = bench.workload_of(b, margs, 0, dev)
        P, n_img = w["P"], w["n_img"]
        model.setup_cache(batch=2, s_max=((P + n_img + 2 * 16 + 64 + 31) // 32) * 32)
        eng = SJDEngine(model, margs.vocab_size, dev, max_window=16, use_graph=True)
        pin0 = getattr(attn, "_pin_regime", None)
        for pin in ("keysplit", "colsplit"):             # the graphs of both K1 regimes are captured before any clock starts (bench.py's other_config)
            if hasattr(attn, "_pin_regime"):
                attn._pin_regime = pin
            eng.decode(w["prompt"], w["spec"], copy.deepcopy(w["grammar"]), w["cfg"], warmup_iters=0, timed_iters=a.warmup + 8)
        if hasattr(attn, "_pin_regime"):
            attn._pin_regime = pin0
        torch.cuda.synchronize()
        legs[tag] = dict(model=model, eng=eng, w=w, ms=[], kv=[], tok=[],
                         lead=int(P + n_img // 2 - w["tau_est"] * (a.steps / 2.0 + a.warmup)))
    sync = torch.cuda.synchronize
    for _ in range(a.rounds):
        for tag in tags:
            lg = legs[tag]
            w = lg["w"]
            _, st = lg["eng"].decode(w["prompt"], w["spec"], copy.deepcopy(w["grammar"]), w["cfg"], warmup_iters=a.warmup, timed_iters=a.steps,
                                     on_timed_start=sync, on_timed_end=sync, lead_in_kv=lg["lead"])
            lg["ms"].append(st.seconds / max(st.timed_nfe, 1) * 1e3)
            lg["kv"].append([st.kv_len_start, st.kv_len])
            lg["tok"].append(round(st.tokens / max(st.timed_nfe, 1), 3))
    rec = dict(workload="Lumina-mGPT-7B architecture 768x768 (synthetic weights), 1 prompt, draft window 16, CFG 3.0 (32 rows per forward), bf16, 16-bit KV cache",
               steps=a.steps, warmup=a.warmup, rounds=a.rounds, order="alternating " + ", ".join(tags) + " per round; one process, one device")
    for tag, lg in legs.items():
        m = lg["model"]
        rec[tag] = dict(weights=m.weights, G1_CFG={k: list(v) for k, v in m.G1_CFG.items()}, ms_per_step=spread(lg["ms"]), kv_len=lg["kv"], tokens_per_step=lg["tok"],
                        layer_bytes_per_step=m.packed_bytes(head=False), compress_stats={k: v for k, v in m.compress_stats.items() if not isinstance(v, dict)})
    z, q = rec["z12"]["ms_per_step"], rec["q8"]["ms_per_step"]
    rec["q8_minus_z12_ms"] = round(q["median"] - z["median"], 4)
    rec["largest_spread_between_rounds_ms"] = round(max(z["max"] - z["min"], q["max"] - q["min"]), 4)
    rec["gain_exceeds_spread"] = bool(z["median"] - q["median"] > rec["largest_spread_between_rounds_ms"])
    if a.mxfp4:          # the 4-bit leg against the 8-bit leg of the SAME run: faster only if the difference exceeds the spread between this run's rounds
        q4 = rec["q4"]["ms_per_step"]
        rec["q4_minus_q8_ms"] = round(q4["median"] - q["median"], 4)
        rec["largest_spread_between_rounds_ms"] = round(max(rec["largest_spread_between_rounds_ms"], q4["max"] - q4["min"]), 4)
        rec["q4_faster_than_q8_beyond_spread"] = bool(q["median"] - q4["median"] > rec["largest_spread_between_rounds_ms"])
    if a.e2m3:           # the 6-bit leg against the 8-bit leg of the SAME run, by the same rule
        q6 = rec["q6"]["ms_per_step"]
        rec["q6_minus_q8_ms"] = round(q6["median"] - q["median"], 4)
        rec["largest_spread_between_rounds_ms"] = round(max(rec["largest_spread_between_rounds_ms"], q6["max"] - q6["min"]), 4)
        rec["q6_faster_than_q8_beyond_spread"] = bool(q["median"] - q6["median"] > rec["largest_spread_between_rounds_ms"])
        if a.mxfp4:
            rec["q4_faster_than_q8_beyond_spread"] = bool(q["median"] - rec["q4"]["ms_per_step"]["median"] > rec["largest_spread_between_rounds_ms"])
    for tag in tags:     # stored layer bytes per step against the HBM peak
        rec[tag]["frac_of_8TBps_on_layer_bytes"] = round(rec[tag]["layer_bytes_per_step"] / (rec[tag]["ms_per_step"]["median"] * 1e-3) / PEAK, 4)
    print(json.dumps(rec), flush=True)
    return rec


def batch_launches(a, model, rows, dev, lib):
    """us per launch of the four projections of `model` at `rows` window rows, as its window forward runs them"""
    m = model.args
    H, Hkv, D, hid, inter = model.n_heads, model.n_kv_heads, model.head_dim, m.hidden_size, m.intermediate_size
    out = {}
    for name, (N, K) in dict(qkv=((H + 2 * Hkv) * D, hid), o=(hid, H * D), gate_up=(2 * inter, hid), down=(hid, inter)).items():
        KC0, waves, sm = model.G1_CFG[name]
        KC = model._q8_chunk(name, rows, K)
        pk = [d[name] for d in model._packed]
        x = torch.randn(rows, K, device=dev).to(torch.bfloat16)
        fused = name == "gate_up" and rows <= 64 and ops.gateup_silu_ok(rows, inter, hid, KC0, isinstance(pk[0], ops.PackedZ), model.weights is not None)
        if fused:
            run = lambda i: ops.gateup_silu(x, pk[i % len(pk)], inter, hid, sm)
        elif name == "gate_up":
            run = lambda i: ops.silu_mul(ops.skinny_gemm(x, pk[i % len(pk)], N, K, KC, waves, sm), rows=rows, dtype=x.dtype)
        else:
            run = lambda i: ops.skinny_gemm(x, pk[i % len(pk)], N, K, KC, waves, sm)
        us = [timed_graph(run, a.launches, lib)[1] * 1e3 for _ in range(a.rounds)]
        size = pk[0].nbytes() if isinstance(pk[0], (ops.PackedZ, ops.PackedQ8)) else pk[0].numel() * pk[0].element_size()
        out[name] = dict(cfg=[KC, waves, int(sm)], launch="fused gate|up + SiLU" if fused else ("projection + F3" if name == "gate_up" else "projection"),
                         us=spread(us), stored_bytes=size, frac_of_8TBps_on_stored_bytes=round(size / (statistics.median(us) * 1e-6) / PEAK, 4))
    return out


def batch_legs(a, dev, lib):
    import bench
    from sjd_amd.engine_batch import SJDBatchEngine
    from sjd_amd.frontends import lumina_prompt, lumina_window_spec
    out = []
    for PP in [int(v) for v in a.prompts.split(",")]:
        rows = 2 * PP * 16
        base = bench.parse(["--gpus", "1", "--steps", str(a.steps), "--warmup", str(a.warmup)])
        base.model, base.window, base.prompts_per_gpu, base.n_split = "lumina7b", 16, PP, 0
        legs = {}
        tags = (("z12",) if rows <= 64 else ("z12", "bf16") if rows <= 128 else ("bf16",)) + ("q8",)      # (four prompts: bench.py itself runs compress=False)
        for tag in tags:
            b = copy.copy(base)
            b.no_fused = True                             # (each leg calls enable_fused itself, on the same synthetic weights)
            if tag == "q8":
                b.prompts_per_gpu = 1                     # (no G1_CFG of the caller's: enable_fused takes its 8-bit set)
            model, margs, attn = bench.build_model(b, dev)
            if tag == "q8":
                model.enable_fused(ops, gemm="sjd", weights="e4m3", max_rows=64 if rows <= 64 else 128 if rows <= 128 else 256)
            else:
                model.enable_fused(ops, gemm="sjd", compress=False if tag == "bf16" else None)
            w = bench.workload_of(base, margs, 0, dev)
            P, n_img = w["P"], w["n_img"]
            model.setup_cache(batch=2 * PP, s_max=((P + n_img + 2 * 16 + 64 + 31) // 32) * 32)
            eng = SJDBatchEngine(model, margs.vocab_size, dev, PP, max_window=16, use_graph=True)
            prompts = [lumina_prompt(P, w["grid"], w["grid"], seed=1234 + i) for i in range(PP)]
            legs[tag] = dict(model=model, eng=eng, w=w, prompts=prompts, specs=[lumina_window_spec(p_, dev) for p_ in prompts], ms=[], tok=[], kv=[],
                             warm=max(a.warmup, int(n_img / 2 / w["tau_est"] - a.steps / 2)))
        sync = torch.cuda.synchronize
        for rnd in range(a.rounds + 1):                   # round 0 is untimed practice: every hipGraph of the decode is captured in it
            for tag in tags:
                lg = legs[tag]
                w = lg["w"]
                res = lg["eng"].decode_many(lg["prompts"], lg["specs"], [copy.deepcopy(w["grammar"]) for _ in range(PP)], w["cfg"], warmup_iters=lg["warm"],
                                            timed_iters=a.steps, on_timed_start=sync, on_timed_end=sync)
                rs = lg["eng"].run_stats
                if rnd:
                    lg["ms"].append(rs["seconds"] / max(rs["timed_iterations"], 1) * 1e3)
                    lg["tok"].append(round(rs["tokens"] / max(rs["timed_iterations"], 1), 3))
                    lg["kv"].append([len(seq) for seq, _ in res])
        rec = dict(prompts_per_forward=PP, rows=rows, steps=a.steps, warmup_iterations=legs["q8"]["warm"], rounds=a.rounds,
                   order="alternating " + ", ".join(tags) + " per round after one untimed round; one process, one device",
                   today="z12" if rows <= 128 else "bf16")
        for tag, lg in legs.items():
            m = lg["model"]
            rec[tag] = dict(weights=m.weights, compress=bool(m.compress), max_rows=getattr(m, "max_rows", None), G1_CFG={k: list(v) for k, v in m.G1_CFG.items()},
                            ms_per_step=spread(lg["ms"]), tokens_per_step=lg["tok"], sequence_len_at_end=lg["kv"], layer_bytes_per_step=m.packed_bytes(head=False),
                            bytes_per_step_with_head=m.packed_bytes(), per_launch=batch_launches(a, m, rows, dev, lib))
        q = rec["q8"]["ms_per_step"]
        rec["largest_spread_between_rounds_ms"] = round(max(rec[tag]["ms_per_step"]["max"] - rec[tag]["ms_per_step"]["min"] for tag in tags), 4)
        for tag in tags[:-1]:
            rec[f"q8_minus_{tag}_ms"] = round(q["median"] - rec[tag]["ms_per_step"]["median"], 4)
            rec[f"q8_minus_{tag}_exceeds_spread"] = bool(abs(rec[f"q8_minus_{tag}_ms"]) > rec["largest_spread_between_rounds_ms"])
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del legs, model, eng
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launch", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--batch", action="store_true")
    ap.add_argument("--mxfp4", action="store_true", help="--launch / --step: add the MXFP4 leg (q4)")
    ap.add_argument("--e2m3", action="store_true", help="--launch / --step: add the 6-bit e2m3 leg (q6)")
    ap.add_argument("--prompts", default="2,4,8", help="--batch: prompts per forward, comma separated")
    ap.add_argument("--launches", type=int, default=48)
    ap.add_argument("--copies", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = L.load()
    doc = dict(device=torch.cuda.get_device_name(0), peak_TBps=8.0)
    if a.launch:
        doc["per_launch"] = launch_legs(a, dev, lib)
        doc["per_launch_method"] = (f"{a.launches} launches per hipGraph over {a.copies} weight sets, the graph replayed three times and the middle time taken; "
                                    f"{a.rounds} rounds alternating bf16 / 12-bit / 8-bit{' / e2m3' if a.e2m3 else ''}{' / mxfp4' if a.mxfp4 else ''}; us per launch: median, min, max over the rounds")
    if a.step:
        doc["per_step"] = step_legs(a, dev)
    if a.batch:
        doc["per_batch_step"] = batch_legs(a, dev, lib)
        doc["per_batch_step_workload"] = ("Lumina-mGPT-7B architecture 768x768 (synthetic weights), 2 / 4 / 8 prompts sharing one window forward, draft window 16, "
                                          "CFG 3.0, bf16, 16-bit KV cache")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
