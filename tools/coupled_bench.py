#!/usr/bin/env python3
"""Coupled Jacobi decoding (prefix_token_sampler_scheme="coupled_jacobi": plain Jacobi whose sampling noise is keyed by the token's position, lossless):
accepted tokens per step and ms per step of the three verify schemes, in ONE process, the legs alternating, three rounds, median and spread
(min .. max over the rounds) per leg.

Workload: Lumina-mGPT-7B architecture 768x768 (synthetic weights), 1 prompt, draft window 16, CFG 3.0, bf16, the default weight stream -- bench.py's
model, prompt, grammar and config, ONE backbone and ONE engine for every leg: the legs differ in SJDConfig.prefix_token_sampler_scheme only, which
travels in the blob, so they replay the same captured graphs.  Each leg decodes through a real lead-in so that its timed iterations are centred on
the mean KV length (bench.py's method), with the leg's own tokens per step, measured before any clock starts.

There is no gate.  ms per step is compared with the speculative_jacobi leg of the SAME run; a difference counts only beyond the largest spread
between a leg's rounds, reported beside it.

TOKENS PER STEP COMES FROM ONE SEEDED PATH ON SYNTHETIC WEIGHTS: it is neither a quality nor a speed claim for a real checkpoint -- how many drafts
a fixed-point iteration keeps depends on how strongly a position's distribution depends on the tokens before it, which random weights do not model.

One JSON document on stdout (and in --out)."""
import argparse
import copy
import dataclasses
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")          # as bench.py: read by the HIP runtime when it is loaded
import torch  # noqa: E402

NOTE = ("tokens per step comes from ONE seeded path on SYNTHETIC weights: neither a quality nor a speed claim for a real checkpoint; "
        "all three schemes are lossless (every emitted token is a sample of the model's own distribution)")
LEGS = ["speculative_jacobi", "coupled_jacobi", "jacobi"]


def spread(xs):
    return dict(median=round(statistics.median(xs), 3), min=round(min(xs), 3), max=round(max(xs), 3), rounds=[round(x, 3) for x in xs])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coupled.json"))
    a = ap.parse_args(argv)
    from sjd_amd.engine import SJDEngine
    names = list(LEGS)
    if not torch.cuda.is_available():
        raise SystemExit("coupled_bench.py measures on the GPU: none found")
    import bench
    dev = torch.device("cuda:0")
    b = bench.parse(["--gpus", "1", "--steps", str(a.steps), "--warmup", str(a.warmup)])
    b.model, b.window, b.prompts_per_gpu, b.n_split = "lumina7b", 16, 1, 0
    model, margs, attn = bench.build_model(b, dev)
    w = bench.workload_of(b, margs, 0, dev)
    P, n_img = w["P"], w["n_img"]
    model.setup_cache(batch=2, s_max=((P + n_img + 2 * 16 + 64 + 31) // 32) * 32)
    eng = SJDEngine(model, margs.vocab_size, dev, max_window=16, use_graph=True)
    cfgs = {leg: dataclasses.replace(w["cfg"], prefix_token_sampler_scheme=leg) for leg in names}
    run = lambda leg, **kw: eng.decode(w["prompt"], w["spec"], copy.deepcopy(w["grammar"]), cfgs[leg], **kw)
    pin0 = getattr(attn, "_pin_regime", None)
    for pin in ("keysplit", "colsplit"):             # the graphs of both K1 regimes are captured before any clock starts (bench.py's other_config)
        if hasattr(attn, "_pin_regime"):
            attn._pin_regime = pin
        run(LEGS[0], warmup_iters=0, timed_iters=a.warmup + 8)
    if hasattr(attn, "_pin_regime"):
        attn._pin_regime = pin0
    graphs = len(eng._graphs)
    legs = {}
    for leg in names:                                 # the leg's own tokens per step, over an untimed stretch: where its lead-in has to end
        _, st = run(leg, warmup_iters=a.warmup, timed_iters=a.steps, lead_in_kv=P + n_img // 4)
        tau = st.tokens / max(st.timed_nfe, 1)
        legs[leg] = dict(ms=[], kv=[], tok=[], lead=max(P + 16, int(P + n_img // 2 - tau * (a.steps / 2.0 + a.warmup))))
    torch.cuda.synchronize()
    sync = torch.cuda.synchronize
    for _ in range(a.rounds):
        for leg in names:
            lg = legs[leg]
            _, st = run(leg, warmup_iters=a.warmup, timed_iters=a.steps, on_timed_start=sync, on_timed_end=sync, lead_in_kv=lg["lead"])
            lg["ms"].append(st.seconds / max(st.timed_nfe, 1) * 1e3)
            lg["kv"].append([st.kv_len_start, st.kv_len])
            lg["tok"].append(st.tokens / max(st.timed_nfe, 1))
    rec = dict(device=torch.cuda.get_device_name(0),
               workload="Lumina-mGPT-7B architecture 768x768 (synthetic weights), 1 prompt, draft window 16, CFG 3.0 (32 rows per forward), bf16, 16-bit KV "
                        "cache, default weight stream",
               note=NOTE, steps=a.steps, warmup=a.warmup, rounds=a.rounds,
               order="alternating " + ", ".join(names) + " per round; one process, one device, one backbone, one engine",
               graphs_captured_before_the_legs=graphs, graphs_captured_at_the_end=len(eng._graphs), legs={})
    for leg in names:
        lg = legs[leg]
        rec["legs"][str(leg)] = dict(scheme=leg, ms_per_step=spread(lg["ms"]), tokens_per_step=spread(lg["tok"]), kv_len=lg["kv"], lead_in_kv=lg["lead"])
    one = rec["legs"][LEGS[0]]
    rec["largest_spread_between_rounds_ms"] = round(max(v["ms_per_step"]["max"] - v["ms_per_step"]["min"] for v in rec["legs"].values()), 4)
    for v in rec["legs"].values():
        v["ms_per_step_minus_speculative_jacobi"] = round(v["ms_per_step"]["median"] - one["ms_per_step"]["median"], 4)
        v["tokens_per_step_over_speculative_jacobi"] = round(v["tokens_per_step"]["median"] / one["tokens_per_step"]["median"], 4)
        v["ms_per_token"] = round(v["ms_per_step"]["median"] / v["tokens_per_step"]["median"], 4)
    text = json.dumps(rec, indent=1)
    print(text, flush=True)
    print("NOTE: " + NOTE, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
