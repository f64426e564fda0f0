#!/usr/bin/env python3
"""Lenient verification (SJDConfig.lenience, LOSSY and off by default): accepted tokens per step and ms per step against the factor, in ONE process,
the legs alternating, three rounds, median and spread (min .. max over the rounds) per leg.

Workload: Lumina-mGPT-7B architecture 768x768 (synthetic weights), 1 prompt, draft window 16, CFG 3.0, bf16, the default weight stream -- bench.py's
model, prompt, grammar and config, ONE backbone and ONE engine for every leg: the legs differ in SJDConfig.lenience only, which travels in the blob,
so they replay the same captured graphs.  Each leg decodes through a real lead-in so that its timed iterations are centred on the mean KV length
(bench.py's method), with the leg's own tokens per step, measured before any clock starts.

ms per step at lambda > 1 is compared with the lambda = 1 leg of the SAME run and reported beside the largest spread between rounds; no gate is set on
it (K4 gains one fp32 division per element it already reads).

TOKENS PER STEP ON SYNTHETIC WEIGHTS IS NOT A QUALITY STATEMENT and no promise for a real checkpoint: a relaxed verify step emits drafts the exact
rule would have rejected, and what that does to an image was NOT measured -- no real checkpoint is available to this project.

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

NOTE = ("tokens per step on SYNTHETIC weights: not a quality statement and not a promise for a real checkpoint; "
        "image quality under lenience > 1 was NOT measured")


def spread(xs):
    return dict(median=round(statistics.median(xs), 3), min=round(min(xs), 3), max=round(max(xs), 3), rounds=[round(x, 3) for x in xs])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lenience", type=float, nargs="+", default=[1.0, 1.25, 1.5, 2.0, 4.0], help="the legs; 1.0 (the exact rule) must be among them")
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lenience.json"))
    a = ap.parse_args(argv)
    from sjd_amd.engine import SJDEngine, lenience_field
    lams = [float(x) for x in a.lenience]
    if 1.0 not in lams:
        ap.error("--lenience needs the 1.0 leg: the others are compared with it")
    for lam in lams:
        lenience_field(lam)
    if not torch.cuda.is_available():
        raise SystemExit("lenience_bench.py measures on the GPU: none found")
    import bench
    dev = torch.device("cuda:0")
    b = bench.parse(["--gpus", "1", "--steps", str(a.steps), "--warmup", str(a.warmup)])
    b.model, b.window, b.prompts_per_gpu, b.n_split = "lumina7b", 16, 1, 0
    model, margs, attn = bench.build_model(b, dev)
    w = bench.workload_of(b, margs, 0, dev)
    P, n_img = w["P"], w["n_img"]
    model.setup_cache(batch=2, s_max=((P + n_img + 2 * 16 + 64 + 31) // 32) * 32)
    eng = SJDEngine(model, margs.vocab_size, dev, max_window=16, use_graph=True)
    cfgs = {lam: dataclasses.replace(w["cfg"], lenience=lam) for lam in lams}
    run = lambda lam, **kw: eng.decode(w["prompt"], w["spec"], copy.deepcopy(w["grammar"]), cfgs[lam], **kw)
    pin0 = getattr(attn, "_pin_regime", None)
    for pin in ("keysplit", "colsplit"):             # the graphs of both K1 regimes are captured before any clock starts (bench.py's other_config)
        if hasattr(attn, "_pin_regime"):
            attn._pin_regime = pin
        run(1.0, warmup_iters=0, timed_iters=a.warmup + 8)
    if hasattr(attn, "_pin_regime"):
        attn._pin_regime = pin0
    graphs = len(eng._graphs)
    legs = {}
    for lam in lams:                                 # the leg's own tokens per step, over an untimed stretch: where its lead-in has to end
        _, st = run(lam, warmup_iters=a.warmup, timed_iters=a.steps, lead_in_kv=P + n_img // 4)
        tau = st.tokens / max(st.timed_nfe, 1)
        legs[lam] = dict(ms=[], kv=[], tok=[], lead=max(P + 16, int(P + n_img // 2 - tau * (a.steps / 2.0 + a.warmup))))
    torch.cuda.synchronize()
    sync = torch.cuda.synchronize
    for _ in range(a.rounds):
        for lam in lams:
            lg = legs[lam]
            _, st = run(lam, warmup_iters=a.warmup, timed_iters=a.steps, on_timed_start=sync, on_timed_end=sync, lead_in_kv=lg["lead"])
            lg["ms"].append(st.seconds / max(st.timed_nfe, 1) * 1e3)
            lg["kv"].append([st.kv_len_start, st.kv_len])
            lg["tok"].append(st.tokens / max(st.timed_nfe, 1))
    rec = dict(device=torch.cuda.get_device_name(0),
               workload="Lumina-mGPT-7B architecture 768x768 (synthetic weights), 1 prompt, draft window 16, CFG 3.0 (32 rows per forward), bf16, 16-bit KV "
                        "cache, default weight stream",
               note=NOTE, steps=a.steps, warmup=a.warmup, rounds=a.rounds,
               order="alternating lenience " + ", ".join(str(x) for x in lams) + " per round; one process, one device, one backbone, one engine",
               graphs_captured_before_the_legs=graphs, graphs_captured_at_the_end=len(eng._graphs), legs={})
    for lam in lams:
        lg = legs[lam]
        rec["legs"][str(lam)] = dict(lenience=lam, ms_per_step=spread(lg["ms"]), tokens_per_step=spread(lg["tok"]), kv_len=lg["kv"], lead_in_kv=lg["lead"])
    one = rec["legs"]["1.0"]
    rec["largest_spread_between_rounds_ms"] = round(max(v["ms_per_step"]["max"] - v["ms_per_step"]["min"] for v in rec["legs"].values()), 4)
    for v in rec["legs"].values():
        v["ms_per_step_minus_lenience_1"] = round(v["ms_per_step"]["median"] - one["ms_per_step"]["median"], 4)
        v["tokens_per_step_over_lenience_1"] = round(v["tokens_per_step"]["median"] / one["tokens_per_step"]["median"], 4)
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
