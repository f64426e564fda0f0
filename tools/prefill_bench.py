"""The prompt prefill from the quantised weight copies (kernel G1p, enable_fused(..., release_16bit=True)) against today's 16-bit prefill: time and memory.

Lumina-mGPT-7B shapes, synthetic weights (bench.build_model), CFG batch 2, prompts of 32 / 128 / 1024 / 2400 tokens (the last: an image-conditioned prompt).
Legs, each its own backbone with the same weights, all alive in ONE process:
  unreleased     enable_fused(weights="mxfp4"): the prefill runs hipBLASLt on the 16-bit parameters, which stay resident next to the packed copy
  e4m3_released  enable_fused(weights="e4m3", release_16bit=True): the prefill on kernel G1p over the e4m3 copy
  mxfp4_released enable_fused(weights="mxfp4", release_16bit=True): the same over the MXFP4 copy
(A 32-token prompt is 64 rows: a window forward on every leg, not a prefill -- the row is there to say so.)
Protocol: every (leg, length) runs once untimed; then `--rounds` rounds, the legs alternating inside a round, one forward per (leg, length) between two
events; median, min and max over the rounds.  Memory: torch.cuda.memory_allocated after enable_fused (and empty_cache) minus the figure in front of the
backbone's construction -- what the allocator holds for that backbone, the 16-bit layer matrices included or not.

    python tools/prefill_bench.py [--rounds 3] [--out profiles/prefill_quant.json]"""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")          # as bench.py: read by the HIP runtime when it is loaded
import torch  # noqa: E402

import sjd_amd.launch_shapes as LS  # noqa: E402
import sjd_amd.ops as ops  # noqa: E402

LEGS = dict(unreleased=dict(weights="mxfp4"), e4m3_released=dict(weights="e4m3", release_16bit=True), mxfp4_released=dict(weights="mxfp4", release_16bit=True))
LENGTHS = (32, 128, 1024, 2400)


def spread(xs):
    return dict(median=round(statistics.median(xs), 3), min=round(min(xs), 3), max=round(max(xs), 3), rounds=[round(x, 3) for x in xs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefill_quant.json"))
    a = ap.parse_args()
    import bench
    dev = torch.device("cuda:0")
    base = bench.parse(["--gpus", "1", "--steps", "8", "--warmup", "1"])
    base.model, base.window, base.prompts_per_gpu, base.n_split, base.no_fused = "lumina7b", 16, 1, 0, True
    legs = {}
    for tag, kw in LEGS.items():
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(dev)
        model, margs, _ = bench.build_model(copy.copy(base), dev)
        built = torch.cuda.memory_allocated(dev)
        model.enable_fused(ops, gemm="sjd", **kw)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        after = torch.cuda.memory_allocated(dev)
        model.setup_cache(batch=2, s_max=((max(LENGTHS) + 31) // 32) * 32)
        st = model.compress_stats
        legs[tag] = dict(model=model, enable_fused=kw, ms={P: [] for P in LENGTHS},
                         memory=dict(allocated_before_enable_fused_gb=round((built - before) / 1e9, 3), allocated_after_enable_fused_gb=round((after - before) / 1e9, 3),
                                     packed_layer_bytes_gb=round(model.packed_bytes(head=False) / 1e9, 3), bytes_released_gb=round(st.get("bytes_released", 0) / 1e9, 3)))
        print(json.dumps({tag: legs[tag]["memory"]}), flush=True)
    g = torch.Generator().manual_seed(0)
    inputs = {}
    for P in LENGTHS:
        tok = torch.randint(4, 8196, (2, P), generator=g).to(dev)
        pos = torch.stack([torch.arange(P), torch.tensor([1] * (P - 1) + [0])]).to(dev)
        inputs[P] = (tok, pos, torch.tensor([0, P - 1], dtype=torch.int32, device=dev))

    def forward(model, P):
        tok, pos, ks = inputs[P]
        with torch.no_grad():
            return model.forward_window(tok, pos, 0, ks)

    routes = {}
    for tag, leg in legs.items():          # untimed: allocator, hipBLASLt's heuristics, the kernels' code objects
        for P in LENGTHS:
            forward(leg["model"], P)
            no = LS.serves_rows(leg["model"], 2 * P, P)
            routes.setdefault(tag, {})[P] = "window" if no is None else ("G1p" if leg["model"].released_16bit else "hipBLASLt on the 16-bit parameters")
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for P in LENGTHS:
            for tag, leg in legs.items():          # the legs alternate
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                forward(leg["model"], P)
                e1.record()
                torch.cuda.synchronize()
                leg["ms"][P].append(e0.elapsed_time(e1))
    doc = dict(tool="tools/prefill_bench.py", device=torch.cuda.get_device_name(dev), model="Lumina-mGPT-7B shapes, synthetic weights, bf16, CFG batch 2",
               protocol=f"one process, three backbones alive, one untimed forward per (leg, length), then {a.rounds} rounds with the legs alternating; ms per "
                        "prefill forward (32 layers + head): median, min, max over the rounds",
               g1p_launch_shape=f"{LS.PREFILL_ROW_BLOCK} rows x 4 column tiles per workgroup, stages of eight k-steps: UNTUNED, no sweep was run",
               legs={tag: dict(enable_fused=leg["enable_fused"], memory=leg["memory"], route={str(P): routes[tag][P] for P in LENGTHS},
                               ms_per_prefill={str(P): spread(leg["ms"][P]) for P in LENGTHS}) for tag, leg in legs.items()})
    for P in LENGTHS:
        u = doc["legs"]["unreleased"]["ms_per_prefill"][str(P)]["median"]
        doc.setdefault("released_over_unreleased", {})[str(P)] = {tag: round(doc["legs"][tag]["ms_per_prefill"][str(P)]["median"] / u, 3)
                                                                  for tag in ("e4m3_released", "mxfp4_released")}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc["released_over_unreleased"]), flush=True)


if __name__ == "__main__":
    main()
