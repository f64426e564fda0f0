#!/usr/bin/env python3
"""G1s (gate|up projection with SiLU * up as its epilogue) alone: hipGraph replays over several packed weight copies (every launch streams
from HBM), HIP-event time per launch; the driver for the PMC passes behind profiles/g1s_traffic.json.
  python tools/g1s_bench.py [--launches 48] [--copies 6] [--unfused]      (--unfused: G1 + F3 on the same weights, for comparison)
Each gate|up kernel alone (the A/B of profiles/gateup_epilogue_ab.json; SJD_HIP_LIB / SJD_HIP_EXP_LIB pick the build):
  --form plain|z|q8|q4   the weight stream: 16-bit (g1_gateup_silu), 12-bit (g1z_), e4m3 (g1q_), MXFP4 (g1q4_)
  --rows 32|64           64: the tall kernels (plain and z)
  --dtype bf16|fp16      (fp16: plain only)
  --hidden K             8192 with --form q4: g1q4_gateup_silu_k4 (the copy packed in four chunks of 2048)
  --inter I              11008; 14336 is Emu3's"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import sjd_amd.ops as ops

KERNEL = {"plain": "g1_gateup_silu", "z": "g1z_gateup_silu", "q8": "g1q_gateup_silu", "q4": "g1q4_gateup_silu"}          # (q4: g1qb_gateup_silu<G1Q4Stream>, under the label profiles/ knows it by)
BITS = {"plain": 16, "z": 12, "q8": 8, "q4": 4.25}          # stored bits per weight (z: without the unit headers)


def measure(form="plain", rows=32, dtype="bf16", hidden=4096, inter=11008, launches=48, copies=6, unfused=False):
    dev = torch.device("cuda:0")
    dt = {"bf16": torch.bfloat16, "fp16": torch.float16}[dtype]
    K, k4 = hidden, form == "q4" and hidden == 8192
    KC = 2048 if k4 else K // 2
    x = torch.randn(rows, K, device=dev).to(dt)
    pack = {"plain": lambda w: ops.pack_weight(w, KC, True), "z": lambda w: ops.pack_weight_z(w, KC, True, gateup=True),
            "q8": lambda w: ops.pack_weight_q8(w, KC, True, gateup=True), "q4": lambda w: ops.pack_weight_q4(w, KC, True, gateup=not k4)}[form]
    wps = [pack((torch.randn(2 * inter, K, device=dev) / K ** 0.5).to(dt)) for _ in range(copies)]
    # the folded norm's row statistics: F1r's; past its eight slices (hidden 8192) four slices of any positive numbers
    rn = (ops.residual_sumsq(x.clone(), None) if K <= 4096 else torch.rand(4, (rows + 31) // 32 * 32, device=dev) * 3000 + 50, K, 1e-5)

    def one(i):
        if unfused:
            return ops.silu_mul(ops.skinny_gemm(x, wps[i % copies], 2 * inter, K, KC, waves=8, step_major=True), rows=rows, dtype=x.dtype, row_norm=rn)
        return ops.gateup_silu(x, wps[i % copies], inter, K, True, row_norm=rn)

    with torch.cuda.stream(torch.cuda.Stream()):
        one(0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(launches):
            one(i)
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(4):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / (4 * launches)
    alg = int(2 * inter * K * BITS[form] / 8) + rows * K * 2 + rows * inter * 2
    name = KERNEL[form] + ("_k4" if k4 else "_tall" if rows > 32 else "")
    return dict(kernel=("g1_skinny_gemm + f3_silu_mul (%s)" % form) if unfused else name, rows=rows, dtype=dtype, hidden=K, inter=inter,
                us_per_launch=round(us, 2), algorithmic_bytes=alg, TBps=round(alg / us / 1e6, 3))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=48)
    ap.add_argument("--copies", type=int, default=6)
    ap.add_argument("--unfused", action="store_true")
    ap.add_argument("--form", choices=sorted(KERNEL), default="plain")
    ap.add_argument("--rows", type=int, choices=[32, 64], default=32)
    ap.add_argument("--dtype", choices=["bf16", "fp16"], default="bf16")
    ap.add_argument("--hidden", type=int, default=4096)
    ap.add_argument("--inter", type=int, default=11008)
    print(json.dumps(measure(**vars(ap.parse_args()))))
