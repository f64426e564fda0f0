"""The opt-in experiments of ChameleonBackbone's folded window forward.  All are correct, tested, measured no faster than the product's launches and OFF
by default; all call entry points that exist only in libsjd_hip_exp.so.  backbones.py imports this module only when a switch is set (backbones._experiments_on:
the environment variable, or the instance attribute of the same name), so a default decode never reaches _lib.load_exp() -- engine.check_reduce_timeouts relies on it.

  k1_fused (SJD_K1_FUSED=1)           K1F: F2 + K1 + combine in one launch, 64 workgroups.  A CU streams ~30 GB/s at most, so 64 workgroups cap at ~1.9 TB/s where
                                      the 256-workgroup split kernel reaches 2.8 TB/s, and the dependent round trips (partials -> q/K/V -> tiles -> merge) remain inside
                                      the fused kernel (profiles/r2_attention_block.jsonl: 17.3 / 23.2 / 32.5 / 47.6 us against 17.7 / 21.6 / 27.0 / 33.7 us at kv_len
                                      64 / 448 / 1216 / 2368).  k1_fused_split (SJD_K1_FUSED_SPLIT, default on): the split form K1Fs, else one workgroup per (batch, head).
  reduce_fused (SJD_REDUCE_FUSED=1)   the o / down projections of a <= 32-row window reduce their own split-K planes, add the residual and write the row statistics in
                                      their tail (sjd_skinny_gemm_reduce: device-coherent exchange between the workgroups of a 512-column slice, bit-identical h and
                                      statistics), so that stage F1r -- two graph nodes per layer -- disappears.  By kernel time o 13.55 -> 12.79 us, down 23.13 -> 22.05 us,
                                      but 3.512 against 3.416 ms/step end to end: three dependent device-scope round trips (store acknowledgement, ticket, plane loads) cost
                                      more than a graph-node boundary plus ONE round trip.
  mlp_pair (SJD_MLP_PAIR=1)           sjd_mlp_pair_z: gate|up + SiLU * up AND the down projection in one launch.  Needs the fused gate|up and no reducing down.
  PREFETCH (SJD_PREFETCH="o:128:after,gate_up:0,...")   the packed weights of projection j+1 are read into the Infinity Cache on a side stream (a parallel branch of the
                                      forward hipGraph) "g1": from the moment G1(j) is launched, "after": from the moment G1(j) has finished, i.e. under the latency-bound
                                      kernels that follow it ("Idle HBM").  Prefetch on disables the fused gate|up and the reducing tail.
  gateup_fused = "tall" (SJD_GATEUP_FUSED=tall)   kernel G1s also at 65..128 rows, where G1 + F3 measured faster (profiles/r3_g1_tiled8.txt)."""
import os as _os

import torch

from . import backbones as BB
from .backbones import _chk

_K1_FUSED_SPLIT_DEFAULT = _os.environ.get("SJD_K1_FUSED_SPLIT", "1") != "0"
_PF_NEXT = dict(qkv=("o", 0), o=("gate_up", 0), gate_up=("down", 0), down=("qkv", 1))


def attention_block(m, qkv_part, li, qn, pos, B, n, params, kv_len, key_start, row_norm=None, tag=None):
    """QK-norm + RoPE + KV append + draft-window attention of one layer on the G1 partials of the q|k|v projection: kernel K1F (one launch) for the
    multi-head 16-row window, F2 then K1 (+ combine) otherwise."""
    ops, H, Hkv, D = m._ops, m.n_heads, m.n_kv_heads, m.head_dim
    ks_ok = isinstance(key_start, torch.Tensor) and key_start.is_cuda and key_start.dtype == torch.int32
    if getattr(m, "k1_fused", BB._K1_FUSED_DEFAULT) and ks_ok and not m.args.swin_norm and m.args.model_parallel_size == 1 and ops.fused_attention_ok(B, n, H, Hkv, D, m.cache.k.dtype):
        ns, ws = 1, None
        if getattr(m, "k1_fused_split", _K1_FUSED_SPLIT_DEFAULT):       # K1Fs: the split form (F2 + k1_partial in one launch, then k1_combine)
            ns = m.attn._resolve_split(B, Hkv, n, H)
            ws = m.attn._workspace(B, H, n, D, m.cache.k.device) if ns > 1 else None
        return ops.qkv_attention_fused(qkv_part, m.cache.k[li], m.cache.v[li], *qn, m._inv_freq32, pos, B, n, H, D, params,
                                       kv_len if params is None else 0, key_start, row_norm=row_norm, dtype=m.lm_head.weight.dtype, n_split=ns, workspace=ws)
    q = m._f2(qkv_part, li, qn, pos, B, n, params, kv_len, row_norm=row_norm)
    return m.attn.attend(li, q, m.cache, kv_len, key_start)


def _prefetch_plan(m):
    """the plan (m.PREFETCH, then SJD_PREFETCH) and its side stream, resolved at the backbone's first forward with a switch set"""
    if getattr(m, "_pf_plan", None) is None:
        plan = dict(m.PREFETCH)
        for item in filter(None, _os.environ.get("SJD_PREFETCH", "").split(",")):
            f = item.split(":")
            plan[f[0]] = (int(f[1]), f[2] if len(f) > 2 else "after")
        m._pf_plan = plan
        m._pf_on = any(b > 0 for b, _ in plan.values())
        m._pf_stream = torch.cuda.Stream(device=m.lm_head.weight.device) if m._pf_on else None
    return m._pf_plan


def _prefetch(m, li, name, when):
    """issue the prefetch of the projection that FOLLOWS (li, name), if the plan asks for it at this point"""
    if not m._pf_on:
        return
    nxt, dl = _PF_NEXT[name]
    blocks, w = m._pf_plan[nxt]
    if blocks <= 0 or w != when or li + dl >= len(m._packed):
        return
    m._pf_stream.wait_stream(torch.cuda.current_stream())          # gate: not before the main branch got here
    with torch.cuda.stream(m._pf_stream):
        m._ops.weight_prefetch(m._packed[li + dl][nxt], blocks)


def forward_folded(m, tokens, positions, kv_len, key_start, cols=None, head_partials=False):
    """backbones._forward_folded for a ChameleonBackbone with the experiments its switches select:
      F1r, G1 q|k|v, F2 + K1 or K1F, G1 o + F1r or the reducing o, G1s or G1 gate|up + F3, G1 down or the reducing down -- or the MLP as one launch
    with the weight prefetches of the plan around each G1."""
    ops, w, cfg = m._ops, m._window, m.G1_CFG
    (H, Hkv, D, _), hid, inter, eps, (B, n) = w.heads, w.hid, w.inter, w.eps, tokens.shape
    T, h, pos = BB._window_rows(w, tokens, positions)
    _prefetch_plan(m)
    plain = BB._g1_of(m, T)

    def g1(x_, name, N_, K_):
        _prefetch(m, li, name, "g1")
        out = plain(x_, li, name, N_, K_)
        _prefetch(m, li, name, "after")
        return out

    params = getattr(m.attn, "params", None)
    want_fused = getattr(m, "gateup_fused", BB._GATEUP_FUSED_DEFAULT)
    fuse_mlp = want_fused and (T <= 64 or want_fused == "tall") and not m._pf_on and ops.gateup_silu_ok(T, inter, hid, cfg["gate_up"][0],
                                                                                                        isinstance(m._packed[0]["gate_up"], ops.PackedZ),
                                                                                                        getattr(m, "weights", None) is not None)
    # o / down with F1r as their tail (one launch each; the reducing kernel wants whole 512-column slices per workgroup pair: 8 waves)
    red = getattr(m, "reduce_fused", BB._REDUCE_FUSED_DEFAULT) and not m._pf_on
    raw = lambda name: not isinstance(m._packed[0][name], ops.Packed) and getattr(m, "weights", None) is None        # (the reducing kernel streams the uncompressed packing)
    h_dev = m.lm_head.weight.device
    red_o = red and raw("o") and ops.skinny_gemm_reduce_ok(T, hid, H * D, cfg["o"][0], 8, h_dev)
    red_d = red and raw("down") and ops.skinny_gemm_reduce_ok(T, hid, inter, cfg["down"][0], 8, h_dev)
    pair_mlp = (getattr(m, "mlp_pair", BB._MLP_PAIR_DEFAULT) and fuse_mlp and not red_d and h_dev.type == "cuda" and
                ops.mlp_pair_ok(T, inter, hid, m._packed[0]["gate_up"], m._packed[0]["down"], cfg["down"][0], cfg["down"][1], h_dev))
    delta, ss_next = None, None         # the down projection's split-K planes (summed by the next F1r), or the statistics its tail already wrote
    for li, qn in enumerate(w.qk_norms):
        rn = (ss_next if ss_next is not None else ops.residual_sumsq(h, delta), hid, eps)
        _chk(f"L{li} sumsq", rn[0][:, :T] if rn[0].dim() == 2 and rn[0].shape[1] >= T else rn[0])
        o = attention_block(m, _chk(f"L{li} qkv", g1(h, "qkv", (H + 2 * Hkv) * D, hid), T), li, qn, pos, B, n, params, kv_len, key_start, row_norm=rn)
        _chk(f"L{li} attention", o)
        if red_o:
            rn = (ops.skinny_gemm_reduce(o.view(T, H * D), m._packed[li]["o"], hid, H * D, cfg["o"][0], h, 8, cfg["o"][2]), hid, eps)
        else:
            rn = (ops.residual_sumsq(h, g1(o.view(T, H * D), "o", hid, H * D)), hid, eps)
        if pair_mlp:
            if getattr(m, "_pair_ready", None) is None or m._pair_ready.device != h.device:       # this backbone's own arrival counters
                m._pair_ready = torch.zeros(max(64, (inter + cfg["down"][0] - 1) // cfg["down"][0] + 1), dtype=torch.int32, device=h.device)
            _, delta = ops.mlp_pair(h, m._packed[li]["gate_up"], m._packed[li]["down"], inter, hid, cfg["down"][0], row_norm=rn, ready=m._pair_ready)
            ss_next = None
            continue
        if fuse_mlp:
            act = ops.gateup_silu(h, m._packed[li]["gate_up"], inter, hid, cfg["gate_up"][2], row_norm=rn)
        else:
            act = ops.silu_mul(g1(h, "gate_up", 2 * inter, hid), rows=T, dtype=h.dtype, row_norm=rn)
        _chk(f"L{li} act", act)
        if red_d:
            delta, ss_next = None, ops.skinny_gemm_reduce(act, m._packed[li]["down"], hid, inter, cfg["down"][0], h, 8, cfg["down"][2])
        else:
            delta, ss_next = g1(act, "down", hid, inter), None
        _chk(f"L{li} down", delta, T)
        _chk(f"L{li} h", h)
    if m._pf_on:
        torch.cuda.current_stream().wait_stream(m._pf_stream)       # every forked branch rejoins (hipGraph capture needs it)
    return BB._window_head(m, h, delta, ss_next, B, n, cols, head_partials)
