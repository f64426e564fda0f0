"""PyTorch(-ROCm) transformer backbones for the SJD engine.

Per north_star the transformer forward stays on PyTorch-ROCm (GEMMs -> hipBLASLt); what is hand
written is the draft-window attention + KV append (kernels K1/K3), which plug in through the
``attn`` callable of every layer.  There is NO torch/CPU attention in this package: the default
backend is the HIP one (ops.HipWindowAttention) and it raises if libsjd_hip.so is missing.  Tests
that need a CPU forward inject oracle.attention_ref.OracleWindowAttention explicitly.

State-dict keys follow the reference checkpoints so real weights load unchanged:
  * LlamaGenBackbone   <- reference llamagen/llamagen.py:297-419 (Transformer), RoPE :441-467
  * ChameleonBackbone  <- reference lumina_mgpt/model/chameleon/modeling_chameleon.py:59-82 (RMSNorm),
                          :198-219 (per-head QK LayerNorm), :144-178 (RoPE), :499-581 (attention),
                          :593-668 (decoder layer), :1494-1561 (lm_head, fp32 logits)
    with qk_norm=False / n_kv_heads<n_heads it is the Llama-style Emu3 LM
    (reference emu3/mllm/configuration_emu3.py:130-152) and, unchanged, HF Chameleon (Anole).

All backbones expose one hot-path entry point:
    forward_window(tokens [B,n] int64, positions [B,n] int64, kv_len, key_start [B]) -> logits [B,n,V] fp32
which writes the n new K/V rows of every layer at cache rows [kv_len, kv_len+n) and attends causally
inside the window; ``key_start[b]`` hides cache rows < key_start[b] (uncond prompt / left padding).
"""
import math
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F


from . import launch_shapes as LS

import logging as _logging
import os as _os
_log = _logging.getLogger("sjd_amd.backbones")

# The opt-in experiments of the folded window forward -- K1F / K1Fs, the reducing o / down tail, the one-launch MLP, the side-stream weight prefetch and
# `gateup_fused = "tall"` -- live in backbones_exp.py with their measurements; every one is OFF by default and calls libsjd_hip_exp.so.  This module only
# reads their switches (environment, or the instance attribute of the same name: _experiments_on) and imports backbones_exp when one is set.
_K1_FUSED_DEFAULT = _os.environ.get("SJD_K1_FUSED", "0") == "1"
_REDUCE_FUSED_DEFAULT = _os.environ.get("SJD_REDUCE_FUSED", "0") == "1"
_MLP_PAIR_DEFAULT = _os.environ.get("SJD_MLP_PAIR", "0") == "1"
_GATEUP_FUSED_DEFAULT = {"0": False, "tall": "tall"}.get(_os.environ.get("SJD_GATEUP_FUSED", "1"), True)     # kernel G1s (gate|up + F3 in one launch); 0: G1 then F3; tall: also above 64 rows (an experiment)
# the same switch for the swin-norm route's K = 8192 MXFP4 form (enable_fused(weights="mxfp4", swin_quant=True)).  OFF by default: measured on the whole 30B
# preset the fused launch is slower than G1q4 + F3 on the same copy (7.64 against 7.30 ms per step, 0.03 ms between rounds; 54.7 against 50.2 us per launch:
# every one of its 344 workgroups stages the whole 32 x 8192 activation -- profiles/swin30b_quant.json).  `backbone.gateup_fused = True` reaches the kernel.
_SWIN_GATEUP_FUSED_DEFAULT = False
_NAN_CHECK = _os.environ.get("SJD_NAN_CHECK", "0") == "1"                    # debug aid: name the first kernel whose output is not finite


def _experiments_on(m):
    """is one of backbones_exp's experiments switched on for backbone `m`?"""
    return bool(getattr(m, "k1_fused", _K1_FUSED_DEFAULT) or getattr(m, "reduce_fused", _REDUCE_FUSED_DEFAULT) or getattr(m, "mlp_pair", _MLP_PAIR_DEFAULT)
                or getattr(m, "gateup_fused", _GATEUP_FUSED_DEFAULT) == "tall"
                or getattr(m, "_pf_on", _os.environ.get("SJD_PREFETCH") or any(b > 0 for b, _ in m.PREFETCH.values())))          # (the plan, once backbones_exp resolved it)


def _exp():
    from . import backbones_exp
    return backbones_exp


def _chk(tag, x, rows=None):
    """SJD_NAN_CHECK=1: raise at the first forward stage whose output holds a non-finite value (rows: the valid rows of padded planes)"""
    if not _NAN_CHECK or x is None:
        return x
    t = x.data if hasattr(x, "n_chunks") else x
    v = t if rows is None else (t[:, :rows] if hasattr(x, "n_chunks") else t[:rows])
    if not torch.isfinite(v.float()).all():
        bad = (~torch.isfinite(v.float())).nonzero()
        raise FloatingPointError(f"{tag}: {bad.shape[0]} non-finite values, first at {bad[0].tolist()} of {tuple(v.shape)}")
    return x


def _head_logits(linear, x, cols):
    """fp32 logits of the output head, optionally only for the vocabulary columns [cols[0], cols[1]) -- the rows of the weight the
    grammar can give probability mass to in this iteration (Lumina image body: 8192 of 65536 ids).  K2 never reads a masked column,
    so the narrow head is bit-identical downstream and streams 1/8 of the weight."""
    if cols is None:
        return linear(x).float()
    w = linear.weight[cols[0]:cols[1]]
    b = linear.bias[cols[0]:cols[1]] if linear.bias is not None else None
    return F.linear(x, w, b).float()


def _packer(ops, weights, compress, st):
    """pack(w, kc, step_major, gateup=False) of either backbone's enable_fused, counting into its compress_stats `st`.  Under `weights` the quantised copy
    (its stream's packer, ops.pack_weight_<tag> of LS.STREAMS) or, for an "_as_bf16" twin, its dequantised values packed uncompressed; else the lossless 12-bit
    stream where `compress` asks for it and ops.pack_weight_z takes the matrix (a declined one is counted, and logged once per reason); else the plain packing."""
    stream, twin = LS.stream_of(weights)

    def pack(w, kc, sm, gateup=False):          # gateup: [Wg; Wu] in the two K halves the fused gate|up launch streams
        st["matrices"] += 1
        st["bytes_raw"] += w.numel() * w.element_size()
        if stream is not None:
            tag, z = stream.tag, getattr(ops, "pack_weight_" + stream.tag)(w, kc, sm, gateup=gateup)
            st[tag + "_matrices"] = st.get(tag + "_matrices", 0) + 1
            st["rel_rms_error"] = max(st.get("rel_rms_error", 0.0), z.stats["rel_rms_error"])
            if twin:
                st["bytes_packed"] += w.numel() * w.element_size()
                return ops.pack_weight(z.dequant(), kc, sm)
            st["bytes_packed"] += z.nbytes()
            st[tag + "_bytes_packed"] = st.get(tag + "_bytes_packed", 0) + z.nbytes()
            return z
        z = ops.pack_weight_z(w, kc, sm, gateup=gateup) if compress else None
        if z is None:
            if compress:      # asked for and declined: say so (a checkpoint with folded norm gains may land here; the plain stream is
                st["declined"] = st.get("declined", 0) + 1          # bit-identical but 25 % more bytes -- VERDICT r3 weak #12)
                why = ("dtype %s (the 12-bit form encodes bf16)" % str(w.dtype).replace("torch.", "") if w.dtype != torch.bfloat16
                       else "KC %d > 4096" % kc)
                seen = st.setdefault("declined_reasons", {})
                seen[why] = seen.get(why, 0) + 1
                if seen[why] == 1:         # once per reason; the count is in compress_stats["declined_reasons"]
                    (_log.info if w.dtype != torch.bfloat16 else _log.warning)(
                        "pack_weight_z declined a %dx%d matrix (%s): it streams uncompressed (G1 / G1s); further ones are counted in "
                        "compress_stats", w.shape[0], w.shape[1], why)
            st["bytes_packed"] += w.numel() * w.element_size()
            return ops.pack_weight(w, kc, sm)
        st["compressed"] += 1
        st["bytes_packed"] += z.nbytes()
        st["exceptions"] += z.n_exceptions
        st["units"] = st.get("units", 0) + z.stats.get("units", 0)
        st["raw_units"] = st.get("raw_units", 0) + z.stats.get("raw_units", 0)            # (round 6: units that travel verbatim, ops.PackedZ)
        st["max_exceptions_per_unit"] = max(st.get("max_exceptions_per_unit", 0), z.stats.get("max_exceptions", 0))
        return z
    return pack


def _refuse_quant_copy(prefix, g1_cfg, head_cfg, dims, max_rows, granule, reasons=LS.QUANT_REASONS):
    """ValueError for the first thing LS.quant_copy_errors finds: enable_fused calls it before anything is assigned"""
    for name, why in LS.quant_copy_errors(g1_cfg, dims, max_rows, granule, head_cfg, reasons)[:1]:
        raise ValueError(prefix + LS.quant_copy_refusal(name, why, granule, head_cfg if name == "head" else g1_cfg[name], dims.get(name, (0, 0))[1]))


def _pack_fused(m, ops, layers, pack, head=None, pack_head=None):
    """The packing loop of both enable_fused, after their validation.  layers: per layer (q|k|v Linears, o matrix, gate Linear, up Linear, down matrix,
    norm gain in front of q|k|v, norm gain in front of gate|up); a gain of None folds nothing.  Several q|k|v Linears and gate | up are concatenated ONCE and
    the parameters re-pointed at the slices (state dict unchanged, no extra memory): m._fused.  pack (None: no packed copy) packs the four projections
    on m.G1_CFG with the gains folded in: m._packed.  head = (matrix, final norm gain): the output head on G1, ONE packed copy with the
    gain folded in -- a launch covers only the vocabulary columns the grammar allows and K2 reads its split-K partials: m._packed_head, m._head_cols."""
    fold = lambda w, g: w if g is None else (w.float() * g.float()[None, :]).to(w.dtype)      # W' = W diag(gamma): the norm becomes a row scale (F2 / F3 / K2)

    def joined(linears):
        if len(linears) == 1:
            return linears[0].weight
        w, r0 = torch.cat([lin.weight for lin in linears], dim=0).contiguous(), 0
        for lin in linears:
            lin.weight.data, r0 = w[r0:r0 + lin.weight.shape[0]], r0 + lin.weight.shape[0]
        return w

    c = m.G1_CFG
    m._packed, m._fused, m._packed_head = [], [], None
    with torch.no_grad():
        for qkv_lin, wo, gate, up, wd, g_qkv, g_gu in layers:
            qkv, gu = joined(qkv_lin), joined([gate, up])           # gate | up: F3 / G1s read the gate half first
            m._fused.append((qkv, gu) if len(qkv_lin) > 1 else gu)
            if pack is not None:
                m._packed.append(dict(qkv=pack(fold(qkv, g_qkv), c["qkv"][0], c["qkv"][2]),
                                      o=pack(wo, c["o"][0], c["o"][2]),
                                      gate_up=pack(fold(gu, g_gu), c["gate_up"][0], c["gate_up"][2], gateup=2 * c["gate_up"][0] == gu.shape[1]),
                                      down=pack(wd, c["down"][0], c["down"][2])))
        if head is not None:
            wf = fold(*head)
            pad = (-wf.shape[0]) % 32
            if pad:
                # the columns past the vocabulary are never read (K2's rules end at V); they are copies of the last real row, not zeros:
                # a tile that is half zeros has no eight-exponent window, and the 12-bit packer declined Emu3's whole 184622-row head for
                # that ONE tile (round 5: 14 real rows x 2048 weights "out of window" in the last tile, every other unit <= 60)
                wf = torch.cat([wf, wf[-1:].expand(pad, -1)], dim=0)
            m._head_cols = wf.shape[0]
            m._packed_head = pack_head(wf, m.HEAD_CFG[0], m.HEAD_CFG[2])


@dataclass
class _WindowPath:
    """what the shared window forwards read where the two backbones differ, gathered once by enable_fused (the packed copies stay in m._packed)"""
    heads: tuple                  # (H, H_kv, D, DS); DS: the storage head dim of q, the cache rows and K1's output (128 for a padded head_dim 100)
    hid: int
    inter: int
    eps: float
    qk_norms: list                # per layer (q gain, q bias, k gain, k bias) of the QK-norm, or (None,) * 4
    inv_freq: Optional[torch.Tensor]          # F2's rotary frequencies (None: it reads a table, see the F2 keywords)
    attend_kw: dict               # K1's keyword arguments (a padded head_dim 100: the true head dim)
    embed: nn.Module
    norm: nn.Module               # the final norm
    head: nn.Module               # the output head


def _chunk(m, name, T, K_):
    """split-K chunk of projection `name` for a T-row window of K_ columns (LS.chunk_for_rows); ValueError where none exists"""
    return LS.chunk_for_rows(name, m.G1_CFG[name], T, K_, getattr(m, "weights", None), getattr(m, "max_rows", 64))


def _g1_of(m, T):
    """g1(x, li, name, N, K): kernel G1 over layer li's packed projection `name` on its launch shape, for a T-row window"""
    def g1(x_, li, name, N_, K_):
        cfg = m.G1_CFG[name]
        return m._ops.skinny_gemm(x_, m._packed[li][name], N_, K_, _chunk(m, name, T, K_), cfg[1], cfg[2])
    return g1


def _window_rows(w, tokens, positions):
    T = tokens.shape[0] * tokens.shape[1]
    return T, w.embed(tokens).view(T, -1).contiguous(), positions.reshape(T).contiguous()


def _window_head(m, h, delta, sumsq, B, n, cols, head_partials):
    """The end of a window forward.  head_partials (and a packed head): the final residual add + the output head as G1 split-K partials over the column
    window `cols` -> ops.HeadOut (K2 applies the folded final RMSNorm as a row scale and the 16-bit rounding of the head's output while it reads them);
    else F1 and the library head -> fp32 logits.  sumsq: the statistics of h when the last residual add is already done."""
    ops, w = m._ops, m._window
    if not (head_partials and m._packed_head is not None):
        x = ops.add_rmsnorm(h, None if sumsq is not None else delta, w.norm.weight, w.eps)
        return _head_logits(w.head, x, cols).view(B, n, -1)
    if sumsq is None:
        sumsq = ops.residual_sumsq(h, delta)
    lo, hi = cols if cols is not None else (0, m.vocab_size)
    lo32, hi32 = (lo // 32) * 32, min(m._head_cols, ((hi + 31) // 32) * 32)
    kc, tiles, sm = m.HEAD_CFG
    part = ops.skinny_gemm_cols(h, m._packed_head, m._head_cols, w.hid, kc, lo32, hi32 - lo32, tiles, sm)
    return ops.HeadOut(part, lo32, n if h.shape[0] > n else 0, h.dtype, row_norm=(sumsq, w.hid, w.eps))


def _forward_folded(m, tokens, positions, kv_len, key_start, cols, head_partials, *, f2_kw, fuse_rows):
    """The window forward with the RMSNorms folded away, for both backbones: the projections run on the residual stream h itself (norm gain inside the
    packed weight), F1r does the residual add and the per-slice sums of h^2, F2 / F3 / K2 apply the row scale on the partials.  Per layer
      F1r, G1 q|k|v, F2, K1, G1 o, F1r, G1s (up to fuse_rows rows, where ops.gateup_silu_ok allows) or G1 gate|up + F3, G1 down
    then the head (_window_head).  f2_kw: F2's keyword arguments per layer."""
    ops, w, cfg = m._ops, m._window, m.G1_CFG
    (H, Hkv, D, DS), hid, inter, eps, (B, n) = w.heads, w.hid, w.inter, w.eps, tokens.shape
    T, h, pos = _window_rows(w, tokens, positions)
    params = getattr(m.attn, "params", None)
    g1 = _g1_of(m, T)
    fuse_mlp = T <= fuse_rows and ops.gateup_silu_ok(T, inter, hid, cfg["gate_up"][0], isinstance(m._packed[0]["gate_up"], ops.PackedZ),
                                                     getattr(m, "weights", None) is not None)          # (a quantised copy's bf16 twin takes the 8-bit route)
    delta = None                        # the down projection's split-K planes, summed by the next F1r
    for li, qn in enumerate(w.qk_norms):
        rn = (ops.residual_sumsq(h, delta), hid, eps)
        _chk(f"L{li} sumsq", rn[0][:, :T] if rn[0].dim() == 2 and rn[0].shape[1] >= T else rn[0])
        qkv = _chk(f"L{li} qkv", g1(h, li, "qkv", (H + 2 * Hkv) * D, hid), T)
        q = ops.qknorm_rope_append(qkv, m.cache.k[li], m.cache.v[li], *qn, w.inv_freq, pos, B, n, H, Hkv, D, params, kv_len if params is None else 0,
                                   row_norm=rn, **f2_kw[li])
        o = _chk(f"L{li} attention", m.attn.attend(li, q, m.cache, kv_len, key_start, **w.attend_kw))
        rn = (ops.residual_sumsq(h, g1(o.view(T, H * DS), li, "o", hid, H * DS)), hid, eps)
        if fuse_mlp:       # G1s: gate|up with SiLU * up as its epilogue (one launch, no partial planes, bit-identical to G1 + F3)
            act = ops.gateup_silu(h, m._packed[li]["gate_up"], inter, hid, cfg["gate_up"][2], row_norm=rn)
        else:
            act = ops.silu_mul(g1(h, li, "gate_up", 2 * inter, hid), rows=T, dtype=h.dtype, row_norm=rn)
        delta = _chk(f"L{li} down", g1(_chk(f"L{li} act", act), li, "down", hid, inter), T)
        _chk(f"L{li} h", h)
    return _window_head(m, h, delta, None, B, n, cols, head_partials)


class StaticKVCache:
    """[n_layers, B, H_kv, S_max, D]: one contiguous D-row per (layer, batch, head, position)."""

    def __init__(self, n_layers, batch, n_kv_heads, s_max, head_dim, dtype, device):
        shape = (n_layers, batch, n_kv_heads, s_max, head_dim)
        self.k = torch.zeros(shape, dtype=dtype, device=device)
        self.v = torch.zeros(shape, dtype=dtype, device=device)
        self.s_max = s_max

    def nbytes(self):
        return self.k.numel() * self.k.element_size() * 2


# ------------------------------------------------------------------------------------------ LlamaGen
@dataclass
class LlamaGenArgs:
    dim: int = 768
    n_layer: int = 12
    n_head: int = 12
    n_kv_head: Optional[int] = None
    multiple_of: int = 256
    ffn_dim_multiplier: Optional[float] = None
    rope_base: float = 10000
    norm_eps: float = 1e-5
    num_classes: int = 1000
    caption_dim: int = 2048
    class_dropout_prob: float = 0.1
    model_type: str = "c2i"
    vocab_size: int = 16384
    cls_token_num: int = 1
    block_size: int = 256


class _RMSNorm(nn.Module):
    def __init__(self, dim, eps):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(dim))

    def forward(self, x):   # llamagen.py:176-181
        xf = x.float()
        out = (xf * torch.rsqrt(torch.mean(xf * xf, dim=-1, keepdim=True) + self.eps)).type_as(x)
        return out * self.weight


def _rope_2d_table(grid_size, n_elem, base, cls_token_num):
    """llamagen.py:441-454: (cls_token_num + grid^2, head_dim//2, 2) cos/sin table, zeros for the cond rows."""
    half_dim = n_elem // 2
    freqs = 1.0 / (base ** (torch.arange(0, half_dim, 2)[: (half_dim // 2)].float() / half_dim))
    t = torch.arange(grid_size)
    freqs = torch.outer(t, freqs)
    grid = torch.concat([freqs[:, None, :].expand(-1, grid_size, -1), freqs[None, :, :].expand(grid_size, -1, -1)], dim=-1)
    cache = torch.stack([torch.cos(grid), torch.sin(grid)], dim=-1).flatten(0, 1)
    return torch.cat([torch.zeros(cls_token_num, n_elem // 2, 2), cache])


def _rope_table_extended(freqs, s_max):
    """the (cos, sin) table F2 reads on the fused path: one row per cache position (>= s_max rows); the rows past cls + grid^2 repeat the
    last real row, which is what forward_embeds' positions.clamp(max=len - 1) reads there"""
    f = freqs.float()
    if s_max > f.shape[0]:
        f = torch.cat([f, f[-1:].expand(s_max - f.shape[0], -1, -1)])
    return f.contiguous()


def _apply_rope_interleaved(x, freqs):
    """llamagen.py:457-467.  x [B,n,H,D], freqs [B or 1,n,D/2,2]"""
    xs = x.float().reshape(*x.shape[:-1], -1, 2)
    fc = freqs.view(freqs.shape[0], xs.size(1), 1, xs.size(3), 2)
    out = torch.stack([xs[..., 0] * fc[..., 0] - xs[..., 1] * fc[..., 1],
                       xs[..., 1] * fc[..., 0] + xs[..., 0] * fc[..., 1]], dim=-1)
    return out.flatten(3).type_as(x)


class _LGAttention(nn.Module):
    def __init__(self, a: LlamaGenArgs):
        super().__init__()
        self.n_head = a.n_head
        self.n_kv_head = a.n_kv_head or a.n_head
        self.head_dim = a.dim // a.n_head
        self.dim = a.dim
        self.wqkv = nn.Linear(a.dim, (self.n_head + 2 * self.n_kv_head) * self.head_dim, bias=False)
        self.wo = nn.Linear(a.dim, a.dim, bias=False)


class _LGFeedForward(nn.Module):
    def __init__(self, a: LlamaGenArgs):
        super().__init__()
        hidden = int(2 * (4 * a.dim) / 3)
        if a.ffn_dim_multiplier is not None:
            hidden = int(a.ffn_dim_multiplier * hidden)
        hidden = hidden if hidden % a.multiple_of == 0 else hidden + a.multiple_of - (hidden % a.multiple_of)
        self.w1 = nn.Linear(a.dim, hidden, bias=False)
        self.w3 = nn.Linear(a.dim, hidden, bias=False)
        self.w2 = nn.Linear(hidden, a.dim, bias=False)

    def forward(self, x):
        return self.w2(F.silu(self.w1(x)) * self.w3(x))


class _LGBlock(nn.Module):
    def __init__(self, a: LlamaGenArgs):
        super().__init__()
        self.attention = _LGAttention(a)
        self.feed_forward = _LGFeedForward(a)
        self.attention_norm = _RMSNorm(a.dim, a.norm_eps)
        self.ffn_norm = _RMSNorm(a.dim, a.norm_eps)


class _LabelEmbedder(nn.Module):
    def __init__(self, num_classes, hidden, dropout_prob):
        super().__init__()
        self.embedding_table = nn.Embedding(num_classes + int(dropout_prob > 0), hidden)
        self.num_classes = num_classes


class _CapMLP(nn.Module):
    def __init__(self, cin, hidden):
        super().__init__()
        self.fc1 = nn.Linear(cin, hidden, bias=False)
        self.fc2 = nn.Linear(hidden, hidden, bias=False)

    def forward(self, x):
        return self.fc2(F.gelu(self.fc1(x), approximate="tanh"))


class _CaptionEmbedder(nn.Module):
    def __init__(self, cin, hidden, token_num):
        super().__init__()
        self.cap_proj = _CapMLP(cin, hidden)
        self.register_buffer("uncond_embedding", torch.zeros(token_num, cin))


class LlamaGenBackbone(nn.Module):
    def __init__(self, args: LlamaGenArgs, attn=None):
        super().__init__()
        self.args = args
        self.vocab_size = args.vocab_size
        self.num_classes = args.num_classes
        self.model_type = args.model_type
        self.cls_token_num = args.cls_token_num
        if args.model_type == "c2i":
            self.cls_embedding = _LabelEmbedder(args.num_classes, args.dim, args.class_dropout_prob)
        else:
            self.cls_embedding = _CaptionEmbedder(args.caption_dim, args.dim, args.cls_token_num)
        self.tok_embeddings = nn.Embedding(args.vocab_size, args.dim)
        self.layers = nn.ModuleList([_LGBlock(args) for _ in range(args.n_layer)])
        self.norm = _RMSNorm(args.dim, args.norm_eps)
        self.output = nn.Linear(args.dim, args.vocab_size, bias=False)
        grid = int(args.block_size ** 0.5)
        assert grid * grid == args.block_size
        self.freqs = _rope_2d_table(grid, args.dim // args.n_head, args.rope_base, args.cls_token_num)
        self.attn = attn
        self.cache = None
        self.n_heads, self.n_kv_heads = args.n_head, args.n_kv_head or args.n_head
        self.head_dim = args.dim // args.n_head
        self.n_layers = args.n_layer

    def setup_cache(self, batch, s_max, dtype=None, device=None):
        """the cache rows are head_dim wide -- or 128 wide with zero pad columns once enable_fused(pad_head_dim=True) has switched a
        head_dim-100 model (GPT-3B) to padded storage; the rotary table keeps its true width ([., head_dim / 2, 2])"""
        p = self.tok_embeddings.weight
        self.cache = StaticKVCache(self.n_layers, batch, self.n_kv_heads, s_max, getattr(self, "_head_pad", None) or self.head_dim,
                                   dtype or p.dtype, device or p.device)
        self.buffers_version = getattr(self, "buffers_version", 0) + 1
        self.freqs = self.freqs.to(p.device)
        self._rope_ext = _rope_table_extended(self.freqs, s_max)
        return self.cache

    def embed_condition(self, cond):
        """c2i: class ids [B] -> [B,1,dim]; t2i: caption embeddings [B,T,caption_dim] -> [B,T,dim] (llamagen.py:111-116,143-148)"""
        if self.model_type == "c2i":
            return self.cls_embedding.embedding_table(cond).unsqueeze(1)[:, : self.cls_token_num]
        return self.cls_embedding.cap_proj(cond)[:, : self.cls_token_num]

    def forward_embeds(self, h, positions, kv_len, key_start, cols=None):
        B, n, _ = h.shape
        freqs = self.freqs[positions.clamp(max=self.freqs.shape[0] - 1)]   # [B,n,D/2,2]; padded window rows clamp
        for li, layer in enumerate(self.layers):
            a = layer.attention
            x = layer.attention_norm(h)
            q, k, v = a.wqkv(x).split([a.dim, a.n_kv_head * a.head_dim, a.n_kv_head * a.head_dim], dim=-1)
            q = _apply_rope_interleaved(q.view(B, n, a.n_head, a.head_dim), freqs)
            k = _apply_rope_interleaved(k.view(B, n, a.n_kv_head, a.head_dim), freqs)
            v = v.view(B, n, a.n_kv_head, a.head_dim)
            o = self.attn(li, q, k, v, self.cache, kv_len, key_start)
            h = h + a.wo(o.reshape(B, n, a.dim))
            h = h + layer.feed_forward(layer.ffn_norm(h))
        return _head_logits(self.output, self.norm(h), cols)

    def forward_window(self, tokens, positions, kv_len, key_start, cols=None, head_partials=False):
        """head_partials: on the fused G1 window path return an ops.HeadOut (the output head's split-K partials for kernel K2) instead
        of fp32 logits; longer inputs (prefill) run forward_embeds and return logits as usual."""
        if getattr(self, "_ops", None) is not None and tokens.shape[0] * tokens.shape[1] <= getattr(self, "_fused_rows", 64):
            return self._forward_window_g1(tokens, positions, kv_len, key_start, cols, head_partials)
        return self.forward_embeds(self.tok_embeddings(tokens), positions, kv_len, key_start, cols=cols)

    # the tuned launch-shape sets under the names tools and tests read (launch_shapes.py holds them, with where each came from)
    (G1_CFG_LLAMAGEN, HEAD_CFG), (G1_CFG_LLAMAGEN_3B, HEAD_CFG_3B) = LS.LLAMAGEN_SETS[False, 64], LS.LLAMAGEN_SETS[True, 64]
    (G1_CFG_LLAMAGEN_128ROW, HEAD_CFG_128ROW), (G1_CFG_LLAMAGEN_3B_128ROW, HEAD_CFG_3B_128ROW) = LS.LLAMAGEN_SETS[False, 128], LS.LLAMAGEN_SETS[True, 128]
    (G1_CFG_LLAMAGEN_256ROW, HEAD_CFG_256ROW), (G1_CFG_LLAMAGEN_3B_256ROW, HEAD_CFG_3B_256ROW) = LS.LLAMAGEN_SETS[False, 256], LS.LLAMAGEN_SETS[True, 256]
    G1_WIDE_TILES = LS.WIDE_TILES
    HEAD_PAD = 128                # storage head dim of a padded model (the K1 / F2 shape of Lumina-7B: 32 heads, D 128, H == H_kv)

    @staticmethod
    def _pad_o_weight(wo, n_heads, head_dim, head_pad):
        """wo [dim, H * head_dim] -> [dim, H * head_pad]: zero columns at each head's pad positions, so K1's [T, H * head_pad] output feeds the o
        projection as it stands (its pad columns are zero and meet zero weights)"""
        w = wo.new_zeros(wo.shape[0], n_heads, head_pad)
        w[:, :, :head_dim] = wo.view(wo.shape[0], n_heads, head_dim)
        return w.view(wo.shape[0], n_heads * head_pad)

    def enable_fused(self, ops, gemm="sjd", max_rows=64, untuned_fp16=False, pad_head_dim=False, padded_batch=False, weights=None, compress=False):
        """Switch draft windows of <= max_rows rows (64, 128 or 256: rows = prompts per forward x CFG batch x window; fp16 weights take 256
        with untuned_fp16=True only: kernel G1w serves them on the launch shapes swept in bf16) to the hand-written HIP path: per layer F1r, G1 q|k|v, F2 (the interleaved rotary from a
        table, SJD_F2_ROPE_TABLE), K1, G1 o, F1r, G1 gate|up (+ F3, or G1s where ops.gateup_silu_ok allows), G1 down; then the output head
        on G1, whose split-K partials K2 reads (head_partials).  pad_head_dim=True serves head_dim 100 (GPT-3B) stored 128 wide: q|k|v is
        packed at its true size and F2 (SJD_F2_HEAD_PAD128) writes 128-wide q / cache rows with zero pad columns, K1 runs at D = 128 with the
        softmax scale of 100 (SJD_K1_HEAD_DIM_100), wo is packed with zero columns at the pad positions; the cache becomes 128 wide (an existing
        one is re-allocated: prefill again); windows of at most 64 rows unless padded_batch=True, which packs the padded model for max_rows 128 / 256 on
        the sets swept at GPT-3B's shapes (G1_CFG_LLAMAGEN_3B_128ROW / _256ROW: several prompts per forward; no effect without pad_head_dim=True at
        head_dim 100, nor at 64 rows); no effect at head_dim 64 / 128.  The RMSNorm gains are folded into packed copies of the weights (the
        norm becomes a row scale applied by F2 / F3 / K2, as ChameleonBackbone's folded path does).  w1 / w3 are concatenated once into
        [w1; w3] (gate | up) and re-pointed at its halves (state dict unchanged).  The prefill and longer inputs stay on forward_embeds.
        weights (default None: the packed copy holds the checkpoint's values, as above) -- LOSSY, opt-in, as on ChameleonBackbone:
          "e4m3" / "mxfp4"   the four per-layer projections are QUANTISED after norm folding (GPT-3B's wo as padded, zero pad columns included) and packed
                          with ops.pack_weight_q8 (one byte per weight) / ops.pack_weight_q4 (4.25 bits); lm_head and the prefill keep 16-bit parameters.
                          ONE copy serves every row count up to max_rows: <= 64 rows on kernels G1q / G1q4 (33..64 through LS.chunk_for_rows), 65..256 on
                          G1wq / G1wq4.  gate|up runs fused (G1sq / G1sq4) only where ops.gateup_silu_ok(..., packed_q8=True) allows (<= 32 rows, hidden
                          512 / 1024 / 2048 / 4096 packed in two K halves), else G1 + F3.  Launch shapes: LS.LLAMAGEN_QUANT_SETS (UNTUNED) unless the caller
                          set G1_CFG; either way they must pass LS.quant_copy_errors -- checked here, before anything is assigned.
          "e4m3_as_bf16" / "mxfp4_as_bf16"   the verification twins: pack_weight(dequant()) on the same chunks and the same fused / unfused route; every
                          token agrees with the quantised copy.
        compress_stats carries rel_rms_error (the largest over the matrices of RMS(w - dequant) / RMS(w)) and the packed bytes.  What either format does to
        image quality on a real checkpoint has NOT been measured.  bf16 only; not with untuned_fp16; dim and the intermediate size multiples of 128
        (mxfp4) / 32 (e4m3).
        compress (default False: nothing changes) -- LOSSLESS, opt-in: the packed copies of the four projections AND of the output head are kept in the 12-bit
        stream of ops.pack_weight_z (kernels G1z / G1sz, as ChameleonBackbone.enable_fused(compress=True)): about 0.78 of the bytes, the same split-K planes
        bit for bit, so every logit and token is that of compress=False on the same launch shapes.  Launch shapes: LS.LLAMAGEN_Z_SETS (UNTUNED: the 16-bit
        sets) unless the caller set G1_CFG / HEAD_CFG; either way they must pass LS.z_copy_errors.  ONE copy serves every row count up to max_rows = 64 or 128
        (the stream ends at LS.Z_MAX_ROWS rows).  gate|up stays G1z + F3 at LlamaGen's widths (LS.gateup_silu_ok).  GPT-3B's padded wo packs too: a unit of
        zero pad columns travels as exceptions or verbatim (a raw unit), never as a declined matrix.  compress_stats carries ChameleonBackbone's keys
        (compressed, exceptions, raw_units, declined, declined_reasons, ...).  Refused: fp16 weights (the format encodes bf16), together with `weights`
        (one stream per copy), max_rows=256, a chunk above LS.Z_MAX_KC.
        `ops` is sjd_amd.ops.  Raises ValueError for what the kernels do not serve -- a refused call leaves the backbone as it was."""
        stream = LS.stream_of(weights)[0]
        if weights is not None and not (stream is not None and "llamagen" in stream.has):
            raise ValueError(f"weights={weights!r}: " + ", ".join(["None"] + ["%r or %r" % s.names for s in LS.STREAMS if "llamagen" in s.has]))
        if gemm != "sjd":
            raise ValueError(f"LlamaGenBackbone.enable_fused serves gemm='sjd' only (the G1 weight-streaming kernels), got gemm={gemm!r}")
        dt = self.output.weight.dtype
        if dt not in (torch.bfloat16, torch.float16):
            raise ValueError(f"LlamaGenBackbone.enable_fused needs 16-bit weights (bf16 or fp16), got {dt}")
        if weights is not None and dt != torch.bfloat16:
            raise ValueError(f"weights={weights!r} needs bf16 weights (got {dt}): the dequantised values are bf16 numbers, fp16's exponent range does not hold them")
        if weights is not None and untuned_fp16:
            raise ValueError(f"weights={weights!r} packs bf16 weights: untuned_fp16=True does not go with it")
        if compress and dt != torch.bfloat16:          # (asked for by name: refused, not packed uncompressed behind the caller's back)
            raise ValueError(f"LlamaGenBackbone.enable_fused: compress=True needs bf16 weights (got {dt}): the 12-bit form encodes bf16, fp16's high byte "
                             "does not concentrate")
        if compress and weights is not None:
            raise ValueError(f"LlamaGenBackbone.enable_fused: compress=True does not go with weights={weights!r}: one stream per copy (the 12-bit stream "
                             "is lossless, a quantised copy is not)")
        pad100 = bool(pad_head_dim) and self.head_dim == 100
        if self.head_dim not in (64, 128) and not pad100:
            raise ValueError(f"LlamaGenBackbone.enable_fused: head_dim {self.head_dim} is not served (F2's table rotary takes head_dim 64 or 128; "
                             "head_dim 100 runs stored 128 wide with pad_head_dim=True)")
        if pad100:
            if self.n_heads != self.n_kv_heads:
                raise ValueError("LlamaGenBackbone.enable_fused: pad_head_dim=True serves multi-head attention (n_kv_head == n_head) only")
            if max_rows > 64 and not padded_batch:
                # (the plain call keeps what it did before the wider sets were swept: nobody's GPT-3B is packed for several prompts per forward unasked)
                raise ValueError("LlamaGenBackbone.enable_fused: pad_head_dim=True serves windows of at most 64 rows (one prompt per forward) unless "
                                 f"padded_batch=True, which packs max_rows={max_rows!r} on the launch shapes swept at head_dim 100 "
                                 "(G1_CFG_LLAMAGEN_3B_128ROW / _256ROW)")
            if self.args.dim % 32 != 0 or (3 * self.args.dim) % 32 != 0:
                raise ValueError(f"LlamaGenBackbone.enable_fused: dim {self.args.dim} -- kernel G1 takes whole 32-column tiles and 16-wide k-steps "
                                 "(dim a multiple of 32: at head_dim 100 a head count that is a multiple of 8)")
        if max_rows not in (64, 128, 256):
            raise ValueError(f"LlamaGenBackbone.enable_fused: max_rows is 64, 128 or 256 (the three sets of G1 launch shapes), got {max_rows!r}")
        if max_rows > 128 and dt != torch.bfloat16 and not untuned_fp16:
            # (the plain call keeps what it did before fp16 was served at 129..256 rows: nobody gets launch shapes that were never swept for fp16 unasked)
            raise ValueError("LlamaGenBackbone.enable_fused: max_rows=256 packs bf16 weights; it keeps fp16 windows of at most 128 rows unless "
                             "untuned_fp16=True (kernel G1 serves fp16 at 129..256 rows on the launch shapes swept in bf16)")
        if compress and max_rows > LS.Z_MAX_ROWS:
            raise ValueError(f"LlamaGenBackbone.enable_fused: compress=True serves windows of at most {LS.Z_MAX_ROWS} rows (the 12-bit stream's kernels end "
                             f"there, and one copy serves every row count up to max_rows), got max_rows={max_rows!r}: max_rows=64 or {LS.Z_MAX_ROWS}, or compress=False")
        # (a G1_CFG / HEAD_CFG set by the caller still wins)
        g1_cfg, head_cfg = (LS.LLAMAGEN_Z_SETS if compress else LS.LLAMAGEN_SETS if weights is None else LS.LLAMAGEN_QUANT_SETS)[pad100, max_rows]
        g1_cfg = self.__dict__.get("G1_CFG") or dict(g1_cfg)          # (the default keeps packing exactly what it packed before: the class's HEAD_CFG)
        head_cfg = self.__dict__.get("HEAD_CFG") or (head_cfg if max_rows > 64 or pad100 else None)
        if max_rows > 64:
            bad = [name for name, _ in LS.check_set(g1_cfg, head_cfg or self.HEAD_CFG)]
            if bad:
                raise ValueError(f"windows of more than 64 rows take {LS.WIDE_TILES} column tiles per workgroup; offending launch shapes: {bad}")
        if weights is not None:          # (one quantised copy for every row count: validated before anything is assigned)
            inter = self.layers[0].feed_forward.w1.weight.shape[0]
            if self.args.dim % stream.granule or inter % stream.granule:
                raise ValueError(f"weights={weights!r}: dim {self.args.dim} and the intermediate size {inter} must be multiples of {stream.granule} "
                                 + ("(the MXFP4 stream travels in whole ring trips of eight k-steps)" if stream.tag == "q4" else "(the e4m3 stream travels in whole record pairs)"))
            dims = LS.llamagen_dims(self.args.dim, self.n_heads, self.head_dim, inter, self.HEAD_PAD if pad100 else None)
            _refuse_quant_copy(f"weights={weights!r}, max_rows={max_rows}: ", g1_cfg, head_cfg or self.HEAD_CFG, dims, max_rows, stream.granule)
        if compress:          # (one 12-bit copy, the head's included: validated by shape before anything is assigned)
            inter = self.layers[0].feed_forward.w1.weight.shape[0]
            dims = dict(LS.llamagen_dims(self.args.dim, self.n_heads, self.head_dim, inter, self.HEAD_PAD if pad100 else None),
                        head=(self.output.weight.shape[0], self.args.dim))
            for name, why in LS.z_copy_errors(g1_cfg, dims, max_rows, head_cfg or self.HEAD_CFG)[:1]:
                raise ValueError(f"compress=True, max_rows={max_rows}: "
                                 + LS.z_copy_refusal(name, why, (head_cfg or self.HEAD_CFG) if name == "head" else g1_cfg[name], dims))
        self.G1_CFG = g1_cfg
        if head_cfg is not None:
            self.HEAD_CFG = tuple(head_cfg)
        self.weights = weights
        self.compress = bool(compress)
        self._max_rows_given = weights is not None          # (SJDBatchEngine: a quantised copy serves the rows it was packed for)
        self.compress_stats = (dict(matrices=0, compressed=0, bytes_raw=0, bytes_packed=0, exceptions=0, raw_units=0, declined=0, declined_reasons={})
                               if compress else dict(matrices=0, bytes_raw=0, bytes_packed=0))
        wo_of = (lambda w: self._pad_o_weight(w, self.n_heads, self.head_dim, self.HEAD_PAD)) if pad100 else (lambda w: w)
        layers = (([b.attention.wqkv], wo_of(b.attention.wo.weight), b.feed_forward.w1, b.feed_forward.w3, b.feed_forward.w2.weight,
                   b.attention_norm.weight, b.ffn_norm.weight) for b in self.layers)          # (a generator: one padded wo at a time)
        pack = _packer(ops, weights, bool(compress), self.compress_stats)
        _pack_fused(self, ops, layers, pack, (self.output.weight, self.norm.weight),          # (the 12-bit stream takes the head too, counted like a layer matrix;
                    pack if compress else lambda w, kc, sm: ops.pack_weight(w, kc, sm))          #  else it is neither quantised nor counted in compress_stats)
        self._ops = ops
        self._fused_rows = self.max_rows = int(max_rows)
        self.supports_head_partials = True
        self._head_pad = self.HEAD_PAD if pad100 else None
        self._window = _WindowPath((self.n_heads, self.n_kv_heads, self.head_dim, self._head_pad or self.head_dim), self.args.dim, self._fused[0].shape[0] // 2,
                                   self.args.norm_eps, [(None,) * 4] * self.n_layers, None, dict(head_dim=self.head_dim) if pad100 else {}, self.tok_embeddings,
                                   self.norm, self.output)
        if pad100 and self.cache is not None and self.cache.k.shape[-1] != self.HEAD_PAD:
            # (a cache set up before this call is head_dim wide: the same cache at the storage width, empty -- either order of the two calls ends 128 wide)
            ck = self.cache.k
            self.setup_cache(ck.shape[1], ck.shape[3], ck.dtype, ck.device)
        self.buffers_version = getattr(self, "buffers_version", 0) + 1          # captured hipGraphs hold the packed weights' addresses
        return self

    def packed_bytes(self):
        """bytes of packed weights one fused window forward streams (every layer and the whole output head)"""
        return sum(LS.packed_nbytes(w) for d in self._packed for w in d.values()) + LS.packed_nbytes(self._packed_head)

    def _forward_window_g1(self, tokens, positions, kv_len, key_start, cols=None, head_partials=False):
        """the folded window forward (_forward_folded) with F2's interleaved rotary from the table and, for a padded head_dim 100, K1 told the true head dim"""
        f2 = dict(dtype=self.tok_embeddings.weight.dtype, rope_table=self._rope_ext, head_pad=self._head_pad)
        return _forward_folded(self, tokens, positions, kv_len, key_start, cols, head_partials, f2_kw=[f2] * self.n_layers, fuse_rows=LS.WINDOW_MAX_ROWS)


# ------------------------------------------------------------------------------------------ Chameleon / Llama
@dataclass
class ChameleonArgs:
    vocab_size: int = 65536
    hidden_size: int = 4096
    intermediate_size: int = 11008
    num_hidden_layers: int = 32
    num_attention_heads: int = 32
    num_key_value_heads: int = 32
    rms_norm_eps: float = 1e-5
    rope_theta: float = 10000.0
    qk_norm: bool = True          # Chameleon/Lumina/Anole: True; Emu3 (Llama): False
    max_position_embeddings: int = 4096
    swin_norm: bool = False       # ChameleonSwinDecoderLayer (modeling_chameleon.py:670-735): the RMSNorm after each sublayer, not before it
    model_parallel_size: int = 1  # shards of the QK-norm gain / bias ([mp, head_dim], each row repeat-interleaved over heads / mp heads)


class _CRMSNorm(nn.Module):
    def __init__(self, dim, eps):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        self.variance_epsilon = eps

    def forward(self, x):       # modeling_chameleon.py:68-73
        dt = x.dtype
        xf = x.to(torch.float32)
        xf = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + self.variance_epsilon)
        return self.weight * xf.to(dt)


class _HeadLayerNorm(nn.Module):
    """ChameleonLayerNorm (modeling_chameleon.py:198-219): stats over head_dim, per-head gamma/beta.
    weight/bias are stored [model_parallel_size, head_dim]; row r serves heads [r * n_heads / mp, (r + 1) * n_heads / mp)."""

    def __init__(self, head_dim, n_heads, model_parallel_size=1):
        super().__init__()
        if model_parallel_size < 1 or n_heads % model_parallel_size:
            raise ValueError(f"model_parallel_size {model_parallel_size} must divide the {n_heads} heads of the QK-norm")
        self.weight = nn.Parameter(torch.ones(model_parallel_size, head_dim))
        self.bias = nn.Parameter(torch.zeros(model_parallel_size, head_dim))
        self.head_dim, self.n_heads = head_dim, n_heads
        self.heads_per_shard = n_heads // model_parallel_size

    def forward(self, x):       # x [..., n_heads, head_dim]
        x = F.layer_norm(x, (self.head_dim,), None, None, eps=1e-5)
        return (x * self.weight.repeat_interleave(self.heads_per_shard, dim=0)
                + self.bias.repeat_interleave(self.heads_per_shard, dim=0))


class _CAttention(nn.Module):
    def __init__(self, a: ChameleonArgs):
        super().__init__()
        self.num_heads, self.num_kv = a.num_attention_heads, a.num_key_value_heads
        self.head_dim = a.hidden_size // a.num_attention_heads
        self.q_proj = nn.Linear(a.hidden_size, self.num_heads * self.head_dim, bias=False)
        self.k_proj = nn.Linear(a.hidden_size, self.num_kv * self.head_dim, bias=False)
        self.v_proj = nn.Linear(a.hidden_size, self.num_kv * self.head_dim, bias=False)
        self.o_proj = nn.Linear(a.hidden_size, a.hidden_size, bias=False)
        if a.qk_norm:
            self.q_norm = _HeadLayerNorm(self.head_dim, self.num_heads, a.model_parallel_size)
            self.k_norm = _HeadLayerNorm(self.head_dim, self.num_kv, a.model_parallel_size)


class _CMLP(nn.Module):
    def __init__(self, a: ChameleonArgs):
        super().__init__()
        self.gate_proj = nn.Linear(a.hidden_size, a.intermediate_size, bias=False)
        self.up_proj = nn.Linear(a.hidden_size, a.intermediate_size, bias=False)
        self.down_proj = nn.Linear(a.intermediate_size, a.hidden_size, bias=False)

    def forward(self, x):
        return self.down_proj(F.silu(self.gate_proj(x)) * self.up_proj(x))


class _CLayer(nn.Module):
    def __init__(self, a: ChameleonArgs):
        super().__init__()
        self.self_attn = _CAttention(a)
        self.mlp = _CMLP(a)
        self.input_layernorm = _CRMSNorm(a.hidden_size, a.rms_norm_eps)
        self.post_attention_layernorm = _CRMSNorm(a.hidden_size, a.rms_norm_eps)


class _CModel(nn.Module):
    def __init__(self, a: ChameleonArgs):
        super().__init__()
        self.embed_tokens = nn.Embedding(a.vocab_size, a.hidden_size)
        self.layers = nn.ModuleList([_CLayer(a) for _ in range(a.num_hidden_layers)])
        self.norm = _CRMSNorm(a.hidden_size, a.rms_norm_eps)


def _rotate_half(x):
    h = x.shape[-1] // 2
    return torch.cat((-x[..., h:], x[..., :h]), dim=-1)


class ChameleonBackbone(nn.Module):
    def __init__(self, args: ChameleonArgs, attn=None):
        super().__init__()
        mp = args.model_parallel_size
        if mp < 1 or args.num_attention_heads % mp or args.num_key_value_heads % mp:
            raise ValueError(f"model_parallel_size {mp} must divide both num_attention_heads {args.num_attention_heads} and "
                             f"num_key_value_heads {args.num_key_value_heads}")
        self.args = args
        self.model = _CModel(args)
        self.lm_head = nn.Linear(args.hidden_size, args.vocab_size, bias=False)
        self.vocab_size = args.vocab_size
        self.n_layers = args.num_hidden_layers
        self.n_heads, self.n_kv_heads = args.num_attention_heads, args.num_key_value_heads
        self.head_dim = args.hidden_size // args.num_attention_heads
        inv = 1.0 / (args.rope_theta ** (torch.arange(0, self.head_dim, 2, dtype=torch.int64).float() / self.head_dim))
        self.register_buffer("inv_freq", inv, persistent=False)
        self.attn = attn
        self.cache = None

    def setup_cache(self, batch, s_max, dtype=None, device=None):
        p = self.lm_head.weight
        if self.args.swin_norm and dtype is not None and str(dtype).startswith("torch.float8"):
            raise ValueError("an fp8 KV cache is not served for swin-norm backbones (swin_norm=True): use a 16-bit cache")
        self.cache = StaticKVCache(self.n_layers, batch, self.n_kv_heads, s_max, self.head_dim, dtype or p.dtype,
                                   device or p.device)
        self.buffers_version = getattr(self, "buffers_version", 0) + 1      # captured hipGraphs hold the old cache's addresses
        return self.cache

    def _rope(self, positions, dtype):   # modeling_chameleon.py:97-110: fp32 angles, cast to activation dtype
        freqs = positions[:, :, None].float() * self.inv_freq.float()[None, None, :]
        emb = torch.cat((freqs, freqs), dim=-1)
        return emb.cos().to(dtype)[:, :, None, :], emb.sin().to(dtype)[:, :, None, :]

    # launch_shapes.py's tuned sets under the names bench.py, tools and tests read; G1_CFG / HEAD_CFG: the default when neither the caller nor LS.default_shapes sets another
    G1_CFG, G1_CFG_Z, G1_CFG_64ROW, G1_CFG_128ROW, G1_CFG_256ROW = LS.G1_CFG, LS.G1_CFG_Z, LS.G1_CFG_64ROW, LS.G1_CFG_128ROW, LS.G1_CFG_256ROW
    G1_CFG_EMU3, G1_CFG_EMU3_Z, G1_CFG_Q8, G1_CFG_EMU3_Q8 = LS.G1_CFG_EMU3, LS.G1_CFG_EMU3_Z, LS.G1_CFG_Q8, LS.G1_CFG_EMU3_Q8
    G1_CFG_Q8_WIDE, G1_CFG_EMU3_Q8_WIDE, G1_CFG_30B, G1_CFG_30B_Z = LS.G1_CFG_Q8_WIDE, LS.G1_CFG_EMU3_Q8_WIDE, LS.G1_CFG_30B, LS.G1_CFG_30B_Z
    G1_CFG_Q4, G1_CFG_EMU3_Q4 = LS.G1_CFG_Q4, LS.G1_CFG_EMU3_Q4
    HEAD_CFG, HEAD_CFG_WIDE, G1_WIDE_TILES = LS.HEAD_CFG, LS.HEAD_CFG_WIDE, LS.WIDE_TILES

    # Weight prefetch plan of the G1 window forward (an experiment: backbones_exp.py), projection -> (workgroups of the prefetch kernel, when it is issued).
    # 0 workgroups = no prefetch; override with SJD_PREFETCH="o:128:after,gate_up:0,..." or model.PREFETCH = {...} before the first forward.
    PREFETCH = dict(qkv=(0, "after"), o=(0, "after"), gate_up=(0, "after"), down=(0, "after"))
    _q8_chunk = _chunk

    def _dims(self):
        return LS.chameleon_dims(self.args.hidden_size, self.n_heads, self.n_kv_heads, self.head_dim, self.args.intermediate_size)

    def _q8_wide_check(self, cfg, head_cfg, max_rows, dims=None):
        """enable_fused(weights=..., max_rows > 64): can ONE e4m3 copy with launch shapes `cfg` serve every row count up to max_rows?  dims: the projections'
        (N, K) -- this backbone's by default.  ValueError names what cannot; nothing is assigned.  (Up to LS.Z_MAX_ROWS rows the head keeps its own kernels.)"""
        _refuse_quant_copy(f"max_rows={max_rows}: ", cfg, head_cfg if max_rows > LS.Z_MAX_ROWS else None, dims or self._dims(), max_rows, LS.STREAMS[0].granule)

    released_16bit = False        # enable_fused(..., release_16bit=True) has dropped the 16-bit layer matrices: the packed quantised copy is the only one

    def enable_fused(self, ops, gemm="torch", fold_norm=True, compress=None, weights=None, max_rows=None, swin_quant=False, release_16bit=False):
        """Switch to the fused HIP glue path (F1-F3): q|k|v and gate|up projections become single GEMMs whose weights are
        concatenated once; the original parameters are re-pointed at slices of the fused tensors (state-dict unchanged,
        no extra memory).  gemm="sjd": the window forward (<= 32 rows) also runs its four per-layer projections on the
        hand-written weight-streaming kernel G1 over pre-packed weights (a second, fragment-major copy of the layer
        weights); other shapes (prefill) keep hipBLASLt.  `ops` is sjd_amd.ops (raises if libsjd_hip.so is missing).
        compress (default: on for bf16 weights, SJD_G1Z=0 switches it off): the packed copy is kept in the LOSSLESS 12-bit stream format of
        kernels G1z / G1sz (ops.pack_weight_z: 25 % fewer bytes through the fabric that bounds the window forward, bit-identical results);
        a matrix that does not fit the format (fp16, or a unit with too many out-of-window weights) stays uncompressed.
        weights (default None: the packed copy holds the checkpoint's values, as above):
          "e4m3"          the four per-layer projections (q|k|v, o, gate|up, down) are QUANTISED -- after norm folding -- to OCP e4m3 with one
                          power-of-two scale per output column (ops.quantize_e4m3) and streamed at one byte per weight by kernels G1q / G1sq
                          (ops.pack_weight_q8): half of bf16's bytes, two thirds of the 12-bit stream's.  LOSSY, taken knowingly: `compress` is
                          ignored for them; lm_head is never quantised (12-bit or uncompressed as above).  Launch shapes: G1_CFG_Q8 /
                          G1_CFG_EMU3_Q8 unless the caller set G1_CFG.  compress_stats gains q8_matrices, q8_bytes_packed and rel_rms_error
                          (the largest over the matrices of RMS(w - dequant) / RMS(w)) -- what there is to judge a checkpoint by: what e4m3
                          weights do to image quality on a real checkpoint has NOT been measured.
          "e4m3_as_bf16"  the same quantisation, the DEQUANTISED values packed uncompressed (G1 / G1s): the verification and A/B twin -- the
                          same values at two bytes each, so every token agrees with "e4m3".
          "mxfp4"         the same four projections QUANTISED to OCP MXFP4 -- e2m1 codes with one power-of-two (e8m0) scale per output column and
                          block of 32 consecutive k (ops.quantize_mxfp4) -- and streamed at 4.25 bits per weight by kernels G1q4 / G1sq4
                          (ops.pack_weight_q4).  LOSSY and COARSER than e4m3 (one mantissa bit); what it does to image quality on a real checkpoint
                          has NOT been measured.  Launch shapes: G1_CFG_Q4 / G1_CFG_EMU3_Q4 (UNTUNED) unless the caller set G1_CFG; K and every chunk
                          must be multiples of LS.Q4_GRANULE.  At most 64 window rows: max_rows is None or 64 (there is no wide form).  compress_stats
                          gains q4_matrices, q4_bytes_packed and the format's rel_rms_error.
          "mxfp4_as_bf16" its verification twin: the dequantised values packed uncompressed, the same chunks and the same fused / unfused route.
          "e2m3"          the same four projections QUANTISED to 6-bit OCP e2m3 codes (three mantissa bits, as e4m3) with one power-of-two (e8m0) scale per
                          block of 32 weights (ops.quantize_e2m3: the block is an output column x 64-k record x MFMA lane half, NOT 32 consecutive k -- a
                          private stream format) and streamed at 6.25 bits per weight by kernels G1q6 / G1sq6 (ops.pack_weight_q6).  LOSSY, e4m3's error
                          class at 78 % of its bytes; what it does to image quality on a real checkpoint has NOT been measured.  Launch shapes: the MXFP4
                          sets G1_CFG_Q4 / G1_CFG_EMU3_Q4 (UNTUNED for this stream) unless the caller set G1_CFG; K and every chunk must be multiples of
                          LS.Q4_GRANULE.  At most 64 window rows: max_rows is None or 64.  No swin-norm / model_parallel_size > 1 (with or without
                          swin_quant) and no release_16bit: the stream has no K = 8192 gate|up form and no prefill kernel -- ValueError before anything is
                          assigned.  compress_stats gains q6_matrices, q6_bytes_packed and the format's rel_rms_error.
          "e2m3_as_bf16"  its verification twin: the dequantised values packed uncompressed, the same chunks and the same fused / unfused route.
        Only the window forward (inputs of at most 64 rows) reads the 8-bit copy: the prompt prefill (hipBLASLt on the 16-bit parameters) is
        NOT quantised.  SJD's draft and verify both run the window forward, so the sampler stays exact with respect to ITS model -- and that
        model is the quantised one.  8-bit weights serve bf16 backbones with gemm="sjd", no swin-norm / model_parallel_size > 1, at most 64
        window rows (one prompt per forward): anything else raises ValueError.  Chunks: every G1_CFG chunk <= LS.CHUNK_CAP_32ROW columns (checked here); at
        33..64 rows kernel G1q stages <= LS.CHUNK_CAP_64ROW, and a projection packed with a longer chunk is read in halved chunks where its packing allows
        it (step-major, see LS.chunk_for_rows: the default sets do) -- a forward that cannot raises ValueError before its first launch.
        max_rows (with weights only; default None = 64): 128 or 256 packs for several prompts per forward (SJDBatchEngine: rows = prompts x CFG batch x
        window) -- windows of 65..max_rows rows run on kernel G1wq, the 8-bit form of G1w ("e4m3_as_bf16": G1w itself, on the same launch shapes; the
        two stay token-identical).  Launch shapes: LS.default_shapes (UNTUNED sets) unless the caller set G1_CFG; ONE packed copy serves
        every row count, so it must pass LS.quant_copy_errors -- checked here, before anything is assigned.  max_rows=256: lm_head is packed UNCOMPRESSED
        whatever `compress` says (the 12-bit stream ends at LS.Z_MAX_ROWS rows) and HEAD_CFG[1] must be one of LS.WIDE_TILES.  Whether the 8-bit
        stream is faster than what those row counts run otherwise is a measurement, not a promise: README.md.
        swin_quant=True (with weights only): a swin-norm backbone (swin_norm=True, model_parallel_size > 1 included: the QK-norm shards live in F2, not in
        a projection) is quantised too -- without it such a backbone raises as before.  A swin layer has no norm in front of a projection, so the quantisers
        run on the checkpoint's own matrices; the unfolded window path streams the packed copies through ops.skinny_gemm.  LOSSY and opt-in like the rest;
        image quality on a real checkpoint has NOT been measured.  bf16 only, max_rows None or 64, no fp8 KV cache, lm_head and the prefill keep their
        16-bit parameters.  Launch shapes: LS.G1_CFG_30B_Q8 / LS.G1_CFG_30B_Q4 (UNTUNED) at hidden >= 8192 unless the caller set G1_CFG, which is checked
        (LS.quant_copy_errors on a granule of LS.Q4_GRANULE; e4m3: 32) before anything is assigned.  On "mxfp4" at hidden 8192 a window of <= 32 rows runs
        gate|up + SiLU * up as ONE launch over the four-chunk copy when the backbone's `gateup_fused` attribute is set to True (LS.gateup_silu_chunked_ok;
        measured slower than G1q4 + F3 with the untuned launch shapes, so the default is off: profiles/swin30b_quant.json);
        33..64 rows, "e4m3" (which has no fused form at K = 8192: G1q + F3), the "_as_bf16" twins and other widths run G1 + F3 on the same packed copy, so a
        twin stays token-identical to its stream.  `gateup_route` records, per row count, which of the two the last forward took.
        release_16bit=True (with weights only; opt-in, default False changes nothing): the PREFILL reads the packed copy too -- every input LS.serves_rows calls
        "prefill", and every input above 64 rows the window kernels were not packed for ("max_rows"), runs the per-layer sequence with kernel G1p
        (ops.prefill_gemm, any row count) as its multiplier: _forward_prefill_packed.  Prompt rows and window rows then come from ONE model, the quantised
        one, and after packing the data of every layer's q / k / v / o / gate / up / down parameters is released (the parameters are re-pointed at empty
        tensors, `_fused` goes; embed_tokens, the norms, the QK-norm gains and lm_head stay): compress_stats["bytes_released"] counts the bytes,
        `released_16bit` is True.  The "_as_bf16" twins run G1p over the plain packing, bit for bit their stream.  A released backbone refuses, with
        ValueError: a second enable_fused, the un-fused forward (`_ops` set to None) and state_dict() -- the checkpoint's matrices are gone.  Refused before
        anything is assigned: release_16bit without weights (the lossless 12-bit stream has no G1p form), gemm != "sjd", a non-bf16 backbone, K or a chunk that
        is no multiple of 32 (e4m3) / LS.Q4_GRANULE.  G1p's launch shape is UNTUNED and whether it is faster than the library GEMM at a row count is a
        measurement: README.md."""
        if self.released_16bit:
            raise ValueError("enable_fused: this backbone was packed with release_16bit=True -- its 16-bit layer matrices are gone, there is nothing to pack "
                             "again; load the checkpoint into a new backbone")
        if release_16bit:
            if weights is None:
                raise ValueError("release_16bit=True needs weights='e4m3' / 'mxfp4' (or an '_as_bf16' twin): kernel G1p reads those packed copies; the lossless "
                                 "12-bit stream has no G1p form, so its prefill keeps the 16-bit matrices")
            if gemm != "sjd":
                raise ValueError(f"release_16bit=True needs gemm='sjd' (the packed copies are read by the hand-written projection kernels only), got gemm={gemm!r}")
            if self.lm_head.weight.dtype != torch.bfloat16:
                raise ValueError(f"release_16bit=True needs a bf16 backbone (got {self.lm_head.weight.dtype}): the quantised streams and kernel G1p are bf16 only")
        stream = LS.stream_of(weights)[0]
        if weights is not None and stream is None:
            raise ValueError(f"weights={weights!r}: " + ", ".join(["None"] + ["%r or %r" % s.names for s in LS.STREAMS]))
        if stream is not None:          # (what the stream has no kernel for: a wide form, the swin-norm route, the prefill)
            if stream.max_rows <= 64 and max_rows not in (None, stream.max_rows):
                raise ValueError(f"weights={weights!r} serves windows of at most {stream.max_rows} rows (kernels {stream.kernels} have no wide form): max_rows is None or "
                                 f"{stream.max_rows}, got {max_rows!r}")
            if "swin" not in stream.has and (self.args.swin_norm or self.args.model_parallel_size > 1):
                raise ValueError(f"weights={weights!r} is not served for swin-norm backbones (swin_norm=True or model_parallel_size > 1), with or without swin_quant")
            if "prefill" not in stream.has and release_16bit:
                raise ValueError(f"weights={weights!r} has no prefill kernel (G1p reads the e4m3 / MXFP4 copies): release_16bit=True does not go with it")
        if max_rows is not None and weights is None:
            raise ValueError(f"max_rows={max_rows!r} goes with weights='e4m3' / 'e4m3_as_bf16' (without it the packed copy serves the row counts of its G1_CFG)")
        if max_rows not in (None, 64, 128, 256):
            raise ValueError(f"max_rows is 64, 128 or 256, got {max_rows!r}")
        if weights is not None:
            if gemm != "sjd":
                raise ValueError(f"weights={weights!r} needs gemm='sjd': the 8-bit stream is read by the hand-written projection kernels only (got gemm={gemm!r})")
            if (self.args.swin_norm or self.args.model_parallel_size > 1) and not swin_quant:
                raise ValueError(f"weights={weights!r} is not served for swin-norm backbones (swin_norm=True or model_parallel_size > 1)")
            if self.lm_head.weight.dtype != torch.bfloat16:
                raise ValueError(f"weights={weights!r} needs bf16 weights (got {self.lm_head.weight.dtype}): the dequantised values are bf16 numbers, "
                                 "fp16's exponent range does not hold them")
        if compress is None:
            compress = _os.environ.get("SJD_G1Z", "1") != "0"
        compress = bool(compress) and gemm == "sjd"
        # the caller has not chosen launch shapes: the tuned set of the architecture, stream and row count (None: the class default as it stands)
        g1_cfg, head_cfg = LS.default_shapes(self.lm_head.weight.dtype, self.__dict__.get("G1_CFG"), self.__dict__.get("HEAD_CFG"), self.args.hidden_size >= 8192,
                                             self.n_kv_heads != self.n_heads, compress, weights, max_rows, self.vocab_size)
        swin_q = weights is not None and (self.args.swin_norm or self.args.model_parallel_size > 1)
        if swin_q and max_rows not in (None, 64):
            raise ValueError(f"weights={weights!r} serves swin-norm backbones at windows of at most 64 rows (one prompt per forward): max_rows is None or 64, got {max_rows!r}")
        if weights is not None:          # (validated before anything is assigned: a refused call leaves the backbone as it was)
            # ONE copy serves every row count it is packed for.  A plain e4m3 copy for <= 64 rows is held only to what 32 rows stage: it packs, and a 33..64-row
            # window it cannot read in halved chunks is refused at the forward (_q8_chunk); a stream without a wide form, swin-norm and max_rows > 64 are held to the whole rule
            rows = max_rows or 64
            reasons = LS.QUANT_REASONS if stream.max_rows <= 64 or swin_q or rows > 64 else ("granule", "chunk") if release_16bit else ("chunk",)          # (G1p: whole record pairs)
            _refuse_quant_copy(f"weights={weights!r}: " if rows <= 64 else f"weights={weights!r}, max_rows={max_rows}: ", g1_cfg,
                               (head_cfg or self.HEAD_CFG) if rows > LS.Z_MAX_ROWS else None, self._dims(), rows, stream.granule, reasons=reasons)
            self.max_rows, self._max_rows_given = int(max_rows) if max_rows is not None else 64, max_rows is not None
        else:
            self.__dict__.pop("max_rows", None)
            self._max_rows_given = False
        if g1_cfg is not None:
            self.G1_CFG = g1_cfg
        if head_cfg is not None:
            self.HEAD_CFG = head_cfg
        self.weights = weights
        self.gateup_route = {}            # window rows -> "fused" / "g1+f3": what the last swin-norm window forward of that height ran gate|up on
        self._ops = ops
        self._gemm = gemm
        # swin-norm layers have no norm in front of a projection: nothing to fold (the unfolded window path, F1 in its post-norm form)
        self._fold_norm = bool(fold_norm) and gemm == "sjd" and not self.args.swin_norm
        self.compress = compress
        self.compress_stats = dict(matrices=0, compressed=0, bytes_raw=0, bytes_packed=0, exceptions=0)

        pack = pack_head = _packer(ops, None, compress, self.compress_stats)
        if weights is not None:
            pack = _packer(ops, weights, compress, self.compress_stats)          # the layer projections: the quantised copy or its twin
            if self.max_rows > 128:          # 129..256 rows: the head runs on kernel G1w, which streams the uncompressed packing
                pack_head = lambda w, kc, sm: ops.pack_weight(w, kc, sm)
        fold, L_ = self._fold_norm, self.model.layers          # (swin-norm, fold_norm=False: the packed copy holds the matrices as they are)
        layers = (([b.self_attn.q_proj, b.self_attn.k_proj, b.self_attn.v_proj], b.self_attn.o_proj.weight, b.mlp.gate_proj, b.mlp.up_proj, b.mlp.down_proj.weight,
                   b.input_layernorm.weight if fold else None, b.post_attention_layernorm.weight if fold else None) for b in L_)
        with_head = gemm == "sjd" and fold and self.lm_head.bias is None
        _pack_fused(self, ops, layers, pack if gemm == "sjd" else None, (self.lm_head.weight, self.model.norm.weight) if with_head else None, pack_head)
        self._inv_freq32 = self.inv_freq.float().contiguous()
        qn = [(a.q_norm.weight, a.q_norm.bias, a.k_norm.weight, a.k_norm.bias) if self.args.qk_norm else (None,) * 4 for a in (b.self_attn for b in L_)]
        self._window = _WindowPath((self.n_heads, self.n_kv_heads, self.head_dim, self.head_dim), self.args.hidden_size, self.args.intermediate_size,
                                   self.args.rms_norm_eps, qn, self._inv_freq32, {}, self.model.embed_tokens, self.model.norm, self.lm_head)
        if release_16bit:
            self._release_16bit()
        self.buffers_version = getattr(self, "buffers_version", 0) + 1          # ... and the packed weights' (engine._check_graph_buffers)
        return self

    def _layer_projections(self):
        """the seven projection parameters of every layer: what release_16bit=True releases"""
        for b in self.model.layers:
            a, m = b.self_attn, b.mlp
            yield from (a.q_proj.weight, a.k_proj.weight, a.v_proj.weight, a.o_proj.weight, m.gate_proj.weight, m.up_proj.weight, m.down_proj.weight)

    def _release_16bit(self):
        """drop the 16-bit layer matrices behind the packed quantised copy: the parameters keep their names and point at empty tensors, `_fused` (the
        concatenated q|k|v and gate|up matrices they were views of) goes with them"""
        released = 0
        for p in self._layer_projections():
            released += p.numel() * p.element_size()
            p.data = torch.empty(0, dtype=p.dtype, device=p.device)
        del self._fused
        self.compress_stats["bytes_released"] = released
        self.released_16bit = True

    def state_dict(self, *args, **kwargs):
        if self.released_16bit:
            raise ValueError("state_dict(): this backbone was packed with release_16bit=True -- the 16-bit layer matrices are gone and the quantised copy is "
                             "lossy, so there is no checkpoint to save; save from a backbone that still holds them")
        return super().state_dict(*args, **kwargs)

    def packed_bytes(self, head=True):
        """bytes of packed weights one window forward streams: the four projections of every layer and (head=True) the whole output head"""
        per = sum(LS.packed_nbytes(w) for d in self._packed for w in d.values())
        return per + (LS.packed_nbytes(self._packed_head) if head and self._packed_head is not None else 0)

    supports_head_partials = True

    @torch.no_grad()
    def calibrate_kv_scales(self, tokens, positions, key_start, headroom=4.0):
        """Per-layer (k, v) scales of an fp8 KV cache from a calibration prefill (round 6; VERDICT r5 #2b: the product used to leave
        (1.0, 1.0)): the prompt `tokens` [B, P] runs once through the prefill path on a TEMPORARY 16-bit cache, each layer's amax |K| and |V|
        over the prompt's rows sets scale = amax * headroom / 448 (448 = e4m3's largest finite value; headroom 4: later keys may exceed the
        prompt's range, and a float format loses no precision to headroom until its small end underflows -- sixteen binades further down).
        Static calibration: run once per backbone, BEFORE the first window hipGraph is captured (the scales are kernel arguments);
        the engines do on the first prompt they decode over an fp8 cache.  Leaves self.cache untouched.  -> the list it installed."""
        attn, cache = self.attn, self.cache
        if attn is None or not hasattr(attn, "layer_scales"):
            return None
        B, P = tokens.shape
        tmp = StaticKVCache(len(self.model.layers), B, self.n_kv_heads, ((P + 31) // 32) * 32, self.head_dim, self.lm_head.weight.dtype, tokens.device)
        saved = (getattr(attn, "params", None), attn.regime)
        self.cache, attn.params, attn.regime = tmp, None, "keysplit"
        try:
            self.forward_window(tokens, positions, 0, key_start)
        finally:
            self.cache, attn.params, attn.regime = cache, saved[0], saved[1]
        scales = []
        for li in range(len(self.model.layers)):
            ka = float(tmp.k[li][:, :, :P].abs().amax().float())
            va = float(tmp.v[li][:, :, :P].abs().amax().float())
            scales.append((max(ka, 1e-6) * headroom / 448.0, max(va, 1e-6) * headroom / 448.0))
        attn.layer_scales = scales
        self.buffers_version = getattr(self, "buffers_version", 0) + 1      # (captured graphs hold the old scales as kernel arguments)
        return scales

    def _f2_kw(self, li):
        """F2's keyword arguments for layer li: an fp8 cache gets its rows quantised in the same launch (that layer's scales); the QK-norm shards"""
        return dict(kv_scale=self.attn.scale_of(li) if hasattr(self.attn, "scale_of") else (1.0, 1.0), dtype=self.lm_head.weight.dtype,
                    qk_shards=self.args.model_parallel_size)

    def _f2(self, qkv, li, qn, pos, B, n, params, kv_len, row_norm=None):
        """F2 (QK-norm + RoPE + KV append) of the unfolded paths"""
        return self._ops.qknorm_rope_append(qkv, self.cache.k[li], self.cache.v[li], *qn, self._inv_freq32, pos, B, n, self.n_heads, self.n_kv_heads, self.head_dim,
                                            params, kv_len if params is None else 0, row_norm=row_norm, **self._f2_kw(li))

    def _f2_k1(self, qkv, li, qn, pos, B, n, params, kv_len, key_start, tag=None):
        """F2 then K1 (+ combine) of one layer on the q|k|v projection's output"""
        q = self._f2(qkv, li, qn, pos, B, n, params, kv_len)
        return self.attn.attend(li, _chk(f"{tag} L{li} q", q) if tag else q, self.cache, kv_len, key_start)

    def _forward_window_g1_folded(self, tokens, positions, kv_len, key_start, cols=None, head_partials=False):
        """the folded window forward (_forward_folded): F2 with the QK-norm and this layer's cache scales, G1s up to 64 rows unless `gateup_fused` is off
        (65..128-row windows: the four-row-tile G1s is served -- ops.gateup_silu_ok -- but the eight-wave 8-step G1 + F3 measured faster, 4.89 against
        5.06 ms per step with four prompts, profiles/r3_g1_tiled8.txt).  With an experiment switched on: backbones_exp's forward."""
        if _experiments_on(self):
            return _exp().forward_folded(self, tokens, positions, kv_len, key_start, cols, head_partials)
        return _forward_folded(self, tokens, positions, kv_len, key_start, cols, head_partials, f2_kw=[self._f2_kw(li) for li in range(self.n_layers)],
                               fuse_rows=64 if getattr(self, "gateup_fused", _GATEUP_FUSED_DEFAULT) else 0)

    def _forward_unfolded(self, tokens, positions, kv_len, key_start, cols, mm, attention, fused_mlp=False, tag=None):
        """A forward with the norms as launches of their own, the multiplier mm(x, li, name, N, K) given: kernel G1 over the packed copies (split-K partials
        flow straight into the consuming glue kernel) or the library GEMM.  Pre-norm layers: F1, q|k|v, F2, K1, o, F1, gate|up, F3, down.  Swin-norm: the
        projection reads h itself and each sublayer ends in ONE F1 launch in its post-norm form (h += norm(sublayer)).  attention: F2 + K1 (_f2_k1);
        fused_mlp: gate|up + F3 as one launch over the packed copy; tag: the path's name in its SJD_NAN_CHECK stages (None: it has none)."""
        ops, w, swin = self._ops, self._window, self.args.swin_norm
        (H, Hkv, D, _), hid, inter, eps, (B, n) = w.heads, w.hid, w.inter, w.eps, tokens.shape
        T, h, pos = _window_rows(w, tokens, positions)
        params = getattr(self.attn, "params", None)
        delta = None
        chk = (lambda stage, x: _chk(f"{tag} L{li} {stage}", x)) if tag else (lambda stage, x: x)
        for li, (layer, qn) in enumerate(zip(self.model.layers, w.qk_norms)):
            n1, n2 = layer.input_layernorm.weight, layer.post_attention_layernorm.weight
            x = h if swin else ops.add_rmsnorm(h, delta, n1, eps)
            qkv = chk("qkv", mm(x, li, "qkv", (H + 2 * Hkv) * D, hid))
            o = chk("attention", attention(qkv, li, qn, pos, B, n, params, kv_len, key_start, tag=tag))
            attn_out = mm(o.view(T, H * D), li, "o", hid, H * D)
            if swin:           # (the swin-norm order: the norms sit behind the sublayers, h is the next projection's input)
                x = chk("norm1", ops.add_rmsnorm_post(h, attn_out, n1, eps))
            else:
                x = chk("norm2", ops.add_rmsnorm(h, attn_out, n2, eps))
            if fused_mlp:      # (swin-norm on the MXFP4 stream at hidden 8192: the K = 8192 form of G1sq4 over the four-chunk copy; same bits as G1q4 + F3)
                act = ops.gateup_silu(x, self._packed[li]["gate_up"], inter, hid, self.G1_CFG["gate_up"][2])
            else:
                gu = mm(x, li, "gate_up", 2 * inter, hid)
                act = ops.silu_mul(gu) if isinstance(gu, torch.Tensor) else ops.silu_mul(gu, rows=T, dtype=h.dtype)          # (split-K planes carry neither)
            delta = chk("mlp", mm(act, li, "down", hid, inter))
            if swin:
                ops.add_rmsnorm_post(h, delta, n2, eps)
                delta = None
        return _window_head(self, h, delta, None, B, n, cols, False)

    def _forward_window_g1(self, tokens, positions, kv_len, key_start, cols=None):
        """Window forward with the norms unfolded (fold_norm=False, swin-norm backbones) and the four per-layer projections on kernel G1"""
        ops, T, cfg = self._ops, tokens.shape[0] * tokens.shape[1], self.G1_CFG
        cap = LS.CHUNK_CAP_32ROW if T <= 32 else 1 << 30     # the staged activation chunk of a 32-row window must fit in LDS; taller windows are sub-tiled when it does not
        if any(c[0] > cap for c in cfg.values()):
            raise ValueError(f"G1_CFG chunk sizes must be <= {cap} for a {T}-row window")
        swin, gu = self.args.swin_norm, self._packed[0]["gate_up"]
        stream = ops.streamed(gu)[0]          # (a copy whose stream has the four-chunk form of the fused launch: MXFP4)
        fused_mlp = bool(swin and getattr(self, "gateup_fused", _SWIN_GATEUP_FUSED_DEFAULT) and stream is not None and "gateup_k4" in stream.has
                         and LS.gateup_silu_chunked_ok(T, self.args.intermediate_size, self.args.hidden_size, gu.KC))
        if swin and getattr(self, "weights", None) is not None:
            self.gateup_route[T] = "fused" if fused_mlp else "g1+f3"
        k1f = getattr(self, "k1_fused", _K1_FUSED_DEFAULT)          # (an experiment: one launch for F2 + K1 where kernel K1F serves the shape)
        attention = (lambda *a, **k: _exp().attention_block(self, *a, **k)) if k1f else self._f2_k1
        return self._forward_unfolded(tokens, positions, kv_len, key_start, cols, _g1_of(self, T), attention, fused_mlp)

    def _forward_prefill_packed(self, tokens, positions, kv_len, key_start, cols=None):
        """The prefill of a backbone packed with release_16bit=True, at any row count: the per-layer sequence F1, q|k|v, F2, K1, o, F1, gate|up, F3, down with
        kernel G1p (ops.prefill_gemm over self._packed[li], read as packed) as its multiplier -> fp32 logits.  Swin-norm (and fold_norm=False): the copies
        hold the matrices as they are, the sequence is _forward_unfolded's with its norm launches.  Pre-norm with folded gains: the copies hold W diag(gamma),
        so the projection runs on the residual stream itself and G1p applies rsqrt(mean h^2 + eps) as its row scale to the fp32 sums -- the window
        forward's definition (_forward_folded: F2 / F3), so prompt rows and window rows come from the same model."""
        ops, w = self._ops, self._window

        def g1p(x, li, name, N_, K_, row_scale=None):
            kc, _, sm = self.G1_CFG[name]
            return ops.prefill_gemm(x, self._packed[li][name], N_, K_, row_scale, KC=kc, step_major=sm)
        if not self._fold_norm:
            return self._forward_unfolded(tokens, positions, kv_len, key_start, cols, g1p, self._f2_k1, tag="prefill")
        (H, Hkv, D, _), hid, inter, eps, (B, n) = w.heads, w.hid, w.inter, w.eps, tokens.shape
        T, h, pos = _window_rows(w, tokens, positions)
        params = getattr(self.attn, "params", None)
        row_scale = lambda: torch.rsqrt(h.float().square().mean(dim=1) + eps)          # fp32 [T]: the un-gained RMSNorm of the residual stream
        delta = None
        for li, qn in enumerate(w.qk_norms):
            if delta is not None:
                h += delta
            qkv = _chk(f"prefill L{li} qkv", g1p(h, li, "qkv", (H + 2 * Hkv) * D, hid, row_scale()))
            o = _chk(f"prefill L{li} attention", self._f2_k1(qkv, li, qn, pos, B, n, params, kv_len, key_start, tag="prefill"))
            h += g1p(o.view(T, H * D), li, "o", hid, H * D)
            act = ops.silu_mul(_chk(f"prefill L{li} gate_up", g1p(h, li, "gate_up", 2 * inter, hid, row_scale())))
            delta = _chk(f"prefill L{li} down", g1p(act, li, "down", hid, inter))
        return _window_head(self, h, delta, None, B, n, cols, False)

    def _forward_window_fused(self, tokens, positions, kv_len, key_start, cols=None, head_partials=False):
        T_ = tokens.shape[0] * tokens.shape[1]
        no = LS.serves_rows(self, T_, tokens.shape[1])
        if self.released_16bit and no is not None and (no[0] == "prefill" or T_ > 64):          # (a released copy serves every row count: G1p)
            return self._forward_prefill_packed(tokens, positions, kv_len, key_start, cols)
        if no is not None and no[0] == "max_rows":          # (an 8-bit copy packed for fewer rows: there is no 16-bit copy to fall back on)
            stream = LS.stream_of(self.weights)[0]
            if stream.max_rows <= 64:
                raise ValueError(f"weights={self.weights!r} serves draft windows of at most {stream.max_rows} rows (kernels {stream.kernels} have no wide form); got {T_} rows")
            if no[1] > 64:
                raise ValueError(f"weights='e4m3' serves draft windows of at most {no[1]} rows (max_rows={no[1]}); got {T_} rows")
            raise ValueError(f"weights='e4m3' serves draft windows of at most 64 rows (one prompt per forward); got {T_} rows")
        if getattr(self, "weights", None) is not None and self._gemm == "sjd" and 32 < T_ <= 64:          # (refuse before the first launch, not in the middle of a layer)
            for name_, (_, K_) in self._dims().items():
                self._q8_chunk(name_, T_, K_)
        # G1 serves windows: <= 64 rows, or <= 256 rows of up to eight prompts' draft windows (n <= 32 rows per batch row; 129..256 rows: round 5, the
        # uncompressed packing on kernel G1w -- G1_CFG_256ROW); longer inputs are prefill
        if no is None:
            if self._fold_norm:
                return self._forward_window_g1_folded(tokens, positions, kv_len, key_start, cols, head_partials)
            return self._forward_window_g1(tokens, positions, kv_len, key_start, cols)     # (swin-norm backbones: always here)
        def linear(x, li, name, N_, K_):          # the library GEMM over the concatenated matrices and the o / down parameters
            layer, (qkv_w, gu_w) = self.model.layers[li], self._fused[li]
            return F.linear(x, dict(qkv=qkv_w, o=layer.self_attn.o_proj.weight, gate_up=gu_w, down=layer.mlp.down_proj.weight)[name])
        return self._forward_unfolded(tokens, positions, kv_len, key_start, cols, linear, self._f2_k1, tag="prefill")

    def forward_window(self, tokens, positions, kv_len, key_start, cols=None, head_partials=False):
        """cols = (lo, hi): compute the logits of vocabulary columns [lo, hi) only (returned compact, [B, n, hi - lo]).
        head_partials: on the G1 folded-norm path return an ops.HeadOut (split-K partials of the output head for kernel K2) instead of
        materialised fp32 logits; paths that cannot (library GEMMs, prefill shapes) return logits as usual."""
        if getattr(self, "_ops", None) is not None:
            return self._forward_window_fused(tokens, positions, kv_len, key_start, cols, head_partials)
        if self.released_16bit:
            raise ValueError("the un-fused forward reads the 16-bit layer matrices, which release_16bit=True released: a released backbone runs on the "
                             "fused HIP path only (`_ops` must stay set)")
        B, n = tokens.shape
        h = self.model.embed_tokens(tokens)
        cos, sin = self._rope(positions, h.dtype)
        for li, layer in enumerate(self.model.layers):
            a = layer.self_attn
            x = h if self.args.swin_norm else layer.input_layernorm(h)
            q = a.q_proj(x).view(B, n, a.num_heads, a.head_dim)
            k = a.k_proj(x).view(B, n, a.num_kv, a.head_dim)
            v = a.v_proj(x).view(B, n, a.num_kv, a.head_dim)
            if self.args.qk_norm:
                q, k = a.q_norm(q), a.k_norm(k)
            q = q * cos + _rotate_half(q) * sin          # modeling_chameleon.py:175-176
            k = k * cos + _rotate_half(k) * sin
            o = self.attn(li, q, k, v, self.cache, kv_len, key_start)
            if self.args.swin_norm:          # modeling_chameleon.py:717-728: sublayer output (dtype), fp32 norm cast to dtype, gain, residual add
                h = h + layer.input_layernorm(a.o_proj(o.reshape(B, n, -1)))
                h = h + layer.post_attention_layernorm(layer.mlp(h))
                continue
            h = h + a.o_proj(o.reshape(B, n, -1))
            h = h + layer.mlp(layer.post_attention_layernorm(h))
        return _head_logits(self.lm_head, self.model.norm(h), cols)   # modeling_chameleon.py:1560-1561


LUMINA_7B = ChameleonArgs()
# the Chameleon-30B form (swin-norm layers, QK-norm gains in four shards: convert_chameleon_weights_to_hf.py's 30B branch).  The shapes were
# not checked against a released config.json: every test and tool takes them from here, so a correction is this one line
CHAMELEON_30B = ChameleonArgs(vocab_size=65536, hidden_size=8192, intermediate_size=22016, num_hidden_layers=48, num_attention_heads=64,
                              num_key_value_heads=8, model_parallel_size=4, swin_norm=True)
EMU3_8B = ChameleonArgs(vocab_size=184622, hidden_size=4096, intermediate_size=14336, num_hidden_layers=32,
                        num_attention_heads=32, num_key_value_heads=8, rms_norm_eps=1e-5, rope_theta=1000000.0,
                        qk_norm=False, max_position_embeddings=9216)
LLAMAGEN_B = LlamaGenArgs(dim=768, n_layer=12, n_head=12)
