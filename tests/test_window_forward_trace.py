"""CPU: the launch sequence of every window-forward route, call by call, against tests/golden/window_forward_trace.json.

Tiny backbones are packed with the real sjd_amd.ops packers; for the forward `_ops` and `attn` are swapped for a recorder that launches nothing: it
forwards the pure predicates (launch_shapes), answers True where a predicate would ask the device, and returns zero tensors / ops.Partials of the
shapes the real calls return.  Per call it keeps the function name, (layer, projection) of a packed weight, every int / bool / float / tuple
argument and shape + dtype of every tensor; per forward what forward_window returned.  After enable_fused it also keeps what the call left behind
(compress_stats, packed_bytes, the packed types and chunks, the state-dict keys, where the re-pointed parameters alias `_fused`, a SHA-256 of layer
0's packed bytes and of the head's).

The fixture is what this file recorded on the commit BEFORE the window forward and the packing loop were shared between the two backbones
(`python -m tests.test_window_forward_trace --record`, `--record-gpu PATH` on a GPU for the cases that need a device); the recorder reads only names
that commit had, so it can be run there again.  The literal kernel sequences below keep the fixture from being regenerated from a broken tree.

The swin-norm fused gate|up route exists at hidden 8192 only: that one case runs on the meta device with a stand-in MXFP4 packer (shapes only)."""
import dataclasses
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch

import sjd_amd.backbones as BB
import sjd_amd.ops as real_ops
import sjd_amd.synthetic as synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "window_forward_trace.json")
NAMES = ("qkv", "o", "gate_up", "down")
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}


# ------------------------------------------------------------------------------------------ the recorder
def _prows(M):
    return ((int(M) + 31) // 32) * 32


class Recorder:
    """stands in for sjd_amd.ops during a forward"""
    DEVICE_PREDICATES = ("skinny_gemm_reduce_ok", "mlp_pair_ok", "fused_attention_ok")

    def __init__(self, model):
        self.calls = []
        self.names = {}
        for li, d in enumerate(getattr(model, "_packed", None) or []):
            for name, w in d.items():
                self.names[id(w)] = [li, name]
        if getattr(model, "_packed_head", None) is not None:
            self.names[id(model._packed_head)] = ["head", "head"]

    def __getattr__(self, name):          # packers, Packed* / Partials / HeadOut, the predicates launch_shapes answers
        if name in self.DEVICE_PREDICATES:
            return lambda *a, **k: True
        return getattr(real_ops, name)

    def _arg(self, a):
        if id(a) in self.names:
            return ["w"] + self.names[id(a)]
        if isinstance(a, torch.Tensor):
            return ["t", list(a.shape), str(a.dtype).replace("torch.", "")]
        if isinstance(a, real_ops.Partials):
            return ["p", a.n_chunks, a.N, list(a.data.shape)]
        if isinstance(a, (bool, int, float, str)) or a is None:
            return a
        if isinstance(a, (tuple, list)):
            return [self._arg(x) for x in a]
        if isinstance(a, torch.dtype):
            return str(a).replace("torch.", "")
        return type(a).__name__

    def rec(self, fn, *a, **k):
        self.calls.append([fn, [self._arg(x) for x in a], {key: self._arg(v) for key, v in sorted(k.items())}])

    @staticmethod
    def _part(x, nc, rows, N):
        return real_ops.Partials(torch.zeros(nc, rows, N, dtype=torch.float32, device=x.device), nc, N)

    def skinny_gemm(self, x, w, N, K, KC, waves=4, step_major=False):
        self.rec("skinny_gemm", x, w, N, K, KC, waves, step_major)
        return self._part(x, (K + KC - 1) // KC, _prows(x.shape[0]), N)

    def skinny_gemm_cols(self, x, w, N_packed, K, KC, col0, n_cols, waves=8, step_major=True):
        self.rec("skinny_gemm_cols", x, w, N_packed, K, KC, col0, n_cols, waves, step_major)
        return self._part(x, (K + KC - 1) // KC, _prows(x.shape[0]), n_cols)

    def skinny_gemm_reduce(self, x, w, N, K, KC, h, waves=8, step_major=False):
        self.rec("skinny_gemm_reduce", x, w, N, K, KC, h, waves, step_major)
        return torch.zeros(N // 512, 32, dtype=torch.float32, device=x.device)

    def residual_sumsq(self, h, part=None, pull=None, pull_blocks=0):
        self.rec("residual_sumsq", h, part, pull, pull_blocks)
        R = part.data.shape[1] if part is not None else _prows(h.shape[0])
        return torch.zeros((h.shape[1] + 511) // 512, R, dtype=torch.float32, device=h.device)

    def qknorm_rope_append(self, qkv, k_cache, v_cache, qn_w, qn_b, kn_w, kn_b, inv_freq, positions, B, n, H, H_kv, D, params, kv_len, **kw):
        self.rec("qknorm_rope_append", qkv, k_cache, v_cache, qn_w, qn_b, kn_w, kn_b, inv_freq, positions, B, n, H, H_kv, D, params, kv_len, **kw)
        act = kw.get("dtype") or (qkv.dtype if isinstance(qkv, torch.Tensor) else k_cache.dtype)
        return torch.zeros(B, n, H, kw.get("head_pad") or D, dtype=act, device=k_cache.device)

    def qkv_attention_fused(self, qkv_part, k_cache, v_cache, qn_w, qn_b, kn_w, kn_b, inv_freq, positions, B, n, H, D, params, kv_len, key_start, **kw):
        self.rec("qkv_attention_fused", qkv_part, k_cache, v_cache, qn_w, qn_b, kn_w, kn_b, inv_freq, positions, B, n, H, D, params, kv_len, key_start, **kw)
        return torch.zeros(B, n, H, D, dtype=kw.get("dtype") or k_cache.dtype, device=k_cache.device)

    def silu_mul(self, gate_up, rows=None, dtype=None, row_norm=None):
        self.rec("silu_mul", gate_up, rows=rows, dtype=dtype, row_norm=row_norm)
        if isinstance(gate_up, torch.Tensor):
            return torch.zeros(gate_up.shape[0], gate_up.shape[1] // 2, dtype=gate_up.dtype, device=gate_up.device)
        return torch.zeros(rows, gate_up.N // 2, dtype=dtype, device=gate_up.data.device)

    def gateup_silu(self, x, w, inter, hidden, step_major=False, row_norm=None):
        self.rec("gateup_silu", x, w, inter, hidden, step_major, row_norm=row_norm)
        return torch.zeros(x.shape[0], inter, dtype=x.dtype, device=x.device)

    def mlp_pair(self, x, gu, dn, inter, hidden, KC_dn, row_norm=None, ready=None):
        self.rec("mlp_pair", x, gu, dn, inter, hidden, KC_dn, row_norm=row_norm, ready=ready)
        return torch.zeros(x.shape[0], inter, dtype=x.dtype, device=x.device), self._part(x, (inter + KC_dn - 1) // KC_dn, 32, hidden)

    def add_rmsnorm(self, h, delta, weight, eps):
        self.rec("add_rmsnorm", h, delta, weight, eps)
        return torch.zeros_like(h)

    def add_rmsnorm_post(self, h, delta, weight, eps):
        self.rec("add_rmsnorm_post", h, delta, weight, eps)
        return h

    def weight_prefetch(self, w, blocks=128, nbytes=None):
        self.rec("weight_prefetch", w, blocks, nbytes)


class AttnRecorder:
    """stands in for ops.HipWindowAttention"""
    params = None
    n_split = 4

    def __init__(self, rec):
        self._rec = rec

    def attend(self, layer, q, cache, kv_len, key_start, **kw):
        self._rec.rec("attend", layer, q, kv_len, key_start, **kw)
        return torch.zeros_like(q)

    def _resolve_split(self, B, Hkv, n_rows=16, H=None, cache_bytes_per_head=None):
        return self.n_split

    def _workspace(self, B, H, n, D, device):
        return torch.zeros(8, dtype=torch.float32, device=device)

    def __call__(self, layer, q, k, v, cache, kv_len, key_start):          # forward_embeds (no kernel of the window path)
        return torch.zeros_like(q)


# ------------------------------------------------------------------------------------------ the backbones
TOY = dict(vocab_size=1000, hidden_size=512, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
           max_position_embeddings=256)
TOY_CFG = dict(qkv=(256, 4, True), o=(128, 3, False), gate_up=(256, 8, True), down=(128, 2, False))
# the quantised streams: down reads K = 2560 in ONE chunk up to 32 rows and in halved chunks (1280) at 33..64; tile counts the wide kernels take
TOY_Q = dict(TOY, intermediate_size=2560)
TOY_Q_CFG = dict(qkv=(256, 4, True), o=(128, 3, False), gate_up=(256, 8, True), down=(2560, 4, True))
LG = dict(dim=512, n_layer=2, n_head=8, vocab_size=1000, block_size=64)
LG_FUSED_CFG = dict(qkv=(256, 2, True), o=(256, 2, False), gate_up=(256, 2, True), down=(512, 2, False))          # gate|up in two K halves: G1s
LG_100 = dict(dim=800, n_layer=1, n_head=8, vocab_size=1000, block_size=64)
# shapes only (meta weights, stand-in packers): the widths at which G1s is served above 32 rows (LS.gateup_silu_ok: 33..64 rows at hidden >= 1024, 65..128
# at hidden 4096 over the uncompressed packing) and the swin-norm K = 8192 form -- what separates Chameleon's 64-row cap from `gateup_fused = "tall"` and from
# LlamaGen, which has no cap
META_30B = dataclasses.replace(BB.CHAMELEON_30B, num_hidden_layers=1, intermediate_size=128, vocab_size=1024)
META_7B = dataclasses.replace(BB.LUMINA_7B, num_hidden_layers=1, intermediate_size=128, vocab_size=1024)
META_LG = dict(dim=4096, n_layer=1, n_head=32, vocab_size=1024, block_size=64)
META_LG_CFG = dict(qkv=(2048, 4, True), o=(1024, 4, True), gate_up=(2048, 4, True), down=(1408, 4, True))

# key -> (family, args, dtype, G1_CFG or None, enable_fused keywords)
MODELS = {
    "cham_z": ("cham", TOY, "bf16", TOY_CFG, dict(gemm="sjd", compress=True)),
    "cham_raw": ("cham", TOY, "bf16", TOY_CFG, dict(gemm="sjd", compress=False)),
    "cham_nofold": ("cham", TOY, "bf16", TOY_CFG, dict(gemm="sjd", compress=False, fold_norm=False)),
    "cham_swin": ("cham", dict(TOY, swin_norm=True, model_parallel_size=2), "bf16", TOY_CFG, dict(gemm="sjd", compress=True)),
    "cham_swin_mxfp4": ("cham", dict(TOY, swin_norm=True, model_parallel_size=2), "bf16", TOY_CFG, dict(gemm="sjd", weights="mxfp4", swin_quant=True)),
    "cham_swin_mxfp4_8192": ("meta_cham", META_30B, "bf16", None, dict(gemm="sjd", weights="mxfp4", swin_quant=True)),
    "cham_4096_raw": ("meta_cham", META_7B, "bf16", None, dict(gemm="sjd", compress=False)),
    "cham_4096_z": ("meta_cham", META_7B, "bf16", None, dict(gemm="sjd", compress=True)),
    "lg_4096": ("meta_lg", META_LG, "bf16", META_LG_CFG, dict(gemm="sjd", max_rows=128)),
    "cham_e4m3": ("cham", TOY_Q, "bf16", TOY_Q_CFG, dict(gemm="sjd", weights="e4m3")),
    "cham_e4m3_twin": ("cham", TOY_Q, "bf16", TOY_Q_CFG, dict(gemm="sjd", weights="e4m3_as_bf16")),
    "cham_e4m3_128": ("cham", TOY_Q, "bf16", TOY_Q_CFG, dict(gemm="sjd", weights="e4m3", max_rows=128)),
    "cham_mxfp4": ("cham", TOY_Q, "bf16", TOY_Q_CFG, dict(gemm="sjd", weights="mxfp4")),
    "cham_torch": ("cham", TOY, "bf16", TOY_CFG, dict(gemm="torch")),
    "lg_bf16": ("lg", LG, "bf16", None, dict(gemm="sjd")),
    "lg_fp16": ("lg", LG, "fp16", LG_FUSED_CFG, dict(gemm="sjd")),
    "lg_100": ("lg", LG_100, "bf16", None, dict(gemm="sjd", pad_head_dim=True)),
    "lg_128": ("lg", LG, "bf16", None, dict(gemm="sjd", max_rows=128)),
    "lg_e4m3": ("lg", LG, "bf16", None, dict(gemm="sjd", weights="e4m3")),
    "lg_mxfp4": ("lg", LG, "bf16", LG_FUSED_CFG, dict(gemm="sjd", weights="mxfp4")),
    "lg_e4m3_128": ("lg", LG, "bf16", None, dict(gemm="sjd", weights="e4m3", max_rows=128)),
}


class _MetaQ4(real_ops.PackedQ4):
    def __init__(self, w, KC, sm):
        super().__init__(None, w.shape[0], w.shape[1], KC, sm, dict(rel_rms_error=0.0))

    def nbytes(self):
        return self.N * self.K * 17 // 32


class _MetaZ(real_ops.PackedZ):
    def __init__(self, w, KC, sm):
        self.N, self.K, self.KC, self.step_major, self.n_exceptions, self.stats, self.n_raw = w.shape[0], w.shape[1], KC, bool(sm), 0, {}, 0

    def nbytes(self):
        return self.N * self.K * 3 // 2


class _MetaOps:
    """sjd_amd.ops with shapes-only packers (meta weights have no values to quantise or compress)"""
    def __getattr__(self, name):
        return getattr(real_ops, name)

    @staticmethod
    def pack_weight_z(w, KC, step_major=False, gateup=False):
        return _MetaZ(w, KC, step_major)

    @staticmethod
    def pack_weight_q4(w, KC, step_major=False, gateup=False):
        return _MetaQ4(w, KC, step_major)

    @staticmethod
    def pack_weight(w, KC, step_major=False):
        return torch.empty_like(w)


_BUILT = {}


def build(key, device="cpu"):
    """the packed backbone of MODELS[key] (built once per device: a traced forward changes nothing in it)"""
    if (key, device) in _BUILT:
        return _BUILT[key, device]
    family, args, dtype, cfg, kw = MODELS[key]
    if family.startswith("meta"):
        with torch.device("meta"):
            m = (BB.ChameleonBackbone(args) if family == "meta_cham" else BB.LlamaGenBackbone(BB.LlamaGenArgs(**args))).to(DT[dtype])
        if cfg is not None:
            m.G1_CFG = dict(cfg)
        m.enable_fused(_MetaOps(), **kw)
        _BUILT[key, device] = m
        return m
    if family == "cham":
        m = BB.ChameleonBackbone(BB.ChameleonArgs(qk_norm=True, **args)).eval()
        norms = [n for layer in m.model.layers for n in (layer.input_layernorm, layer.post_attention_layernorm)] + [m.model.norm]
    else:
        m = BB.LlamaGenBackbone(BB.LlamaGenArgs(**args)).eval()
        norms = [n for layer in m.layers for n in (layer.attention_norm, layer.ffn_norm)] + [m.norm]
    synthetic.fill_state_dict(m, seed=3, embed_token_scale=0.25)
    g = torch.Generator().manual_seed(1)
    for nrm in norms:          # gains far from one: a gain folded twice, or not at all, shows in the packed bytes
        nrm.weight.data = 1.0 + 0.5 * torch.randn(nrm.weight.shape[0], generator=g)
    m = m.to(device=device, dtype=DT[dtype])
    if cfg is not None:
        m.G1_CFG = dict(cfg)
    m.enable_fused(real_ops, **kw)
    _BUILT[key, device] = m
    return m


def _sha(w):
    t = w if isinstance(w, torch.Tensor) else w.data
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def _kind(w):
    if w is None:
        return None
    if isinstance(w, torch.Tensor):
        return ["Tensor", str(w.dtype).replace("torch.", ""), list(w.shape)]
    return [type(w).__name__.lstrip("_").replace("Meta", "Packed"), w.N, w.K, w.KC, bool(w.step_major)]


def state_of(key):
    """what enable_fused left behind"""
    m = build(key)
    meta = MODELS[key][0].startswith("meta")
    layers = m.model.layers if hasattr(m, "model") else m.layers
    alias = []
    for li, layer in enumerate(layers):
        fused = m._fused[li] if isinstance(m._fused[li], tuple) else (m._fused[li],)
        if hasattr(m, "model"):
            a, f = layer.self_attn, layer.mlp
            params = dict(q_proj=a.q_proj, k_proj=a.k_proj, v_proj=a.v_proj, gate_proj=f.gate_proj, up_proj=f.up_proj)
        else:
            params = dict(w1=layer.feed_forward.w1, w3=layer.feed_forward.w3)
        for name, lin in params.items():
            hit = [[fi, lin.weight.data_ptr() - t.data_ptr()] for fi, t in enumerate(fused)
                   if 0 <= lin.weight.data_ptr() - t.data_ptr() < max(1, t.numel() * t.element_size())]
            alias.append([li, name, "meta" if meta else hit, list(lin.weight.shape)])
    return dict(compress_stats=m.compress_stats, packed_bytes=m.packed_bytes(),
                fused=[[type(f).__name__] + [list(t.shape) for t in (f if isinstance(f, tuple) else (f,))] for f in m._fused],
                packed=[{n: _kind(d[n]) for n in NAMES} for d in m._packed], head=_kind(m._packed_head), head_cols=getattr(m, "_head_cols", None),
                g1_cfg={n: list(m.G1_CFG[n]) for n in NAMES}, head_cfg=list(m.HEAD_CFG), max_rows=getattr(m, "max_rows", None),
                max_rows_given=m._max_rows_given, weights=m.weights, fold_norm=getattr(m, "_fold_norm", None), fused_rows=getattr(m, "_fused_rows", None),
                head_pad=getattr(m, "_head_pad", None), state_dict=sorted(m.state_dict().keys()), alias=alias,
                sha256=None if meta else dict({n: _sha(m._packed[0][n]) for n in NAMES if m._packed}, head=_sha(m._packed_head) if m._packed_head is not None else None))


# ------------------------------------------------------------------------------------------ the cases
W32, W64, W128, W256, PREFILL = (2, 16), (4, 16), (8, 16), (8, 32), (1, 288)

# name -> (model, (B, n), forward keywords, instance attributes set for this forward)
CASES = {}
for _z in ("cham_z", "cham_raw"):
    for _w in (W32, W64, W128):
        for _hp in (True, False):
            CASES[f"{_z} {_w[0] * _w[1]} rows head_partials={_hp}"] = (_z, _w, dict(head_partials=_hp), {})
    CASES[f"{_z} 32 rows cols narrow head_partials"] = (_z, W32, dict(head_partials=True, cols=(100, 400)), {})
    CASES[f"{_z} 32 rows cols narrow logits"] = (_z, W32, dict(cols=(100, 400)), {})
CASES.update({
    "cham_nofold 32 rows": ("cham_nofold", W32, dict(head_partials=True), {}),
    "cham_nofold 64 rows cols": ("cham_nofold", W64, dict(cols=(100, 400)), {}),
    "cham_swin 32 rows": ("cham_swin", W32, dict(head_partials=True), {}),
    "cham_swin 128 rows": ("cham_swin", W128, {}, {}),
    "cham_swin prefill": ("cham_swin", PREFILL, {}, {}),
    "cham_swin_mxfp4 32 rows gateup_fused=False": ("cham_swin_mxfp4", W32, {}, dict(gateup_fused=False)),
    "cham_swin_mxfp4 32 rows gateup_fused=True": ("cham_swin_mxfp4", W32, {}, dict(gateup_fused=True)),
    "cham_swin_mxfp4 64 rows gateup_fused=True": ("cham_swin_mxfp4", W64, {}, dict(gateup_fused=True)),
    "cham_swin_mxfp4_8192 32 rows gateup_fused=False": ("cham_swin_mxfp4_8192", W32, {}, dict(gateup_fused=False)),
    "cham_swin_mxfp4_8192 32 rows gateup_fused=True": ("cham_swin_mxfp4_8192", W32, {}, dict(gateup_fused=True)),
    "cham_swin_mxfp4_8192 64 rows gateup_fused=True": ("cham_swin_mxfp4_8192", W64, {}, dict(gateup_fused=True)),
    "cham_4096_raw 64 rows": ("cham_4096_raw", W64, dict(head_partials=True), {}),
    "cham_4096_raw 128 rows": ("cham_4096_raw", W128, dict(head_partials=True), {}),
    "cham_4096_raw 128 rows gateup_fused=False": ("cham_4096_raw", W128, dict(head_partials=True), dict(gateup_fused=False)),
    "cham_4096_raw 64 rows gateup_fused=False": ("cham_4096_raw", W64, dict(head_partials=True), dict(gateup_fused=False)),
    "cham_4096_z 64 rows": ("cham_4096_z", W64, dict(head_partials=True), {}),
    "cham_4096_z 128 rows": ("cham_4096_z", W128, dict(head_partials=True), {}),
    "lg_4096 64 rows": ("lg_4096", W64, dict(head_partials=True), {}),
    "lg_4096 128 rows": ("lg_4096", W128, dict(head_partials=True), {}),
    "cham_e4m3 32 rows": ("cham_e4m3", W32, dict(head_partials=True), {}),
    "cham_e4m3 64 rows": ("cham_e4m3", W64, dict(head_partials=True), {}),
    "cham_e4m3_twin 32 rows": ("cham_e4m3_twin", W32, dict(head_partials=True), {}),
    "cham_e4m3_twin 64 rows": ("cham_e4m3_twin", W64, dict(head_partials=True), {}),
    "cham_e4m3_128 128 rows": ("cham_e4m3_128", W128, dict(head_partials=True), {}),
    "cham_mxfp4 32 rows": ("cham_mxfp4", W32, dict(head_partials=True), {}),
    "cham_torch 32 rows": ("cham_torch", W32, dict(head_partials=True), {}),
    "cham_z prefill": ("cham_z", PREFILL, dict(head_partials=True, cols=(100, 400)), {}),
    "refusal mxfp4 128 rows": ("cham_mxfp4", W128, {}, {}),
    "refusal e4m3 max_rows=128 256 rows": ("cham_e4m3_128", W256, {}, {}),
    "refusal e4m3 128 rows": ("cham_e4m3", W128, {}, {}),
    "lg_bf16 32 rows": ("lg_bf16", W32, dict(head_partials=True), {}),
    "lg_bf16 64 rows logits cols": ("lg_bf16", W64, dict(cols=(100, 400)), {}),
    "lg_bf16 128 rows (forward_embeds)": ("lg_bf16", W128, dict(head_partials=True), {}),
    "lg_fp16 32 rows": ("lg_fp16", W32, dict(head_partials=True), {}),
    "lg_fp16 64 rows": ("lg_fp16", W64, dict(head_partials=True), {}),
    "lg_100 32 rows": ("lg_100", W32, dict(head_partials=True), {}),
    "lg_100 64 rows logits": ("lg_100", W64, {}, {}),
    "lg_128 128 rows": ("lg_128", W128, dict(head_partials=True), {}),
    "lg_e4m3 32 rows": ("lg_e4m3", W32, dict(head_partials=True), {}),
    "lg_e4m3 64 rows": ("lg_e4m3", W64, dict(head_partials=True), {}),
    "lg_mxfp4 32 rows": ("lg_mxfp4", W32, dict(head_partials=True), {}),
    "lg_mxfp4 64 rows": ("lg_mxfp4", W64, dict(head_partials=True), {}),
    "lg_e4m3_128 128 rows": ("lg_e4m3_128", W128, dict(head_partials=True), {}),
    # the experiments, each switched on as an instance attribute (K1F and the pair want a device: on the CPU they take the product's kernels)
    "exp k1_fused split (cpu)": ("cham_z", W32, dict(head_partials=True), dict(k1_fused=True, k1_fused_split=True)),
    "exp k1_fused one workgroup (cpu)": ("cham_z", W32, dict(head_partials=True), dict(k1_fused=True, k1_fused_split=False)),
    "exp reduce_fused": ("cham_raw", W32, dict(head_partials=True), dict(reduce_fused=True)),
    "exp reduce_fused logits": ("cham_raw", W32, {}, dict(reduce_fused=True)),
    "exp reduce_fused 12-bit (not served)": ("cham_z", W32, dict(head_partials=True), dict(reduce_fused=True)),
    "exp mlp_pair (cpu)": ("cham_z", W32, dict(head_partials=True), dict(mlp_pair=True)),
    "exp gateup_fused=False": ("cham_z", W32, dict(head_partials=True), dict(gateup_fused=False)),
    "exp gateup_fused=tall hidden 512 128 rows (not served)": ("cham_raw", W128, dict(head_partials=True), dict(gateup_fused="tall")),
    "exp gateup_fused=tall 4096 raw 128 rows": ("cham_4096_raw", W128, dict(head_partials=True), dict(gateup_fused="tall")),
    "exp gateup_fused=tall 4096 raw 64 rows": ("cham_4096_raw", W64, dict(head_partials=True), dict(gateup_fused="tall")),
    "exp gateup_fused=tall 4096 12-bit 128 rows (not served)": ("cham_4096_z", W128, dict(head_partials=True), dict(gateup_fused="tall")),
    "exp gateup_fused=tall 32 rows": ("cham_z", W32, dict(head_partials=True), dict(gateup_fused="tall")),
})
PLAN = dict(o=(128, "after"), gate_up=(64, "g1"))
GPU_CASES = {
    "gpu prefetch plan": ("cham_z", W32, dict(head_partials=True), dict(PREFETCH=dict(BB.ChameleonBackbone.PREFETCH, **PLAN))),
    "gpu prefetch plan logits": ("cham_raw", W32, {}, dict(PREFETCH=dict(BB.ChameleonBackbone.PREFETCH, **PLAN), reduce_fused=True, mlp_pair=True)),
    "gpu k1_fused split": ("cham_z", W32, dict(head_partials=True), dict(k1_fused=True, k1_fused_split=True)),
    "gpu k1_fused one workgroup": ("cham_z", W32, dict(head_partials=True), dict(k1_fused=True, k1_fused_split=False)),
    "gpu mlp_pair": ("cham_z", W32, dict(head_partials=True), dict(mlp_pair=True)),
    "gpu mlp_pair with reduce_fused": ("cham_raw", W32, dict(head_partials=True), dict(mlp_pair=True, reduce_fused=True)),
    "gpu product": ("cham_z", W32, dict(head_partials=True), {}),
}
_SCRATCH = ("_pf_plan", "_pf_on", "_pf_stream", "_pair_ready")          # what a forward with a switch set may leave on the instance


def trace(case, device="cpu"):
    """-> dict(calls, out, gateup_route) of one forward_window, or dict(calls, error) where it refuses"""
    key, (B, n), kw, attrs = (GPU_CASES if case in GPU_CASES else CASES)[case]
    m = build(key, device)
    dev = "meta" if MODELS[key][0].startswith("meta") else device
    rec = Recorder(m)
    real, attn, cache = m._ops, m.attn, m.cache
    before = {k: m.__dict__[k] for k in list(attrs) + list(_SCRATCH) if k in m.__dict__}
    for k in _SCRATCH:
        m.__dict__.pop(k, None)
    m.__dict__.update(attrs)
    m._ops, m.attn = rec, AttnRecorder(rec)
    if hasattr(m, "gateup_route"):
        m.gateup_route = {}
    try:
        with torch.device(dev):
            m.setup_cache(B, 64)
            tokens = torch.zeros(B, n, dtype=torch.long)
            positions = torch.arange(n).repeat(B, 1)
            key_start = torch.zeros(B, dtype=torch.int32)
        try:
            out = m.forward_window(tokens, positions, 0, key_start, **kw)
        except ValueError as e:
            return dict(calls=rec.calls, error=str(e))
        if isinstance(out, real_ops.HeadOut):
            o = dict(type="HeadOut", part=rec._arg(out.part), col0=out.col0, urow_off=out.urow_off, dtype=rec._arg(out.dtype), row_norm=rec._arg(out.row_norm))
        else:
            o = dict(type="Tensor", shape=list(out.shape), dtype=rec._arg(out.dtype))
        return dict(calls=rec.calls, out=o, gateup_route={str(k): v for k, v in getattr(m, "gateup_route", {}).items()})
    finally:
        m._ops, m.attn, m.cache = real, attn, cache
        for k in list(attrs) + list(_SCRATCH):
            m.__dict__.pop(k, None)
        m.__dict__.update(before)


def _json(x):
    return json.loads(json.dumps(x))


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _names(case, device="cpu"):
    return [c[0] for c in trace(case, device)["calls"]]


# ------------------------------------------------------------------------------------------ A: the traces
@pytest.mark.parametrize("case", list(CASES))
def test_forward_trace(case):
    assert _json(trace(case)) == _golden()["traces"][case]


@pytest.mark.gpu
def test_forward_trace_on_a_device():
    """the cases that want a device (a side stream for the prefetch plan, an int32 key_start on it for K1F, the pair): the same stubbed ops, no launch"""
    for case in GPU_CASES:
        assert _json(trace(case, "cuda")) == _golden()["gpu_traces"][case], case
    # o's weights behind q|k|v's G1 ("after"), gate|up's from the launch of o's G1 ("g1"); prefetch on: G1 + F3, no fused gate|up
    layer = ["residual_sumsq", "skinny_gemm", "weight_prefetch", "qknorm_rope_append", "attend", "weight_prefetch", "skinny_gemm", "residual_sumsq"] + G1_F3
    assert _names("gpu prefetch plan", "cuda") == layer * 2 + HEAD
    assert _names("gpu k1_fused split", "cuda") == (["residual_sumsq", "skinny_gemm", "qkv_attention_fused", "skinny_gemm", "residual_sumsq"] + G1S) * 2 + HEAD
    assert _names("gpu mlp_pair", "cuda") == (FOLDED + ["mlp_pair"]) * 2 + HEAD


FOLDED = ["residual_sumsq", "skinny_gemm", "qknorm_rope_append", "attend", "skinny_gemm", "residual_sumsq"]          # F1r, G1 q|k|v, F2, K1, G1 o, F1r
G1S, G1_F3 = ["gateup_silu", "skinny_gemm"], ["skinny_gemm", "silu_mul", "skinny_gemm"]          # ... G1s | G1 + F3, then G1 down
HEAD, LOGITS = ["residual_sumsq", "skinny_gemm_cols"], ["add_rmsnorm"]
SWIN = ["skinny_gemm", "qknorm_rope_append", "attend", "skinny_gemm", "add_rmsnorm_post"]          # G1 q|k|v on h itself, F2, K1, G1 o, F1 (post-norm)
PRE = ["add_rmsnorm", "skinny_gemm", "qknorm_rope_append", "attend", "skinny_gemm", "add_rmsnorm"]


def test_kernel_sequences():
    assert _names("cham_z 32 rows head_partials=True") == (FOLDED + G1S) * 2 + HEAD
    assert _names("cham_z 128 rows head_partials=False") == (FOLDED + G1_F3) * 2 + LOGITS          # (the 12-bit G1s ends at 64 rows)
    assert _names("lg_fp16 32 rows") == (FOLDED + G1S) * 2 + HEAD
    assert _names("lg_bf16 32 rows") == (FOLDED + G1_F3) * 2 + HEAD          # (gate|up packed in chunks of 320: no two K halves)
    assert _names("lg_mxfp4 32 rows") == (FOLDED + G1S) * 2 + HEAD and _names("lg_mxfp4 64 rows") == (FOLDED + G1_F3) * 2 + HEAD
    assert _names("lg_bf16 128 rows (forward_embeds)") == []
    # G1s above 32 rows: Chameleon up to 64 rows, beyond only with `gateup_fused = "tall"` (hidden 4096, uncompressed); LlamaGen wherever the kernel serves
    assert _names("cham_4096_raw 64 rows") == FOLDED + G1S + HEAD == _names("cham_4096_z 64 rows")
    assert _names("cham_4096_raw 128 rows") == FOLDED + G1_F3 + HEAD == _names("cham_4096_z 128 rows")
    assert _names("exp gateup_fused=tall 4096 raw 128 rows") == FOLDED + G1S + HEAD == _names("exp gateup_fused=tall 4096 raw 64 rows")
    assert _names("exp gateup_fused=tall 4096 12-bit 128 rows (not served)") == FOLDED + G1_F3 + HEAD
    assert _names("cham_4096_raw 64 rows gateup_fused=False") == FOLDED + G1_F3 + HEAD == _names("cham_4096_raw 128 rows gateup_fused=False")
    assert _names("lg_4096 64 rows") == FOLDED + G1S + HEAD == _names("lg_4096 128 rows")
    assert _names("cham_swin 32 rows") == (SWIN + G1_F3 + ["add_rmsnorm_post"]) * 2 + LOGITS
    assert _names("cham_swin_mxfp4_8192 32 rows gateup_fused=True") == SWIN + G1S + ["add_rmsnorm_post"] + LOGITS
    assert _names("cham_swin_mxfp4_8192 32 rows gateup_fused=False") == SWIN + G1_F3 + ["add_rmsnorm_post"] + LOGITS
    assert _names("cham_nofold 32 rows") == (PRE + G1_F3) * 2 + LOGITS
    assert _names("cham_torch 32 rows") == (["add_rmsnorm", "qknorm_rope_append", "attend", "add_rmsnorm", "silu_mul"]) * 2 + LOGITS
    assert _names("exp reduce_fused") == (["residual_sumsq", "skinny_gemm", "qknorm_rope_append", "attend", "skinny_gemm_reduce", "gateup_silu", "skinny_gemm_reduce"]
                                          + ["skinny_gemm", "qknorm_rope_append", "attend", "skinny_gemm_reduce", "gateup_silu", "skinny_gemm_reduce"] + ["skinny_gemm_cols"])


def test_routes_show_in_the_traces():
    t = trace("cham_swin_mxfp4_8192 32 rows gateup_fused=True")
    assert t["gateup_route"] == {"32": "fused"} and trace("cham_swin_mxfp4_8192 64 rows gateup_fused=True")["gateup_route"] == {"64": "g1+f3"}
    assert trace("cham_swin_mxfp4_8192 32 rows gateup_fused=False")["gateup_route"] == {"32": "g1+f3"}
    assert trace("cham_swin_mxfp4 32 rows gateup_fused=True")["gateup_route"] == {"32": "g1+f3"}          # (hidden 512: no K = 8192 form)
    down = lambda case: [c[1][4] for c in trace(case)["calls"] if c[0] == "skinny_gemm" and c[1][1][2:] == ["down"]]
    assert down("cham_e4m3 32 rows") == [2560, 2560] and down("cham_e4m3 64 rows") == [1280, 1280] == down("cham_e4m3_twin 64 rows")          # the halved chunk
    assert down("cham_e4m3_128 128 rows") == [2560, 2560]
    assert trace("refusal mxfp4 128 rows") == dict(calls=[], error="weights='mxfp4' serves draft windows of at most 64 rows (kernels G1q4 / G1sq4 have no wide form); got 128 rows")
    assert trace("refusal e4m3 max_rows=128 256 rows") == dict(calls=[], error="weights='e4m3' serves draft windows of at most 128 rows (max_rows=128); got 256 rows")
    assert trace("refusal e4m3 128 rows") == dict(calls=[], error="weights='e4m3' serves draft windows of at most 64 rows (one prompt per forward); got 128 rows")
    assert trace("cham_z prefill")["out"] == dict(type="Tensor", shape=[1, 288, 300], dtype="float32")
    assert trace("lg_100 32 rows")["out"]["type"] == "HeadOut"


# ------------------------------------------------------------------------------------------ B: the product path does not load the experiments
_PRODUCT_ONLY = """
import sys, torch
import tests.test_window_forward_trace as T
import sjd_amd._lib as L
for case in ("cham_z 32 rows head_partials=True", "cham_raw 128 rows head_partials=False", "cham_swin 32 rows", "lg_bf16 32 rows", "lg_mxfp4 32 rows"):
    assert T.trace(case)["calls"], case
exp = [n for n in sys.modules if n.endswith("backbones_exp")]
assert not exp, exp
assert L._exp is None
print("product only")
"""


def test_default_switches_never_load_the_experiments():
    env = {k: v for k, v in os.environ.items() if not k.startswith("SJD_")}
    r = subprocess.run([sys.executable, "-c", _PRODUCT_ONLY], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "product only" in r.stdout, r.stdout + r.stderr


# ------------------------------------------------------------------------------------------ C: what enable_fused leaves behind
@pytest.mark.parametrize("key", list(MODELS))
def test_enable_fused_state(key):
    got, want = _json(state_of(key)), _golden()["state"][key]
    for stats in (got["compress_stats"], want["compress_stats"]):          # (a float the CPU's reduction order may move in its last bits)
        if "rel_rms_error" in stats:
            stats["rel_rms_error"] = round(stats["rel_rms_error"], 6)
    assert got == want


if __name__ == "__main__":
    if "--record-gpu" in sys.argv:
        path = os.path.abspath(sys.argv[sys.argv.index("--record-gpu") + 1])          # (then: --record --gpu-from PATH)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump({case: trace(case, "cuda") for case in GPU_CASES}, f, indent=0, sort_keys=True)
        print("wrote", path)
    elif "--record" in sys.argv:
        old = _golden() if os.path.exists(GOLDEN) else {}
        doc = dict(traces={case: trace(case) for case in CASES}, state={key: state_of(key) for key in MODELS}, gpu_traces=old.get("gpu_traces", {}))
        if "--gpu-from" in sys.argv:
            with open(sys.argv[sys.argv.index("--gpu-from") + 1]) as f:
                doc["gpu_traces"] = json.load(f)
        with open(GOLDEN, "w") as f:
            json.dump(doc, f, separators=(",", ":"), sort_keys=True)
        print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
