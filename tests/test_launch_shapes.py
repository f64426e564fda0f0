"""CPU: what enable_fused chooses, packs and refuses, and which row counts the window path and SJDBatchEngine then serve -- pinned as literals.

The expected values below were recorded from the code BEFORE the launch-shape rule was gathered into one module; they say what that rule is, so
whoever changes a set, a limit or a refusal text changes a literal here knowingly.  Chameleon-family backbones are built on the meta device at
the real Lumina-7B / Emu3-8B / Chameleon-30B sizes (one layer): the choice and the chunk arithmetic need shapes, not values, and the two packers
that look at values are replaced by stand-ins that keep their `None` rule (pack_weight_z declines fp16 and KC > 4096).  The LlamaGen backbones
(head_dim 64, and head_dim 100 stored 128 wide) are tiny and really packed.  LlamaGen's enable_fused has no `compress`; its axes are
dtype x max_rows x untuned_fp16 (x padded_batch at head_dim 100), and `weights`.

The tables written later -- MXFP4 and swin_quant on the Chameleon families, LlamaGen's `weights`, and the refusals of a quantised copy by reason and call
site -- were recorded the same way from the code before ITS five copies of the quantised-copy rule became one (LS.quant_copy_errors)."""
import dataclasses
import types

import pytest
import torch

import sjd_amd.backbones as BB
import sjd_amd.ops as real_ops
from sjd_amd.engine_batch import SJDBatchEngine

NAMES = ("qkv", "o", "gate_up", "down")
ROWS = (32, 33, 64, 65, 96, 97, 128, 129, 256)
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
MAX_ROWS = (None, 64, 128, 256)


class _Z(real_ops.PackedZ):
    def __init__(self, w, KC, sm):
        self.N, self.K, self.KC, self.step_major, self.n_exceptions, self.stats = w.shape[0], w.shape[1], KC, bool(sm), 0, {}
        self.n_raw = 0

    def nbytes(self):
        return self.N * self.K * 3 // 2


class _Q8(real_ops.PackedQ8):
    def __init__(self, w, KC, sm):
        super().__init__(None, w.shape[0], w.shape[1], KC, sm, dict(rel_rms_error=0.0))
        self._w = w

    def nbytes(self):
        return self.N * self.K + 4 * self.N

    def dequant(self):
        return self._w


class _Q4(real_ops.PackedQ4):
    def __init__(self, w, KC, sm):
        super().__init__(None, w.shape[0], w.shape[1], KC, sm, dict(rel_rms_error=0.0))
        self._w = w

    def nbytes(self):
        return self.N * self.K * 17 // 32

    def dequant(self):
        return self._w


class _Prefill(Exception):
    pass


class _Ops:
    """sjd_amd.ops with the two value-dependent packers replaced for meta weights, and the first kernel of the prefill path made a signal"""
    PackedZ, PackedQ8, PackedQ4 = real_ops.PackedZ, real_ops.PackedQ8, real_ops.PackedQ4

    def __getattr__(self, name):
        return getattr(real_ops, name)

    @staticmethod
    def pack_weight_z(w, KC, step_major=False, gateup=False):
        return None if w.dtype != torch.bfloat16 or KC > 4096 else _Z(w, KC, step_major)

    @staticmethod
    def pack_weight_q8(w, KC, step_major=False, gateup=False):
        if w.dtype != torch.bfloat16:
            raise ValueError("quantize_e4m3: bf16 weights only")
        return _Q8(w, KC, step_major)

    @staticmethod
    def pack_weight_q4(w, KC, step_major=False, gateup=False):
        if w.dtype != torch.bfloat16:
            raise ValueError("quantize_mxfp4: bf16 weights only")
        if w.shape[1] % 128 or KC < 128 or KC % 128:          # (the real packer's rule, and its text)
            raise ValueError(f"pack_weight_q4: K and KC must be multiples of 128 (whole records and scale dwords); got K = {tuple(w.shape)[-1]}, KC = {KC}")
        return _Q4(w, KC, step_major)

    @staticmethod
    def add_rmsnorm(*a, **k):
        raise _Prefill

    qknorm_rope_append = add_rmsnorm          # (a swin-norm layer's first kernel)


OPS = _Ops()
CHAMELEON = {"lumina7b": BB.LUMINA_7B, "emu3_8b": BB.EMU3_8B, "chameleon30b": BB.CHAMELEON_30B}


def _chameleon(family, dtype):
    with torch.device("meta"):
        return BB.ChameleonBackbone(dataclasses.replace(CHAMELEON[family], num_hidden_layers=1)).to(DTYPES[dtype])


def _kind(w):
    return type(w).__name__.lstrip("_") if not isinstance(w, torch.Tensor) else str(w.dtype).replace("torch.", "")


def _dims(m):
    H, Hkv, D, hid, inter = m.n_heads, m.n_kv_heads, m.head_dim, m.args.hidden_size, m.args.intermediate_size
    return dict(qkv=hid, o=H * D, gate_up=hid, down=inter)


def _chunks(m):
    """{name: the nine _q8_chunk values}, a ValueError as its text"""
    out = {}
    for name, K in _dims(m).items():
        row = []
        for T in ROWS:
            try:
                row.append(m._q8_chunk(name, T, K))
            except ValueError as e:
                row.append(str(e))
        out[name] = tuple(row)
    return out


def observe_chameleon(family, dtype, compress, weights, max_rows, swin_quant=False, g1_cfg=None, head_cfg=None):
    m = _chameleon(family, dtype)
    given = {k: v for k, v in (("G1_CFG", g1_cfg), ("HEAD_CFG", head_cfg)) if v is not None}
    m.__dict__.update(given)
    try:
        m.enable_fused(OPS, gemm="sjd", compress=compress, weights=weights, max_rows=max_rows, swin_quant=swin_quant)
    except ValueError as e:
        assert "_packed" not in m.__dict__ and "weights" not in m.__dict__ and m.__dict__.get("G1_CFG") == g1_cfg       # a refused call leaves the backbone as it was
        assert m.__dict__.get("HEAD_CFG") == head_cfg and "max_rows" not in m.__dict__
        return str(e)
    return dict(g1=tuple(m.G1_CFG[k] for k in NAMES), head=tuple(m.HEAD_CFG), max_rows=m.__dict__.get("max_rows"), given=m._max_rows_given,
                qkv=_kind(m._packed[0]["qkv"]), head_kind=_kind(m._packed_head), chunks=_chunks(m))


TINY_LG = {"llamagen64": dict(dim=128, n_layer=1, n_head=2, vocab_size=1024, block_size=64),
           "llamagen100": dict(dim=800, n_layer=1, n_head=8, vocab_size=1024, block_size=64),
           "gpt_xxl": dict(dim=1536, n_layer=1, n_head=24)}          # the real widths (K = 1536, 4096 for the down projection), for refusals only
META_LG = ("gpt_xxl",)


def observe_llamagen(family, dtype, max_rows, untuned_fp16, padded_batch, weights=None, g1_cfg=None, head_cfg=None):
    """weights / g1_cfg / head_cfg given: the outcome also names compress_stats' keys (a quantised copy adds its own)"""
    torch.manual_seed(0)
    with torch.device("meta" if family in META_LG else "cpu"):
        m = BB.LlamaGenBackbone(BB.LlamaGenArgs(**TINY_LG[family])).to(DTYPES[dtype])
    kw = {} if max_rows is None else dict(max_rows=max_rows)
    if family == "llamagen100":
        kw.update(pad_head_dim=True, padded_batch=padded_batch)
    if weights is not None:
        kw.update(weights=weights)
    given = {k: v for k, v in (("G1_CFG", g1_cfg), ("HEAD_CFG", head_cfg)) if v is not None}
    m.__dict__.update(given)
    try:
        m.enable_fused(real_ops, gemm="sjd", untuned_fp16=untuned_fp16, **kw)
    except ValueError as e:
        assert all(k not in m.__dict__ for k in ("_packed", "_ops", "weights", "max_rows")) and {k: m.__dict__.get(k) for k in given} == given
        return str(e)
    out = dict(g1=tuple(m.G1_CFG[k] for k in NAMES), head=tuple(m.HEAD_CFG), max_rows=m.max_rows, fused_rows=m._fused_rows,
               qkv=_kind(m._packed[0]["qkv"]), head_kind=_kind(m._packed_head), head_pad=m._head_pad)
    if weights is not None or given:
        out.update(weights=m.weights, stats=tuple(sorted(m.compress_stats)))
    return out


# rows = n_prompts x n_batch x max_window, and the (B, n) window shapes of the same row counts
ENGINE_ROWS = {64: (2, 2, 16), 65: (5, 1, 13), 128: (4, 2, 16), 129: (43, 1, 3), 160: (5, 2, 16), 256: (8, 2, 16), 257: (257, 1, 1)}
WINDOWS = {64: (2, 32), 65: (5, 13), 128: (4, 32), 129: (43, 3), 160: (5, 32), 256: (8, 32), 257: (257, 1), "128 as 2 x 64": (2, 64)}
ENGINE_BACKBONES = {
    "lumina 12-bit": lambda: _chameleon("lumina7b", "bf16").enable_fused(OPS, gemm="sjd", compress=True),
    "lumina uncompressed": lambda: _chameleon("lumina7b", "bf16").enable_fused(OPS, gemm="sjd", compress=False),
    "lumina uncompressed 256-row set": lambda: _with_cfg(_chameleon("lumina7b", "bf16"), "G1_CFG_256ROW").enable_fused(OPS, gemm="sjd", compress=False),
    "lumina fp16 256-row set": lambda: _with_cfg(_chameleon("lumina7b", "fp16"), "G1_CFG_256ROW").enable_fused(OPS, gemm="sjd"),
    "lumina uncompressed, o on five tiles": lambda: _with_cfg(_chameleon("lumina7b", "bf16"), "G1_CFG", o=(512, 5, False)).enable_fused(OPS, gemm="sjd", compress=False),
    "lumina uncompressed, head on five tiles": lambda: _with_head(_chameleon("lumina7b", "bf16"), (1024, 5, True)).enable_fused(OPS, gemm="sjd", compress=False),
    "emu3 uncompressed": lambda: _chameleon("emu3_8b", "bf16").enable_fused(OPS, gemm="sjd", compress=False),
    "lumina e4m3": lambda: _chameleon("lumina7b", "bf16").enable_fused(OPS, gemm="sjd", weights="e4m3"),
    "lumina e4m3 64": lambda: _chameleon("lumina7b", "bf16").enable_fused(OPS, gemm="sjd", weights="e4m3", max_rows=64),
    "lumina e4m3 128": lambda: _chameleon("lumina7b", "bf16").enable_fused(OPS, gemm="sjd", weights="e4m3", max_rows=128),
    "lumina e4m3 256": lambda: _chameleon("lumina7b", "bf16").enable_fused(OPS, gemm="sjd", weights="e4m3", max_rows=256),
    "lumina e4m3_as_bf16 128": lambda: _chameleon("lumina7b", "bf16").enable_fused(OPS, gemm="sjd", weights="e4m3_as_bf16", max_rows=128),
    "lumina e4m3_as_bf16": lambda: _chameleon("lumina7b", "bf16").enable_fused(OPS, gemm="sjd", weights="e4m3_as_bf16"),
    "lumina torch gemm": lambda: _chameleon("lumina7b", "bf16").enable_fused(OPS, gemm="torch"),
    "chameleon30b": lambda: _chameleon("chameleon30b", "bf16").enable_fused(OPS, gemm="sjd"),
    "llamagen64 unfused": lambda: BB.LlamaGenBackbone(BB.LlamaGenArgs(**TINY_LG["llamagen64"])).to(torch.bfloat16),
    "llamagen100 unfused": lambda: BB.LlamaGenBackbone(BB.LlamaGenArgs(**TINY_LG["llamagen100"])).to(torch.bfloat16),
    "llamagen64 bf16 64": lambda: _lg("llamagen64", "bf16", 64),
    "llamagen64 bf16 128": lambda: _lg("llamagen64", "bf16", 128),
    "llamagen64 bf16 256": lambda: _lg("llamagen64", "bf16", 256),
    "llamagen64 fp16 128": lambda: _lg("llamagen64", "fp16", 128),
    "llamagen64 fp16 256": lambda: _lg("llamagen64", "fp16", 256, untuned_fp16=True),
    "llamagen100 bf16 64": lambda: _lg("llamagen100", "bf16", 64, pad_head_dim=True),
    "llamagen100 fp16 128": lambda: _lg("llamagen100", "fp16", 128, pad_head_dim=True, padded_batch=True),
}


def _with_cfg(m, name, **changed):
    m.G1_CFG = dict(getattr(m, name), **changed)
    return m


def _with_head(m, head_cfg):
    m.HEAD_CFG = head_cfg
    return m


def _lg(family, dtype, max_rows, **kw):
    torch.manual_seed(0)
    return BB.LlamaGenBackbone(BB.LlamaGenArgs(**TINY_LG[family])).to(DTYPES[dtype]).enable_fused(real_ops, gemm="sjd", max_rows=max_rows, **kw)


def observe_engine(backbone, rows, monkeypatch):
    """SJDBatchEngine.__init__ up to its first device allocation: "accepted", or the refusal's text"""
    def stop(*a, **k):
        raise _Prefill                                             # (the guards sit in front of every allocation)
    monkeypatch.setattr(real_ops, "BlobArray", stop)
    P, nb, Lw = ENGINE_ROWS[rows]
    try:
        SJDBatchEngine(backbone, 1024, "cpu", P, max_window=Lw, n_batch=nb)
    except _Prefill:
        return "accepted"
    except ValueError as e:
        return str(e)


def observe_window(m, key):
    """ChameleonBackbone._forward_window_fused for a (B, n) window: "window" (the G1 path), "prefill" (library GEMMs), or the refusal's text"""
    B, n = WINDOWS[key]
    m._forward_window_g1_folded = m._forward_window_g1 = lambda *a, **k: "window"
    m.cache = types.SimpleNamespace(k=[None], v=[None])
    tok = torch.zeros(B, n, dtype=torch.int64, device="meta")
    try:
        return m._forward_window_fused(tok, tok, 0, None)
    except _Prefill:
        return "prefill"
    except ValueError as e:
        return str(e)


# ------------------------------------------------------------------------------------------ what the code did before the rule moved
T_, F_ = True, False
SET_PLAIN = ((896, 8, T_), (512, 6, F_), (2048, 8, T_), (896, 8, F_))
SET_Z = ((1024, 6, T_), (512, 6, F_), (2048, 8, T_), (768, 8, F_))                  # also the 8-bit stream's set at <= 64 rows
SET_Q8_WIDE = ((2048, 4, T_), (1024, 3, T_), (2048, 8, T_), (1408, 4, T_))
SET_EMU3 = ((1024, 4, T_), (512, 4, T_), (2048, 8, T_), (1792, 4, T_))              # also its 8-bit stream's set at 128 / 256 rows
SET_EMU3_Z = ((512, 6, T_), (512, 4, T_), (2048, 8, T_), (896, 8, T_))
SET_EMU3_Q8 = ((512, 6, T_), (512, 4, T_), (1024, 8, T_), (896, 8, T_))
SET_30B = ((1536, 8, T_), (1536, 8, F_), (2048, 8, T_), (1536, 8, F_))
SET_30B_Z = ((1792, 8, T_), (1280, 8, T_), (2048, 8, T_), (1536, 8, T_))
HEAD, HEAD_WIDE = (1024, 4, T_), (2048, 8, T_)


def ok(g1, head, max_rows, given, kinds, **halved):
    """a served enable_fused call; kinds: what q|k|v and the head were packed as; halved: {name: the nine _q8_chunk values at ROWS} for the
    projections that do not read their packed chunk at every row count"""
    return dict(g1=g1, head=head, max_rows=max_rows, given=given, qkv=kinds[0], head_kind=kinds[1],
                chunks={n: halved.get(n, (kc,) * 9) for n, (kc, _, _) in zip(NAMES, g1)})


def no_weights(served):
    return (served,) + tuple(f"max_rows={r} goes with weights='e4m3' / 'e4m3_as_bf16' (without it the packed copy serves the row counts of its G1_CFG)" for r in (64, 128, 256))


NARROW_2048 = (2048,) + (1024,) * 8                                                   # rows 32 | 33 .. 256: packed for <= 64 rows, read in halves above 32
WIDE_2048 = (2048, 1024, 1024) + (2048,) * 6                                          # rows 32 | 33, 64 | 65 .. 256: packed for 128 / 256 rows
WIDE_1408 = (1408, 704, 704) + (1408,) * 6
WIDE_1792 = (1792, 896, 896) + (1792,) * 6


def lumina_q8(qkv, head):
    """max_rows unset, 64, 128, 256 under weights=...: qkv / head = what the projections / lm_head are packed as below 256 rows"""
    return (ok(SET_Z, HEAD, 64, F_, (qkv, head), gate_up=NARROW_2048), ok(SET_Z, HEAD, 64, T_, (qkv, head), gate_up=NARROW_2048),
            ok(SET_Q8_WIDE, HEAD, 128, T_, (qkv, head), qkv=WIDE_2048, gate_up=WIDE_2048, down=WIDE_1408),
            ok(SET_Q8_WIDE, HEAD, 256, T_, (qkv, "bfloat16"), qkv=WIDE_2048, gate_up=WIDE_2048, down=WIDE_1408))


def emu3_q8(qkv, head):
    return (ok(SET_EMU3_Q8, HEAD_WIDE, 64, F_, (qkv, head)), ok(SET_EMU3_Q8, HEAD_WIDE, 64, T_, (qkv, head)),
            ok(SET_EMU3, HEAD_WIDE, 128, T_, (qkv, head), gate_up=WIDE_2048, down=WIDE_1792),
            ok(SET_EMU3, HEAD_WIDE, 256, T_, (qkv, "bfloat16"), gate_up=WIDE_2048, down=WIDE_1792))


FP16_Q8 = {w: (f"weights={w!r} needs bf16 weights (got torch.float16): the dequantised values are bf16 numbers, fp16's exponent range does not hold them",) * 4
           for w in ("e4m3", "e4m3_as_bf16")}
SWIN_Q8 = {w: (f"weights={w!r} is not served for swin-norm backbones (swin_norm=True or model_parallel_size > 1)",) * 4 for w in ("e4m3", "e4m3_as_bf16")}
# (family, dtype, compress, weights) -> the outcome at max_rows unset, 64, 128, 256
EXPECTED_CHAMELEON = {
    ("lumina7b", "bf16", True, None): no_weights(ok(SET_Z, HEAD, None, F_, ("Z", "Z"))),
    ("lumina7b", "bf16", True, "e4m3"): lumina_q8("Q8", "Z"),
    ("lumina7b", "bf16", True, "e4m3_as_bf16"): lumina_q8("bfloat16", "Z"),
    ("lumina7b", "bf16", False, None): no_weights(ok(SET_PLAIN, HEAD, None, F_, ("bfloat16", "bfloat16"))),
    ("lumina7b", "bf16", False, "e4m3"): lumina_q8("Q8", "bfloat16"),
    ("lumina7b", "bf16", False, "e4m3_as_bf16"): lumina_q8("bfloat16", "bfloat16"),
    ("lumina7b", "fp16", True, None): no_weights(ok(SET_PLAIN, HEAD, None, F_, ("float16", "float16"))),
    ("lumina7b", "fp16", False, None): no_weights(ok(SET_PLAIN, HEAD, None, F_, ("float16", "float16"))),
    ("emu3_8b", "bf16", True, None): no_weights(ok(SET_EMU3_Z, HEAD_WIDE, None, F_, ("Z", "Z"))),
    ("emu3_8b", "bf16", True, "e4m3"): emu3_q8("Q8", "Z"),
    ("emu3_8b", "bf16", True, "e4m3_as_bf16"): emu3_q8("bfloat16", "Z"),
    ("emu3_8b", "bf16", False, None): no_weights(ok(SET_EMU3, HEAD_WIDE, None, F_, ("bfloat16", "bfloat16"))),
    ("emu3_8b", "bf16", False, "e4m3"): emu3_q8("Q8", "bfloat16"),
    ("emu3_8b", "bf16", False, "e4m3_as_bf16"): emu3_q8("bfloat16", "bfloat16"),
    ("emu3_8b", "fp16", True, None): no_weights(ok(SET_EMU3, HEAD_WIDE, None, F_, ("float16", "float16"))),
    ("emu3_8b", "fp16", False, None): no_weights(ok(SET_EMU3, HEAD_WIDE, None, F_, ("float16", "float16"))),
    # (swin-norm: nothing is folded, so lm_head is not packed)
    ("chameleon30b", "bf16", True, None): no_weights(ok(SET_30B_Z, HEAD, None, F_, ("Z", "NoneType"))),
    ("chameleon30b", "bf16", False, None): no_weights(ok(SET_30B, HEAD, None, F_, ("bfloat16", "NoneType"))),
    ("chameleon30b", "fp16", True, None): no_weights(ok(SET_30B, HEAD, None, F_, ("float16", "NoneType"))),
    ("chameleon30b", "fp16", False, None): no_weights(ok(SET_30B, HEAD, None, F_, ("float16", "NoneType"))),
}
for _c in (True, False):
    for _w in ("e4m3", "e4m3_as_bf16"):
        EXPECTED_CHAMELEON["lumina7b", "fp16", _c, _w] = EXPECTED_CHAMELEON["emu3_8b", "fp16", _c, _w] = FP16_Q8[_w]
        EXPECTED_CHAMELEON["chameleon30b", "bf16", _c, _w] = EXPECTED_CHAMELEON["chameleon30b", "fp16", _c, _w] = SWIN_Q8[_w]


@pytest.mark.parametrize("family,dtype,compress,weights", sorted(EXPECTED_CHAMELEON, key=str))
def test_chameleon_enable_fused(family, dtype, compress, weights):
    assert len(EXPECTED_CHAMELEON) == 36
    for max_rows, want in zip(MAX_ROWS, EXPECTED_CHAMELEON[family, dtype, compress, weights]):
        assert observe_chameleon(family, dtype, compress, weights, max_rows) == want, max_rows


# The axes added since: weights="mxfp4" and its twin on every family, and swin_quant=True on the 30B class -- recorded the same way, from the code before
# the quantised-copy rule was gathered into one function.  (family, dtype, compress, weights, swin_quant) -> the outcome at max_rows unset, 64, 128, 256
Q4_WIDE = {w: tuple(f"weights={w!r} serves windows of at most 64 rows (kernels G1q4 / G1sq4 have no wide form): max_rows is None or 64, got {r}" for r in (128, 256))
           for w in ("mxfp4", "mxfp4_as_bf16")}
SWIN_WIDE = {w: tuple(f"weights={w!r} serves swin-norm backbones at windows of at most 64 rows (one prompt per forward): max_rows is None or 64, got {r}" for r in (128, 256))
             for w in ("e4m3", "e4m3_as_bf16")}
NEEDS_BF16 = "weights={w!r} needs bf16 weights (got torch.float16): the dequantised values are bf16 numbers, fp16's exponent range does not hold them"
NO_SWIN = "weights={w!r} is not served for swin-norm backbones (swin_norm=True or model_parallel_size > 1)"
SWIN_1792, SWIN_1536 = (1792,) + (896,) * 8, (1536,) + (768,) * 8


def narrow(served, w):
    """max_rows unset and 64 served, 128 and 256 refused: the MXFP4 stream anywhere, either stream on a swin-norm backbone"""
    return (served, dict(served, given=T_)) + (Q4_WIDE[w] if w in Q4_WIDE else SWIN_WIDE[w])


def swin_q(kind, w):
    return narrow(ok(SET_30B_Z, HEAD, 64, F_, (kind, "NoneType"), qkv=SWIN_1792, gate_up=NARROW_2048, down=SWIN_1536), w)


EXPECTED_CHAMELEON_MORE = {}
for _c, _head in ((True, "Z"), (False, "bfloat16")):
    for _w, _k in (("mxfp4", "Q4"), ("mxfp4_as_bf16", "bfloat16")):
        EXPECTED_CHAMELEON_MORE["lumina7b", "bf16", _c, _w, False] = narrow(ok(SET_Z, HEAD, 64, F_, (_k, _head), gate_up=NARROW_2048), _w)
        EXPECTED_CHAMELEON_MORE["emu3_8b", "bf16", _c, _w, False] = narrow(ok(SET_EMU3_Q8, HEAD_WIDE, 64, F_, (_k, _head)), _w)
        EXPECTED_CHAMELEON_MORE["lumina7b", "fp16", _c, _w, False] = EXPECTED_CHAMELEON_MORE["emu3_8b", "fp16", _c, _w, False] = \
            EXPECTED_CHAMELEON_MORE["chameleon30b", "fp16", _c, _w, True] = (NEEDS_BF16.format(w=_w),) * 2 + Q4_WIDE[_w]
        EXPECTED_CHAMELEON_MORE["chameleon30b", "bf16", _c, _w, False] = EXPECTED_CHAMELEON_MORE["chameleon30b", "fp16", _c, _w, False] = \
            (NO_SWIN.format(w=_w),) * 2 + Q4_WIDE[_w]
        EXPECTED_CHAMELEON_MORE["chameleon30b", "bf16", _c, _w, True] = swin_q(_k, _w)
    for _w, _k in (("e4m3", "Q8"), ("e4m3_as_bf16", "bfloat16")):
        EXPECTED_CHAMELEON_MORE["chameleon30b", "bf16", _c, _w, True] = swin_q(_k, _w)
        EXPECTED_CHAMELEON_MORE["chameleon30b", "fp16", _c, _w, True] = (NEEDS_BF16.format(w=_w),) * 4
    for _d in DTYPES:          # (without weights swin_quant changes nothing)
        EXPECTED_CHAMELEON_MORE["chameleon30b", _d, _c, None, True] = EXPECTED_CHAMELEON["chameleon30b", _d, _c, None]


def chameleon_cases():
    """every (family, dtype, compress, weights, swin_quant) of the two tables"""
    return [k + (False,) for k in EXPECTED_CHAMELEON] + list(EXPECTED_CHAMELEON_MORE)


@pytest.mark.parametrize("family,dtype,compress,weights,swin_quant", sorted(EXPECTED_CHAMELEON_MORE, key=str))
def test_chameleon_enable_fused_mxfp4_and_swin_quant(family, dtype, compress, weights, swin_quant):
    assert len(EXPECTED_CHAMELEON_MORE) == 44 and len(set(chameleon_cases())) == 80          # 3 x 2 x 2 x 2 MXFP4 + 2 x 2 x 5 with swin_quant
    for max_rows, want in zip(MAX_ROWS, EXPECTED_CHAMELEON_MORE[family, dtype, compress, weights, swin_quant]):
        assert observe_chameleon(family, dtype, compress, weights, max_rows, swin_quant=swin_quant) == want, max_rows


def lg(g1, head, rows, kind, head_pad=None):
    return dict(g1=g1, head=head, max_rows=rows, fused_rows=rows, qkv=kind, head_kind=kind, head_pad=head_pad)


LG_64 = (((256, 2, T_), (256, 2, F_), (320, 2, F_), (512, 2, F_)), (640, 4, T_), 64)
LG_128 = (((320, 2, F_), (256, 2, F_), (320, 4, T_), (512, 2, F_)), (640, 4, T_), 128)
LG_256 = (((256, 4, F_), (256, 2, F_), (320, 4, T_), (512, 4, F_)), (640, 4, T_), 256)
LG3B_64 = (((640, 8, T_), (512, 4, F_), (1088, 8, T_), (1088, 4, T_)), (1088, 8, T_), 64)
LG3B_128 = (((1088, 4, F_), (512, 4, F_), (1088, 8, F_), (1088, 4, T_)), (1600, 4, T_), 128)
LG3B_256 = (((1088, 4, F_), (512, 4, T_), (1088, 8, T_), (1088, 4, T_)), (1600, 4, T_), 256)
LG_FP16_256 = ("LlamaGenBackbone.enable_fused: max_rows=256 packs bf16 weights; it keeps fp16 windows of at most 128 rows unless untuned_fp16=True "
               "(kernel G1 serves fp16 at 129..256 rows on the launch shapes swept in bf16)")
LG_PAD = {r: "LlamaGenBackbone.enable_fused: pad_head_dim=True serves windows of at most 64 rows (one prompt per forward) unless padded_batch=True, which "
             f"packs max_rows={r} on the launch shapes swept at head_dim 100 (G1_CFG_LLAMAGEN_3B_128ROW / _256ROW)" for r in (128, 256)}
# (family, dtype, untuned_fp16, padded_batch) -> the outcome at max_rows unset, 64, 128, 256
EXPECTED_LLAMAGEN = {
    ("llamagen64", "bf16", False, False): (lg(*LG_64, "bfloat16"), lg(*LG_64, "bfloat16"), lg(*LG_128, "bfloat16"), lg(*LG_256, "bfloat16")),
    ("llamagen64", "bf16", True, False): (lg(*LG_64, "bfloat16"), lg(*LG_64, "bfloat16"), lg(*LG_128, "bfloat16"), lg(*LG_256, "bfloat16")),
    ("llamagen64", "fp16", False, False): (lg(*LG_64, "float16"), lg(*LG_64, "float16"), lg(*LG_128, "float16"), LG_FP16_256),
    ("llamagen64", "fp16", True, False): (lg(*LG_64, "float16"), lg(*LG_64, "float16"), lg(*LG_128, "float16"), lg(*LG_256, "float16")),
    ("llamagen100", "bf16", False, False): (lg(*LG3B_64, "bfloat16", 128), lg(*LG3B_64, "bfloat16", 128), LG_PAD[128], LG_PAD[256]),
    ("llamagen100", "bf16", False, True): (lg(*LG3B_64, "bfloat16", 128), lg(*LG3B_64, "bfloat16", 128), lg(*LG3B_128, "bfloat16", 128), lg(*LG3B_256, "bfloat16", 128)),
    ("llamagen100", "bf16", True, False): (lg(*LG3B_64, "bfloat16", 128), lg(*LG3B_64, "bfloat16", 128), LG_PAD[128], LG_PAD[256]),
    ("llamagen100", "bf16", True, True): (lg(*LG3B_64, "bfloat16", 128), lg(*LG3B_64, "bfloat16", 128), lg(*LG3B_128, "bfloat16", 128), lg(*LG3B_256, "bfloat16", 128)),
    ("llamagen100", "fp16", False, False): (lg(*LG3B_64, "float16", 128), lg(*LG3B_64, "float16", 128), LG_PAD[128], LG_PAD[256]),
    ("llamagen100", "fp16", False, True): (lg(*LG3B_64, "float16", 128), lg(*LG3B_64, "float16", 128), lg(*LG3B_128, "float16", 128), LG_FP16_256),
    ("llamagen100", "fp16", True, False): (lg(*LG3B_64, "float16", 128), lg(*LG3B_64, "float16", 128), LG_PAD[128], LG_PAD[256]),
    ("llamagen100", "fp16", True, True): (lg(*LG3B_64, "float16", 128), lg(*LG3B_64, "float16", 128), lg(*LG3B_128, "float16", 128), lg(*LG3B_256, "float16", 128)),
}


@pytest.mark.parametrize("family,dtype,untuned_fp16,padded_batch", sorted(EXPECTED_LLAMAGEN))
def test_llamagen_enable_fused(family, dtype, untuned_fp16, padded_batch):
    for max_rows, want in zip(MAX_ROWS, EXPECTED_LLAMAGEN[family, dtype, untuned_fp16, padded_batch]):
        assert observe_llamagen(family, dtype, max_rows, untuned_fp16, padded_batch) == want, max_rows


# LlamaGen's `weights` axis, added since: LS.LLAMAGEN_QUANT_SETS, what the layers are packed as, and compress_stats' keys
LGQ_64 = (((256, 2, T_), (256, 2, F_), (384, 2, F_), (512, 2, F_)), (640, 4, T_), 64)
LGQ_128 = (((384, 4, F_), (256, 3, F_), (384, 4, T_), (512, 4, F_)), (640, 4, T_), 128)
LGQ_256 = (((256, 4, F_), (256, 3, F_), (384, 4, T_), (512, 4, F_)), (640, 4, T_), 256)
LGQ3B_64 = (((640, 8, T_), (512, 4, F_), (1152, 8, T_), (1152, 4, T_)), (1088, 8, T_), 64)
LGQ3B_128 = (((1152, 4, F_), (512, 4, F_), (1152, 8, F_), (1152, 4, T_)), (1600, 4, T_), 128)
LGQ3B_256 = (((1152, 4, F_), (512, 4, T_), (1152, 8, T_), (1152, 4, T_)), (1600, 4, T_), 256)
LG_WEIGHTS = {"e4m3": ("PackedQ8", ("bytes_packed", "bytes_raw", "matrices", "q8_bytes_packed", "q8_matrices", "rel_rms_error")),
              "e4m3_as_bf16": ("bfloat16", ("bytes_packed", "bytes_raw", "matrices", "q8_matrices", "rel_rms_error")),
              "mxfp4": ("PackedQ4", ("bytes_packed", "bytes_raw", "matrices", "q4_bytes_packed", "q4_matrices", "rel_rms_error")),
              "mxfp4_as_bf16": ("bfloat16", ("bytes_packed", "bytes_raw", "matrices", "q4_matrices", "rel_rms_error"))}
LG_UNTUNED = "weights={w!r} packs bf16 weights: untuned_fp16=True does not go with it"
LG_DIM_800 = "weights={w!r}: dim 800 and the intermediate size 2304 must be multiples of 128 (the MXFP4 stream travels in whole ring trips of eight k-steps)"


def lgq(g1, head, rows, w, head_pad=None):
    return dict(lg(g1, head, rows, "bfloat16", head_pad), qkv=LG_WEIGHTS[w][0], weights=w, stats=LG_WEIGHTS[w][1])


# (family, dtype, weights, untuned_fp16, padded_batch) -> the outcome at max_rows unset, 64, 128, 256
EXPECTED_LLAMAGEN_WEIGHTS = {}
for _w in LG_WEIGHTS:
    EXPECTED_LLAMAGEN_WEIGHTS["llamagen64", "bf16", _w, False, False] = (lgq(*LGQ_64, _w), lgq(*LGQ_64, _w), lgq(*LGQ_128, _w), lgq(*LGQ_256, _w))
    EXPECTED_LLAMAGEN_WEIGHTS["llamagen64", "bf16", _w, True, False] = (LG_UNTUNED.format(w=_w),) * 4
    EXPECTED_LLAMAGEN_WEIGHTS["llamagen64", "fp16", _w, False, False] = EXPECTED_LLAMAGEN_WEIGHTS["llamagen64", "fp16", _w, True, False] = (NEEDS_BF16.format(w=_w),) * 4
    # head_dim 100 stored 128 wide at dim 800: whole e4m3 pairs (the o projection's K is 8 x 128), not whole MXFP4 trips
    if _w in ("e4m3", "e4m3_as_bf16"):
        EXPECTED_LLAMAGEN_WEIGHTS["llamagen100", "bf16", _w, False, False] = (lgq(*LGQ3B_64, _w, 128), lgq(*LGQ3B_64, _w, 128), LG_PAD[128], LG_PAD[256])
        EXPECTED_LLAMAGEN_WEIGHTS["llamagen100", "bf16", _w, False, True] = (lgq(*LGQ3B_64, _w, 128), lgq(*LGQ3B_64, _w, 128), lgq(*LGQ3B_128, _w, 128), lgq(*LGQ3B_256, _w, 128))
    else:
        EXPECTED_LLAMAGEN_WEIGHTS["llamagen100", "bf16", _w, False, False] = (LG_DIM_800.format(w=_w),) * 2 + (LG_PAD[128], LG_PAD[256])
        EXPECTED_LLAMAGEN_WEIGHTS["llamagen100", "bf16", _w, False, True] = (LG_DIM_800.format(w=_w),) * 4


def llamagen_cases():
    """every (family, dtype, weights, untuned_fp16, padded_batch) of the two tables"""
    return [(f, d, None, u, p) for f, d, u, p in EXPECTED_LLAMAGEN] + list(EXPECTED_LLAMAGEN_WEIGHTS)


@pytest.mark.parametrize("family,dtype,weights,untuned_fp16,padded_batch", sorted(EXPECTED_LLAMAGEN_WEIGHTS))
def test_llamagen_enable_fused_weights(family, dtype, weights, untuned_fp16, padded_batch):
    assert len(EXPECTED_LLAMAGEN_WEIGHTS) == 24 and len(set(llamagen_cases())) == 36
    for max_rows, want in zip(MAX_ROWS, EXPECTED_LLAMAGEN_WEIGHTS[family, dtype, weights, untuned_fp16, padded_batch]):
        assert observe_llamagen(family, dtype, max_rows, untuned_fp16, padded_batch, weights=weights) == want, max_rows


# SJDBatchEngine's answers: "{rows}" is the case's row count, "{to}" the max_rows it names (128 up to 128 rows, 256 above)
OK_ = "accepted"
OVER = "the window forward (G1, F1-F3) serves at most 256 rows: n_prompts * n_batch * max_window <= 256"
NEED_RAW = "{rows} window rows per forward need the uncompressed packing: enable_fused(ops, gemm='sjd', compress=False) (the 12-bit stream serves up to 128 rows)"
BAD_TILES = ("{rows} window rows per forward run on kernel G1w with (2, 3, 4, 6, 8) column tiles per workgroup; set model.G1_CFG = dict(model.G1_CFG_256ROW) "
             "before enable_fused -- offending launch shapes: ")
Q8_SOLO = ("SJDBatchEngine does not serve a backbone packed with enable_fused(weights='e4m3'): 8-bit weights serve one prompt per forward (at most 64 window "
           "rows) in this version -- decode with SJDEngine, or pack with weights=None")
Q8_PACKED = ("the backbone was packed for windows of at most max_rows=%d rows, but n_prompts * n_batch * max_window = {rows}: call enable_fused(ops, gemm='sjd', "
             "weights='e4m3', max_rows={to}), or use fewer prompts per forward")
SWIN = ("SJDBatchEngine does not serve swin-norm backbones (swin_norm=True or model_parallel_size > 1, the 30B-class Chameleon form): decode them one prompt "
        "at a time with SJDEngine / FlexARInferenceSolver")
LG_UNFUSED = "SJDBatchEngine serves a LlamaGen backbone on the fused HIP path only: call model.enable_fused(ops, gemm='sjd', max_rows=...) first ({rows} window rows per forward here"
LG_PACKED = "the backbone was packed for windows of at most max_rows=%d rows, but n_prompts * n_batch * max_window = {rows}: call enable_fused(ops, gemm='sjd', max_rows={to}%s)"
LG_FP16 = ("the backbone was packed for fp16 windows of at most 128 rows, but n_prompts * n_batch * max_window = {rows}: call enable_fused(ops, gemm='sjd', "
           "max_rows=256, untuned_fp16=True%s), or use fewer prompts per forward")
PADDED = ", pad_head_dim=True, padded_batch=True"
# backbone -> the answer at 64, 65, 128, 129, 160, 256, 257 rows
EXPECTED_ENGINE = {
    "lumina 12-bit": (OK_,) * 3 + (NEED_RAW,) * 3 + (OVER,),
    "lumina uncompressed": (OK_,) * 6 + (OVER,),
    "lumina uncompressed 256-row set": (OK_,) * 6 + (OVER,),
    "lumina fp16 256-row set": (OK_,) * 6 + (OVER,),
    "lumina uncompressed, o on five tiles": (OK_,) * 3 + (BAD_TILES + "['o']",) * 3 + (OVER,),
    "lumina uncompressed, head on five tiles": (OK_,) * 3 + (BAD_TILES + "['lm_head (HEAD_CFG)']",) * 3 + (OVER,),
    "emu3 uncompressed": (OK_,) * 6 + (OVER,),
    "lumina e4m3": (Q8_SOLO,) * 7,
    "lumina e4m3 64": (OK_,) + (Q8_PACKED % 64,) * 5 + (OVER,),
    "lumina e4m3 128": (OK_,) * 3 + (Q8_PACKED % 128,) * 3 + (OVER,),
    "lumina e4m3 256": (OK_,) * 6 + (OVER,),
    "lumina e4m3_as_bf16 128": (OK_,) * 6 + (OVER,),
    "lumina e4m3_as_bf16": (OK_,) * 6 + (OVER,),
    "lumina torch gemm": (OK_,) * 6 + (OVER,),
    "chameleon30b": (SWIN,) * 7,
    "llamagen64 unfused": (LG_UNFUSED + ")",) * 6 + (OVER,),
    "llamagen100 unfused": (LG_UNFUSED + "; head_dim 100: with pad_head_dim=True, padded_batch=True)",) * 6 + (OVER,),
    "llamagen64 bf16 64": (OK_,) + (LG_PACKED % (64, ""),) * 5 + (OVER,),
    "llamagen64 bf16 128": (OK_,) * 3 + (LG_PACKED % (128, ""),) * 3 + (OVER,),
    "llamagen64 bf16 256": (OK_,) * 6 + (OVER,),
    "llamagen64 fp16 128": (OK_,) * 3 + (LG_FP16 % "",) * 3 + (OVER,),
    "llamagen64 fp16 256": (OK_,) * 6 + (OVER,),
    "llamagen100 bf16 64": (OK_,) + (LG_PACKED % (64, PADDED),) * 5 + (OVER,),
    "llamagen100 fp16 128": (OK_,) * 3 + (LG_FP16 % PADDED,) * 3 + (OVER,),
}
# ChameleonBackbone._forward_window_fused at the windows of WINDOWS: 64, 65, 128, 129, 160, 256, 257 rows, then 128 rows as 2 x 64
W_, P_ = "window", "prefill"
Q8_ROWS_64 = "weights='e4m3' serves draft windows of at most 64 rows (one prompt per forward); got {rows} rows"
Q8_ROWS_128 = "weights='e4m3' serves draft windows of at most 128 rows (max_rows=128); got {rows} rows"
EXPECTED_WINDOW = {
    "lumina 12-bit": (W_,) * 3 + (P_,) * 5,
    "lumina uncompressed": (W_,) * 6 + (P_,) * 2,
    "lumina uncompressed 256-row set": (W_,) * 6 + (P_,) * 2,
    "lumina fp16 256-row set": (W_,) * 6 + (P_,) * 2,
    "lumina uncompressed, o on five tiles": (W_,) * 3 + (P_,) * 5,
    "lumina uncompressed, head on five tiles": (W_,) * 6 + (P_,) * 2,
    "emu3 uncompressed": (W_,) * 6 + (P_,) * 2,
    "lumina e4m3": (W_,) + (Q8_ROWS_64,) * 5 + (P_,) * 2,
    "lumina e4m3 64": (W_,) + (Q8_ROWS_64,) * 5 + (P_,) * 2,
    "lumina e4m3 128": (W_,) * 3 + (Q8_ROWS_128,) * 3 + (P_,) * 2,
    "lumina e4m3 256": (W_,) * 6 + (P_,) * 2,
    "lumina e4m3_as_bf16 128": (W_,) * 6 + (P_,) * 2,
    "lumina e4m3_as_bf16": (W_,) * 6 + (P_,) * 2,
    "lumina torch gemm": (P_,) * 8,
    "chameleon30b": (W_,) * 3 + (P_,) * 5,
}


@pytest.mark.parametrize("name", list(ENGINE_BACKBONES))
def test_rows_served(name, monkeypatch):
    assert set(EXPECTED_ENGINE) == set(ENGINE_BACKBONES)
    b = ENGINE_BACKBONES[name]()
    for rows, want in zip(ENGINE_ROWS, EXPECTED_ENGINE[name]):
        assert observe_engine(b, rows, monkeypatch) == want.format(rows=rows, to=128 if rows <= 128 else 256), rows
    if name in EXPECTED_WINDOW:
        for key, want in zip(WINDOWS, EXPECTED_WINDOW[name]):
            B, n = WINDOWS[key]
            assert observe_window(b, key) == want.format(rows=B * n), key
    else:
        assert not isinstance(b, BB.ChameleonBackbone)


# ------------------------------------------------------------------------------------------ refusals of a quantised copy, by reason and call site
# Each case changes ONE projection (or the head) of a set that passes, so that exactly one reason applies; the backbones have the real dimensions
# (Lumina-7B, Chameleon-30B, LlamaGen GPT-XXL: one layer on the meta device -- a refusal comes before anything is packed).  The full text is pinned.
def _cham_site(family, weights, max_rows, base, swin_quant=False):
    return lambda g1=None, head=None: observe_chameleon(family, "bf16", True, weights, max_rows, swin_quant, dict(getattr(BB.LS, base), **(g1 or {})), head)


def _lg_site(weights, max_rows):
    return lambda g1=None, head=None: observe_llamagen("gpt_xxl", "bf16", max_rows, False, False, weights, dict(BB.LS.LLAMAGEN_QUANT_SETS[False, max_rows][0], **(g1 or {})), head)


REFUSAL_SITES = {
    "chameleon e4m3": _cham_site("lumina7b", "e4m3", None, "G1_CFG_Q8"),
    "chameleon e4m3 wide": _cham_site("lumina7b", "e4m3", 256, "G1_CFG_Q8_WIDE"),
    "chameleon mxfp4": _cham_site("lumina7b", "mxfp4", None, "G1_CFG_Q4"),
    "swin e4m3": _cham_site("chameleon30b", "e4m3", None, "G1_CFG_30B_Q8", True),
    "swin mxfp4": _cham_site("chameleon30b", "mxfp4", None, "G1_CFG_30B_Q4", True),
    "llamagen e4m3 64": _lg_site("e4m3", 64), "llamagen e4m3 256": _lg_site("e4m3", 256),
    "llamagen mxfp4 64": _lg_site("mxfp4", 64), "llamagen mxfp4 256": _lg_site("mxfp4", 256),
}
# one sentence per reason, whatever the call site (the literals recorded first held four near copies of each: kernel G1q / G1q4 / "G1q / G1q4", "chunks of" / "a chunk
# of", a lead-in naming the stream's record pairs or ring trips; Chameleon's e4m3 chunk cap printed the whole set instead of the projection and its K)
R_GRANULE = "K and the chunk must be multiples of %d"
R_CHUNK = "kernels G1q / G1q4 stage the whole activation chunk in LDS -- every chunk must be <= 2560 columns"
R_HALVED = "windows of 33..64 rows need a chunk of <= 1280 columns, or a step-major packing whose halved chunk is a multiple of %d"
R_TILES = ("windows of more than 64 rows take 3, 4, 6 or 8 column tiles per workgroup on the quantised streams (kernels G1wq / G1wq4 have no form of three row tiles x "
           "two tiles)")
R_HEAD = "the output head runs on kernel G1w at these row counts -- HEAD_CFG[1] must be one of (2, 3, 4, 6, 8); HEAD_CFG = (1024, 5, True)"
LG_HEAD_TILES = "windows of more than 64 rows take (2, 3, 4, 6, 8) column tiles per workgroup; offending launch shapes: ['head']"          # (the 16-bit tile check comes first)
E4M3, E4M3_256, MXFP4 = "weights='e4m3': ", "weights='e4m3', max_rows=256: ", "weights='mxfp4': "
# (call site, reason) -> (the one projection changed, HEAD_CFG when it is the head that changes, the refusal)
EXPECTED_REFUSALS = {
    ("chameleon e4m3", "chunk"): (dict(qkv=(4096, 6, True)), None, E4M3 + R_CHUNK + "; G1_CFG['qkv'] = (4096, 6, True) with K = 4096"),
    ("chameleon e4m3 wide", "granule"): (dict(o=(528, 3, True)), None, E4M3_256 + R_GRANULE % 32 + "; G1_CFG['o'] = (528, 3, True) with K = 4096"),
    ("chameleon e4m3 wide", "chunk"): (dict(qkv=(4096, 4, True)), None, E4M3_256 + R_CHUNK + "; G1_CFG['qkv'] = (4096, 4, True) with K = 4096"),
    ("chameleon e4m3 wide", "halved"): (dict(down=(1408, 4, False)), None, E4M3_256 + R_HALVED % 32 + "; G1_CFG['down'] = (1408, 4, False) with K = 11008"),
    ("chameleon e4m3 wide", "tiles"): (dict(o=(1024, 2, True)), None, E4M3_256 + R_TILES + "; G1_CFG['o'] = (1024, 2, True) with K = 4096"),
    ("chameleon e4m3 wide", "head tiles"): (None, (1024, 5, True), E4M3_256 + R_HEAD),
    ("chameleon mxfp4", "granule"): (dict(qkv=(1000, 6, True)), None, MXFP4 + R_GRANULE % 128 + "; G1_CFG['qkv'] = (1000, 6, True) with K = 4096"),
    ("chameleon mxfp4", "chunk"): (dict(qkv=(4096, 6, True)), None, MXFP4 + R_CHUNK + "; G1_CFG['qkv'] = (4096, 6, True) with K = 4096"),
    ("chameleon mxfp4", "halved"): (dict(down=(1408, 8, True)), None, MXFP4 + R_HALVED % 128 + "; G1_CFG['down'] = (1408, 8, True) with K = 11008"),
    ("swin e4m3", "granule"): (dict(down=(1552, 8, True)), None, E4M3 + R_GRANULE % 32 + "; G1_CFG['down'] = (1552, 8, True) with K = 22016"),
    ("swin e4m3", "chunk"): (dict(qkv=(2688, 8, True)), None, E4M3 + R_CHUNK + "; G1_CFG['qkv'] = (2688, 8, True) with K = 8192"),
    ("swin e4m3", "halved"): (dict(o=(1536, 8, False)), None, E4M3 + R_HALVED % 32 + "; G1_CFG['o'] = (1536, 8, False) with K = 8192"),
    ("swin mxfp4", "granule"): (dict(down=(1552, 8, True)), None, MXFP4 + R_GRANULE % 128 + "; G1_CFG['down'] = (1552, 8, True) with K = 22016"),
    ("swin mxfp4", "chunk"): (dict(qkv=(2688, 8, True)), None, MXFP4 + R_CHUNK + "; G1_CFG['qkv'] = (2688, 8, True) with K = 8192"),
    ("swin mxfp4", "halved"): (dict(o=(1536, 8, False)), None, MXFP4 + R_HALVED % 128 + "; G1_CFG['o'] = (1536, 8, False) with K = 8192"),
}
for _w, _g in (("e4m3", 32), ("mxfp4", 128)):          # (LlamaGen's sentences are the ones kept: nothing changed here)
    for _r in (64, 256):
        _s, _p = f"llamagen {_w} {_r}", f"weights={_w!r}, max_rows={_r}: "
        EXPECTED_REFUSALS[_s, "granule"] = (dict(down=(208, 4, False)), None, _p + R_GRANULE % _g + "; G1_CFG['down'] = (208, 4, False) with K = 4096")
        EXPECTED_REFUSALS[_s, "chunk"] = (dict(down=(2688, 4, True)), None, _p + R_CHUNK + "; G1_CFG['down'] = (2688, 4, True) with K = 4096")
        EXPECTED_REFUSALS[_s, "halved"] = (dict(down=(1408, 4, False)), None, _p + R_HALVED % _g + "; G1_CFG['down'] = (1408, 4, False) with K = 4096")
    EXPECTED_REFUSALS[_s, "tiles"] = (dict(o=(256, 2, False)), None, _p + R_TILES + "; G1_CFG['o'] = (256, 2, False) with K = 1536")
    EXPECTED_REFUSALS[_s, "head tiles"] = (None, (640, 5, True), LG_HEAD_TILES)


@pytest.mark.parametrize("site,reason", sorted(EXPECTED_REFUSALS))
def test_quantised_copy_refusals(site, reason):
    assert len(EXPECTED_REFUSALS) == 31 and {s for s, _ in EXPECTED_REFUSALS} == set(REFUSAL_SITES)
    g1, head, want = EXPECTED_REFUSALS[site, reason]
    assert REFUSAL_SITES[site](g1, head) == want


@pytest.mark.parametrize("site", [s for s in REFUSAL_SITES if not s.startswith("llamagen")])
def test_the_sets_the_refusal_cases_start_from_are_served(site):
    assert isinstance(REFUSAL_SITES[site](), dict)          # (LlamaGen's, at the real widths: tests/test_llamagen_quant_cfg.py)
