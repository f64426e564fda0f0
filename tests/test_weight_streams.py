"""CPU: the lossy weight streams (e4m3, MXFP4, e2m3) are stated once, in launch_shapes.STREAMS, and every call site reads that table.

A: the table against the module-level names that tests and tools read, the ops.PackedQ* classes and the _lib flags.
B: every refusal a stream can cause, message for message -- enable_fused of both backbones, SJDBatchEngine.__init__ and the window forward's row limit --
   against tests/golden/weight_stream_refusals.json.
C: the arguments ops.skinny_gemm_cols / gateup_silu / prefill_gemm hand the C entry points per stream, over a stand-in for the library that launches
   nothing, against the same file.

The fixture is what `python -m tests.test_weight_streams --record` wrote on the commit BEFORE the table existed, when each stream's facts were written out
per call site; the enumeration reads only names that commit had, so it can be run there again.  It must not be regenerated from a later tree."""
import ctypes
import json
import os
import sys
from types import SimpleNamespace as NS

import pytest
import torch

import sjd_amd._lib as L
import sjd_amd.backbones as BB
import sjd_amd.engine_batch as EB
import sjd_amd.launch_shapes as LS
import sjd_amd.ops as ops
import sjd_amd.synthetic as synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "weight_stream_refusals.json")
STREAM_NAMES = ("e4m3", "mxfp4", "e2m3")
WEIGHTS = tuple(n + t for n in STREAM_NAMES for t in ("", "_as_bf16")) + ("int6",)          # the six names and one nobody serves
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}

TOY = dict(vocab_size=1024, hidden_size=256, intermediate_size=512, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=2,
           max_position_embeddings=256)
# chunks of whole MXFP4 granules, tile counts the wide kernels take: every stream packs it at every row count it serves
TOY_CFG = dict(qkv=(128, 4, True), o=(256, 3, False), gate_up=(128, 8, True), down=(256, 4, False))
TOY_LG = dict(dim=128, n_layer=1, n_head=2, vocab_size=1024, block_size=64)
# LlamaGen's dim / intermediate-size check, in both wordings: 192 = 1.5 MXFP4 granules; multiple_of=8 gives an intermediate size of 344 = 10.75 e4m3 pairs
TOY_LG_ODD = {"dim 192": dict(TOY_LG, dim=192, n_head=3), "inter 344": dict(TOY_LG, multiple_of=8)}


def _shapes_only(cls):
    """a packer that keeps the shapes and returns the matrix as its own dequantised form: the refusals come before anything is packed, and a call that goes
    through is only recorded as one"""
    class Shapes(cls):
        def __init__(self, w, KC, step_major):
            super().__init__(None, w.shape[0], w.shape[1], KC, step_major, dict(rel_rms_error=0.0))
            self._w = w

        def nbytes(self):
            return self.N * self.K

        def dequant(self):
            return self._w
    return lambda w, KC, step_major=False, gateup=False: Shapes(w, KC, step_major)


class _Ops:
    """sjd_amd.ops with the three quantising packers replaced by _shapes_only ones"""
    pack_weight_q8, pack_weight_q4, pack_weight_q6 = (staticmethod(_shapes_only(c)) for c in (ops.PackedQ8, ops.PackedQ4, ops.PackedQ6))

    def __getattr__(self, name):
        return getattr(ops, name)


OPS = _Ops()


def _said(fn):
    """None where the call goes through, else the refusal as "Type: text\""""
    try:
        fn()
    except (ValueError, AssertionError, L.SjdLibraryError) as e:
        return type(e).__name__ + ": " + str(e)
    return None


def _cham(dtype="bf16", swin=False):
    m = BB.ChameleonBackbone(BB.ChameleonArgs(qk_norm=True, **dict(TOY, **(dict(swin_norm=True, model_parallel_size=2) if swin else {})))).eval()
    synthetic.fill_state_dict(m, seed=3, embed_token_scale=0.25)
    m = m.to(DT[dtype])
    m.G1_CFG = dict(TOY_CFG)
    return m


def _lg(dtype="bf16", args=TOY_LG):
    torch.manual_seed(0)
    return BB.LlamaGenBackbone(BB.LlamaGenArgs(**args)).to(DT[dtype])


# ------------------------------------------------------------------------------------------ B: the refusals
def chameleon_refusals():
    """enable_fused over names x max_rows x {plain, swin-norm} x swin_quant x release_16bit x dtype.  A refused call leaves the backbone as it was
    (tests/test_q6_cfg.py and its siblings hold that), so one backbone serves until a call packs it."""
    out = {}
    for dtype in DT:
        for swin in (False, True):
            m = None
            for weights in WEIGHTS:
                for max_rows in (None, 64, 128, 256, 96):
                    for sq in (False, True):
                        for rel in (False, True):
                            m = m or _cham(dtype, swin)
                            key = f"chameleon {dtype}{' swin-norm' if swin else ''} weights={weights} max_rows={max_rows} swin_quant={sq} release_16bit={rel}"
                            out[key] = _said(lambda: m.enable_fused(OPS, gemm="sjd", compress=False, weights=weights, max_rows=max_rows, swin_quant=sq, release_16bit=rel))
                            if out[key] is None:
                                m = None
    odd = dict(TOY_CFG, down=(144, 4, False))          # a chunk of 4.5 e4m3 pairs: the granule a refusal names is the stream's
    for weights in WEIGHTS[:-1]:
        for rel in (False, True):
            m = _cham()
            m.G1_CFG = dict(odd)
            out[f"chameleon bf16 down in chunks of 144 weights={weights} release_16bit={rel}"] = _said(lambda: m.enable_fused(OPS, gemm="sjd", compress=False, weights=weights, release_16bit=rel))
    return out


def llamagen_refusals():
    out = {}
    for dtype in DT:
        for weights in WEIGHTS:
            for max_rows in (64, 128, 256):
                out[f"llamagen {dtype} weights={weights} max_rows={max_rows}"] = _said(lambda: _lg(dtype).enable_fused(OPS, gemm="sjd", weights=weights, max_rows=max_rows))
    for what, args in TOY_LG_ODD.items():
        for weights in WEIGHTS[:-1]:
            out[f"llamagen {what} weights={weights}"] = _said(lambda: _lg(args=args).enable_fused(OPS, gemm="sjd", weights=weights))
    return out


class _Accepted(Exception):
    pass


def _accept(*a, **k):
    raise _Accepted


def engine_refusals(monkeypatch):
    """SJDBatchEngine.__init__ up to its first allocation (the guards sit in front of it) over a bare stand-in for a packed Chameleon-family backbone, and
    over packed LlamaGen backbones, which a stream with a LlamaGen route serves above 64 rows"""
    monkeypatch.setattr(ops, "BlobArray", _accept)
    monkeypatch.setattr(L, "load", lambda: None)          # (the guards in front of the first allocation call nothing in the library: no build is needed)
    plain = NS(swin_norm=False, model_parallel_size=1)
    out = {}

    def ask(key, backbone):
        for rows, prompts in ((64, 2), (128, 4), (256, 8)):
            try:
                out[f"engine {key} rows={rows}"] = _said(lambda: EB.SJDBatchEngine(backbone, 1024, "cpu", prompts, max_window=16, n_batch=2))
            except _Accepted:
                out[f"engine {key} rows={rows}"] = None
    for weights in WEIGHTS[:-1]:
        for max_rows in (None, 128, 256) if weights.startswith("e4m3") else (None,):
            ask(f"chameleon weights={weights} max_rows={max_rows}",
                NS(args=plain, weights=weights, max_rows=max_rows or 64, _max_rows_given=max_rows is not None, _gemm="sjd", _ops=ops, _packed=[dict(qkv=None)],
                   _packed_head=None, G1_CFG=LS.G1_CFG_Q8_WIDE, HEAD_CFG=LS.HEAD_CFG))
    for weights in ("e4m3", "mxfp4", "mxfp4_as_bf16"):
        ask(f"llamagen weights={weights} max_rows=128", _lg().enable_fused(OPS, gemm="sjd", weights=weights, max_rows=128))
    return out


def window_refusals():
    """_forward_window_fused's row limit, in front of its first launch: the two window forwards behind it are swapped for a stand-in that launches nothing"""
    out = {}
    for weights in WEIGHTS[:-1]:
        for max_rows in (None, 128) if weights.startswith("e4m3") else (None,):
            m = _cham().enable_fused(OPS, gemm="sjd", compress=False, weights=weights, max_rows=max_rows)
            m._forward_window_g1_folded = m._forward_window_g1 = lambda *a, **k: None
            for B, n in ((8, 16), (8, 32)):
                tok = torch.zeros(B, n, dtype=torch.long)
                out[f"window weights={weights} max_rows={max_rows} rows={B * n}"] = _said(
                    lambda: m._forward_window_fused(tok, tok, 0, torch.zeros(B, dtype=torch.int32)))
    return out


# ------------------------------------------------------------------------------------------ C: the dispatch
class _Library:
    """stands in for L.load(): every entry point records its name and its integer arguments and reports success"""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*a):
            self.calls.append(dict(entry=name, ints=[int(x) for x in a if isinstance(x, (bool, int))]))
            return 0
        return entry


def dispatch(monkeypatch):
    lib = _Library()
    monkeypatch.setattr(L, "load", lambda: lib)
    monkeypatch.setattr(L, "check", lambda rc, what: lib.calls[-1].update(label=what))
    monkeypatch.setattr(ops, "_stream", lambda: ctypes.c_void_p(0))
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(128, 512, generator=g) * 0.05).to(torch.bfloat16)
    x = torch.zeros(4, 512, dtype=torch.bfloat16)
    packers = dict(e4m3=ops.pack_weight_q8, mxfp4=ops.pack_weight_q4, e2m3=ops.pack_weight_q6)
    out = {}

    def run(key, fn):
        lib.calls.clear()
        err = _said(fn)
        out[key] = err if err is not None else [dict(c) for c in lib.calls]
    for name, pack in packers.items():
        cols, halves, quarters = pack(w, 128, True), pack(w, 256, True, gateup=True), pack(w, 128, True)
        run(f"skinny_gemm_cols {name}", lambda: ops.skinny_gemm_cols(x, cols, 128, 512, 256, 32, 64, 4, True))          # (step-major: read in another chunk)
        run(f"skinny_gemm {name}", lambda: ops.skinny_gemm(x, cols, 128, 512, 128, 4, True))
        run(f"gateup_silu {name}", lambda: ops.gateup_silu(x, halves, 64, 512, True))
        run(f"gateup_silu {name} four chunks", lambda: ops.gateup_silu(x, quarters, 64, 512, True))          # (MXFP4 only: the others assert two K halves)
        run(f"prefill_gemm {name}", lambda: ops.prefill_gemm(x, cols, 128, 512))
    plain = ops.pack_weight(w, 128, True)
    run("skinny_gemm_cols plain", lambda: ops.skinny_gemm_cols(x, plain, 128, 512, 128, 32, 64, 4, True))
    run("gateup_silu plain", lambda: ops.gateup_silu(x, ops.pack_weight(w, 256, True), 64, 512, True))
    run("prefill_gemm plain", lambda: ops.prefill_gemm(x, plain, 128, 512, KC=128, step_major=True))
    return out


def record(monkeypatch):
    refusals = dict(chameleon_refusals(), **llamagen_refusals(), **engine_refusals(monkeypatch), **window_refusals())
    return dict(refusals=refusals, dispatch=dispatch(monkeypatch))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


# the sentences the table merged or rebuilt: each must be reached by the enumeration (a fragment no other refusal contains -> how many entries at least)
SENTENCES = {
    "'e4m3' or 'e4m3_as_bf16', 'mxfp4' or 'mxfp4_as_bf16', 'e2m3' or 'e2m3_as_bf16'": 2,          # the accepted names, Chameleon family
    "'mxfp4' or 'mxfp4_as_bf16'\n": 6,          # ... LlamaGen (the sentence ends there: e2m3 and the unknown name)
    "(kernels G1q4 / G1sq4 have no wide form): max_rows is None or 64, got": 2,
    "(kernels G1q6 / G1sq6 have no wide form): max_rows is None or 64, got": 2,
    "is not served for swin-norm backbones (swin_norm=True or model_parallel_size > 1), with or without swin_quant": 2,
    "has no prefill kernel (G1p reads the e4m3 / MXFP4 copies): release_16bit=True does not go with it": 2,
    "is not served for swin-norm backbones (swin_norm=True or model_parallel_size > 1)\n": 4,
    "K and the chunk must be multiples of 32; G1_CFG['down'] = (144, 4, False) with K = 512": 2,          # (e4m3 and its twin with release_16bit)
    "K and the chunk must be multiples of 128; G1_CFG['down'] = (144, 4, False) with K = 512": 4,          # (mxfp4; e2m3 without release_16bit)
    "must be multiples of 128 (the MXFP4 stream travels in whole ring trips of eight k-steps)": 2,
    "must be multiples of 32 (the e4m3 stream travels in whole record pairs)": 2,
    "window rows per forward (kernels G1q4 / G1sq4 have no wide form), but n_prompts": 4,
    "window rows per forward (kernels G1q6 / G1sq6 have no wide form), but n_prompts": 4,
    "serves draft windows of at most 64 rows (kernels G1q4 / G1sq4 have no wide form); got": 4,
    "serves draft windows of at most 64 rows (kernels G1q6 / G1sq6 have no wide form); got": 4,
    "weights='e4m3' serves draft windows of at most 128 rows (max_rows=128); got 256 rows": 1,
    "weights='e4m3' serves draft windows of at most 64 rows (one prompt per forward); got": 2,
    "ValueError: prefill_gemm: the e2m3 stream (PackedQ6) has no prefill kernel; prefill from the 16-bit weights": 1,
}


def test_the_fixture_reaches_every_sentence(golden):
    said = [v + "\n" for v in list(golden["refusals"].values()) + list(golden["dispatch"].values()) if isinstance(v, str)]
    assert said and any(v is None for v in golden["refusals"].values())
    for fragment, at_least in SENTENCES.items():
        assert sum(fragment in s for s in said) >= at_least, fragment
    labels = {c.get("label") for v in golden["dispatch"].values() if isinstance(v, list) for c in v}
    for name in STREAM_NAMES:
        assert {f"sjd_skinny_gemm_cols ({name} weights)", f"sjd_gateup_silu ({name} weights)"} <= labels
    assert {"sjd_skinny_gemm_cols", "sjd_gateup_silu", "sjd_prefill_gemm"} <= labels
    four = golden["dispatch"]["gateup_silu mxfp4 four chunks"]
    assert four[0]["entry"] == "sjd_gateup_silu" and 1 | 4 << L.G1S_CHUNKS_SHIFT in four[0]["ints"]
    assert all(isinstance(golden["dispatch"][f"gateup_silu {n} four chunks"], str) for n in ("e4m3", "e2m3"))


@pytest.mark.parametrize("part", ["chameleon", "llamagen", "engine", "window"])
def test_refusals_message_for_message(part, golden, monkeypatch):
    got = dict(chameleon=chameleon_refusals, llamagen=llamagen_refusals, engine=lambda: engine_refusals(monkeypatch), window=window_refusals)[part]()
    want = {k: v for k, v in golden["refusals"].items() if k.startswith(part + " ")}
    assert len(got) == len(want) > 0
    assert got == want


def test_dispatch_arguments(golden, monkeypatch):
    assert json.loads(json.dumps(dispatch(monkeypatch))) == golden["dispatch"]


# ------------------------------------------------------------------------------------------ A: the table
def test_table_against_the_legacy_names():
    e4m3, mxfp4, e2m3 = LS.STREAMS
    assert [s.names[0] for s in LS.STREAMS] == list(STREAM_NAMES) and [s.tag for s in LS.STREAMS] == ["q8", "q4", "q6"]
    assert LS.Q4_WEIGHTS == mxfp4.names == ("mxfp4", "mxfp4_as_bf16") and LS.Q6_WEIGHTS == e2m3.names == ("e2m3", "e2m3_as_bf16")
    assert LS.QUANT_WEIGHTS == e4m3.names + mxfp4.names == tuple(n for s in LS.STREAMS if "llamagen" in s.has for n in s.names)
    assert LS.Q4_GRANULE == ops.Q4_GRANULE == mxfp4.granule == e2m3.granule == 128 and e4m3.granule == 32
    assert LS.Q4_MAX_ROWS == mxfp4.max_rows == 64 == LS.Q6_MAX_ROWS == e2m3.max_rows and e4m3.max_rows == LS.WINDOW_MAX_ROWS
    assert [sorted(s.has) for s in LS.STREAMS] == [["llamagen", "prefill", "swin"], ["gateup_k4", "llamagen", "prefill", "swin"], []]
    assert [s.kernels for s in LS.STREAMS] == ["G1q / G1sq", "G1q4 / G1sq4", "G1q6 / G1sq6"]
    assert e4m3.sets == (LS.G1_CFG_Q8, LS.G1_CFG_EMU3_Q8, LS.G1_CFG_30B_Q8, LS.G1_CFG_Q8_WIDE, LS.G1_CFG_EMU3_Q8_WIDE)
    assert mxfp4.sets == e2m3.sets == (LS.G1_CFG_Q4, LS.G1_CFG_EMU3_Q4, LS.G1_CFG_30B_Q4, None, None)


def test_lookup_by_name():
    assert LS.stream_of(None) == (None, False) == LS.stream_of("int6") == LS.stream_of(["e4m3"])
    for s in LS.STREAMS:
        assert LS.stream_of(s.names[0]) == (s, False) and LS.stream_of(s.names[1]) == (s, True) and s.names[1] == s.names[0] + "_as_bf16"


def test_each_packed_class_names_its_stream_and_its_flag():
    w = (torch.randn(32, 128, generator=torch.Generator().manual_seed(1)) * 0.05).to(torch.bfloat16)
    flags = []
    for s in LS.STREAMS:
        cls = getattr(ops, "Packed" + s.tag.upper())
        packed = getattr(ops, "pack_weight_" + s.tag)(w, 128)
        assert type(packed) is cls and cls.weight_stream is s and isinstance(packed, ops.Packed) and ops.streamed(packed) == (s, packed.data, getattr(L, s.flag))
        flags.append(getattr(L, s.flag))
    assert flags == [L.G1_W8_E4M3, L.G1_W4_MXFP4, L.G1_W6_E2M3] and len(set(flags)) == 3 and all(f > 0 and f & (f - 1) == 0 for f in flags)
    assert issubclass(ops.PackedZ, ops.Packed) and not hasattr(ops.PackedZ, "weight_stream")          # lossless: its own entry points, not a row of the table
    plain = ops.pack_weight(w, 128)
    assert not isinstance(plain, ops.Packed) and ops.streamed(plain) == (None, plain, 0)


if __name__ == "__main__":
    if "--record" in sys.argv:
        assert not os.path.exists(GOLDEN), "the fixture is recorded once, on the commit before the table"
        mp = pytest.MonkeyPatch()
        try:
            doc = record(mp)
        finally:
            mp.undo()
        with open(GOLDEN, "w") as f:
            json.dump(doc, f, indent=0, sort_keys=True)
        print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes;", sum(v is not None for v in doc["refusals"].values()), "refusals of", len(doc["refusals"]))
