"""CPU: the host side of lenient verification (SJDConfig.lenience, LOSSY and off by default) -- the refusals, the 16 bits the factor travels in
beside the scheme, the distribution the relaxed rule draws from, and the keyword's default on every public signature."""
import ctypes
import dataclasses
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests.conftest import ROOT

LAMBDAS = [1.0, 1.25, 1.5, 2.0, 4.0, 2.0 ** 100]


# ------------------------------------------------------------------------------------------------ refusals
def _solo():
    """SJDEngine's host side without a device: decode validates its config before it touches one (any attribute it reached would raise)"""
    from sjd_amd.engine import SJDEngine
    eng = SJDEngine.__new__(SJDEngine)
    eng.Lmax = 16
    return eng


def _batch():
    from sjd_amd.engine_batch import SJDBatchEngine
    eng = SJDBatchEngine.__new__(SJDBatchEngine)
    eng.P, eng.nb, eng.Lmax, eng.slot_launches, eng.head_partials, eng._guidance, eng._mixed_guidance = 2, 2, 16, True, True, 3.0, False
    return eng


def _decode(kind, cfg):
    if kind == "solo":
        return _solo().decode([1, 2, 3], None, None, cfg)
    return _batch().decode_many([[], []], [None, None], [None, None], cfg)


@pytest.mark.parametrize("kind", ["solo", "batch"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), 0.5, 0.0, -2.0, 0.999])
def test_not_finite_or_below_one_is_refused(kind, bad):
    from sjd_amd.engine import SJDConfig
    with pytest.raises(ValueError, match=r"lenience must be finite and >= 1 \(1 is the exact verify rule\), but got"):
        _decode(kind, SJDConfig(lenience=bad))


@pytest.mark.parametrize("kind", ["solo", "batch"])
@pytest.mark.parametrize("bad,lo,hi", [(1.1, 1.09375, 1.1015625), (3.3, 3.296875, 3.3125), (1.0 + 2.0 ** -8, 1.0, 1.0078125),
                                       (1.0 + 2.0 ** -30, 1.0, 1.0078125), (1000.5, 1000.0, 1004.0)])
def test_not_a_bf16_value_is_refused_with_its_neighbours(kind, bad, lo, hi):
    """never rounded silently: the message names the bf16 values on both sides"""
    from sjd_amd.engine import SJDConfig, lenience_field
    for v in (lo, hi):                                               # the named neighbours are bf16 values, adjacent ones, and they bracket `bad`
        assert int(np.float32(v).view(np.uint32)) & 0xffff == 0 and float(np.float32(v)) == v
    assert lo < bad < hi and (int(np.float32(hi).view(np.uint32)) - int(np.float32(lo).view(np.uint32))) == 0x10000
    with pytest.raises(ValueError, match=r"is not exactly a bf16 value .*the two neighbours that are: (\S+) and (\S+)$") as e:
        _decode(kind, SJDConfig(lenience=bad))
    m = re.search(r"neighbours that are: (\S+) and (\S+)$", str(e.value))
    assert (float(m.group(1)), float(m.group(2))) == (lo, hi)
    assert lenience_field(lo) >= 0 and lenience_field(hi) > 0         # ... and both are accepted


@pytest.mark.parametrize("kind", ["solo", "batch"])
def test_plain_jacobi_with_a_factor_is_refused(kind):
    from sjd_amd.engine import SJDConfig
    with pytest.raises(ValueError, match=r"lenience=2.0 needs prefix_token_sampler_scheme='speculative_jacobi'"):
        _decode(kind, SJDConfig(lenience=2.0, prefix_token_sampler_scheme="jacobi"))
    # lenience 1 with plain Jacobi is today's call: the config check passes and the decode goes on to its (absent) device
    with pytest.raises(AttributeError):
        _decode(kind, SJDConfig(lenience=1.0, prefix_token_sampler_scheme="jacobi"))


def test_the_factor_must_agree_across_the_prompts_of_one_decode_many():
    from sjd_amd.engine import SJDConfig
    from sjd_amd import engine_batch as EB
    assert "lenience" not in EB._PER_PROMPT_FIELDS and dataclasses.fields(SJDConfig)[-1].name == "lenience"
    with pytest.raises(ValueError, match=r"SJDConfig\.lenience must agree .* prompt 0 has 1.0 and prompt 1 has 2.0"):
        _decode("batch", [SJDConfig(seed=1), SJDConfig(seed=2, lenience=2.0)])


def test_solvers_refuse_at_construction():
    from sjd_amd.llamagen_solver import LlamaGenSolver
    from sjd_amd.scheduler.jacobi_iteration_lumina_mgpt import renew_sampler
    with pytest.raises(ValueError, match="lenience must be finite and >= 1"):
        LlamaGenSolver(None, 1000, 1.0, lenience=0.5)
    with pytest.raises(ValueError, match="not exactly a bf16 value"):
        LlamaGenSolver(None, 1000, 1.0, lenience=1.1)
    cls = renew_sampler(type("M", (), {}))
    with pytest.raises(ValueError, match="needs prefix_token_sampler_scheme='speculative_jacobi'"):
        cls()._init_new_params(lenience=4.0, prefix_token_sampler_scheme="jacobi")
    m = cls()
    m._init_new_params(lenience=4.0)
    assert m.lenience == 4.0 and LlamaGenSolver(m, 1000, 1.0).lenience == 4.0 and LlamaGenSolver(m, 1000, 1.0, lenience=2.0).lenience == 2.0


# ------------------------------------------------------------------------------------------------ the encoding
class _HostBlob:
    """ops.DeviceBlob's host half"""

    def __init__(self):
        import sjd_amd._lib as L
        self.host = torch.zeros(ctypes.sizeof(L.IterParams), dtype=torch.uint8)
        self.view = L.IterParams.from_address(self.host.data_ptr())


def _filled(eng, scheme=0):
    import sjd_amd.ops as ops
    eng._rule_bytes, eng._rule_keep = {}, []
    blob = _HostBlob()
    rules = [ops.make_rule(ranges=((4, 8196),), top_k=2000) for _ in range(16)]
    eng._fill_blob(blob, 16, 100, True, scheme, [7, 8, 9], rules, rules[:15], (1024, 1234, 0, 8, 16))
    return blob


def test_default_blob_is_byte_identical_to_one_built_without_the_field():
    import sjd_amd._lib as L
    from sjd_amd.engine import SJDConfig
    never = _solo()                                                   # an engine no decode has configured: what bench.py's direct _fill_params sees
    want = _filled(never).host.clone()
    assert want.any()
    for scheme_name, scheme in (("speculative_jacobi", 0), ("jacobi", 1)):
        eng = _solo()
        eng._check_config(SJDConfig(prefix_token_sampler_scheme=scheme_name), [])
        blob = _filled(eng, scheme)
        assert blob.view.scheme == scheme
        ref = _filled(never, scheme)
        assert bytes(blob.host.numpy().tobytes()) == bytes(ref.host.numpy().tobytes())
    assert SJDConfig().lenience == 1.0
    assert bytes(_filled(never).host.numpy().tobytes()) == bytes(want.numpy().tobytes())
    # the layout did not move
    assert ctypes.sizeof(L.IterParams) == 64 + 8 * L.MAX_WINDOW + 2 * 52 * L.MAX_WINDOW and L.IterParams.scheme.offset == 12


@pytest.mark.parametrize("lam", LAMBDAS)
def test_round_trip(lam):
    from sjd_amd.engine import SJDConfig, lenience_field, lenience_of, LENIENCE_SHIFT
    field = lenience_field(lam)
    assert field & 0xffff == 0 and 0 <= field < 2 ** 31               # bits 16-31 only, and a positive int32
    assert (field == 0) == (lam == 1.0)
    assert lenience_of(field) == lam and lenience_of(field | 1) == lam
    if lam != 1.0:
        assert field >> LENIENCE_SHIFT == int(np.float32(lam).view(np.uint32)) >> 16
    eng = _solo()
    eng._check_config(SJDConfig(lenience=lam), [])
    blob = _filled(eng)                                              # (kept: the view reads the blob's memory)
    word = blob.view.scheme
    assert word & 0xff == 0 and lenience_of(word) == lam
    assert lenience_of(0x3f80 << 16) == 1.0                          # (1.0 spelled out is 1.0 as well)


def test_header_names_the_field():
    hdr = open(os.path.join(ROOT, "include", "sjd_hip.h")).read()
    assert "#define SJD_SCHEME_OF(word) ((int)((uint32_t)(word) & 0xffu))" in hdr
    assert "#define SJD_LENIENCE_BITS_OF(word) ((uint32_t)(word) >> 16)" in hdr
    src = open(os.path.join(ROOT, "accelerating-t2i-ar-with-sjd_amd", "csrc", "sjd_sampling.hip")).read()
    assert "SJD_SCHEME_OF(" in src and "SJD_LENIENCE_BITS_OF(" in src
    assert not re.search(r"params->scheme\s*(==|!=)", src)            # every reader of the word takes the scheme bits


# ------------------------------------------------------------------------------------------------ the distribution
def _norm(v):
    s = v.sum()
    return v / s if s > 0 else v


def r_formula(p, q, lam):
    """r(x) = min(q, lam p) + (1 - sum min(q, lam p)) norm(max(p - q / lam, 0))"""
    a = np.minimum(q, lam * p)
    return a + (1.0 - a.sum()) * _norm(np.maximum(p - q / lam, 0.0))


def r_enumerated(p, q, lam):
    """the rule itself: a draft x ~ q is accepted with min(1, lam p(x) / q(x)), else the token comes from the residual norm(max(p - q / lam, 0))"""
    V = len(p)
    res = _norm(np.maximum(p - q / lam, 0.0))
    out = np.zeros(V)
    for x in range(V):
        if q[x] == 0.0:
            continue
        acc = min(1.0, lam * p[x] / q[x])
        out[x] += q[x] * acc
        out += q[x] * (1.0 - acc) * res
    return out


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("shape", ["dense", "sparse", "one-hot draft"])
def test_output_distribution(seed, shape):
    V = 64
    g = np.random.default_rng(seed)
    p, q = _norm(g.random(V) ** 3), _norm(g.random(V) ** 3)
    if shape == "sparse":                                            # top-k style supports that only partly overlap
        p[g.permutation(V)[:40]] = 0.0
        q[g.permutation(V)[:40]] = 0.0
        p, q = _norm(p), _norm(q)
    elif shape == "one-hot draft":                                   # a fresh random draft: q is a one-hot (q' holds 1 / lam at x)
        q = np.zeros(V)
        q[int(g.integers(V))] = 1.0
    assert np.allclose(r_formula(p, q, 1.0), p, rtol=0, atol=1e-15)   # lam = 1: the exact rule's r = p
    for lam in LAMBDAS[1:]:
        r = r_formula(p, q, lam)
        assert (r >= 0).all()
        # (when min(q, lam p) already holds all the mass -- every draft is accepted, lam = 2^100 -- the residual term is 0 x anything)
        assert abs(r.sum() - 1.0) < 1e-12
        assert np.allclose(r, r_enumerated(p, q, lam), rtol=0, atol=1e-14)
    # the limit: every draft with p(x) > 0 is accepted, r -> q on p's support
    big = r_formula(p, q, 2.0 ** 100)
    on = p > 0
    assert np.allclose(big[on], q[on] + (1.0 - q[on].sum()) * _norm(np.maximum(p - q / 2.0 ** 100, 0))[on], rtol=0, atol=1e-14)


# ------------------------------------------------------------------------------------------------ the public surface
def test_keyword_default_is_one_everywhere():
    from sjd_amd.engine import SJDConfig
    from sjd_amd.inference_solver import FlexARInferenceSolver
    from sjd_amd.llamagen_solver import LlamaGenSolver
    from sjd_amd.scheduler import jacobi_iteration_lumina_mgpt as JL, jacobi_iteration_anhole as JA, jacobi_iteration_emu3 as JE
    assert SJDConfig().lenience == 1.0
    default = lambda fn: inspect.signature(fn).parameters["lenience"].default
    assert default(JL.renew_sampler(type("M", (), {}))._init_new_params) == 1.0
    for fn in (JL.renew_pipeline_sampler, JA.renew_pipeline_sampler, JE.renew_solver, FlexARInferenceSolver.__init__, LlamaGenSolver.__init__):
        assert default(fn) == 1.0, fn
    import importlib.util
    spec = importlib.util.spec_from_file_location("llamagen_c2i_example", os.path.join(ROOT, "examples", "llamagen_c2i.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    assert ex.parse_args([]).lenience == 1.0 and ex.parse_args(["--lenience", "1.5"]).lenience == 1.5
    with pytest.raises(SystemExit):
        ex.parse_args(["--lenience", "1.1"])


def test_the_samplers_hand_the_factor_to_the_config():
    """renew_pipeline_sampler / renew_solver -> model.lenience -> the SJDConfig of _sample and _sample_many"""
    from sjd_amd.scheduler import jacobi_iteration_lumina_mgpt as JL, jacobi_iteration_emu3 as JE
    src = inspect.getsource(JL.renew_sampler)
    assert src.count('lenience=getattr(self, "lenience", 1.0)') == 2

    class _Model:
        pass

    class _Pipe:
        def __init__(self, lenience=None):
            self.model = _Model()
            if lenience is not None:
                self.lenience = lenience
    assert JL.renew_pipeline_sampler(_Pipe()).model.lenience == 1.0
    assert JL.renew_pipeline_sampler(_Pipe(), lenience=1.5).model.lenience == 1.5
    assert JL.renew_pipeline_sampler(_Pipe(lenience=2.0)).model.lenience == 2.0          # the solver's own value holds unless the call names one
    assert JL.renew_pipeline_sampler(_Pipe(lenience=2.0), lenience=4.0).model.lenience == 4.0

    class _Fn:
        visual_tokens = [0]

    class _Proc:
        def build_prefix_constrained_fn(self, h, w):
            return _Fn()
    model, _ = JE.renew_solver(_Model(), _Proc(), h=2, w=2, lenience=1.25)
    assert model.lenience == 1.25
