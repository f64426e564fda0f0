"""CPU: the host side of coupled Jacobi decoding (prefix_token_sampler_scheme="coupled_jacobi", code 2 of sjd_iter_params.scheme) -- the scheme
word, where the blob writer puts base and stride, the refusals, the name on every entry point, and the NumPy model of the loop
(tests/coupled_model.py): for the same per-position noise the emitted sequence does not depend on the draft window."""
import ctypes
import dataclasses
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

from tests import coupled_model as CM
from tests.conftest import ROOT

NAME = "coupled_jacobi"


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


class _HostBlob:
    """ops.DeviceBlob's host half"""

    def __init__(self):
        import sjd_amd._lib as L
        self.host = torch.zeros(ctypes.sizeof(L.IterParams), dtype=torch.uint8)
        self.view = L.IterParams.from_address(self.host.data_ptr())


def _filled(eng, scheme, philox=(1024, 1234, 0, 8, 16)):
    import sjd_amd.ops as ops
    eng._rule_bytes, eng._rule_keep = {}, []
    blob = _HostBlob()
    rules = [ops.make_rule(ranges=((4, 8196),), top_k=2000) for _ in range(16)]
    eng._fill_blob(blob, 16, 100, True, scheme, [7, 8, 9], rules, rules[:15], philox)
    return blob


# ------------------------------------------------------------------------------------------------ the scheme word
def test_scheme_codes():
    from sjd_amd.engine import SCHEME_CODES, SJDConfig, scheme_code
    assert SCHEME_CODES == {"speculative_jacobi": 0, "jacobi": 1, NAME: 2}
    assert scheme_code(NAME) == 2
    with pytest.raises(ValueError, match="prefix_token_sampler_scheme: vertical"):
        scheme_code("vertical")
    eng = _solo()
    eng._check_config(SJDConfig(prefix_token_sampler_scheme=NAME), [])
    blob = _filled(eng, scheme_code(NAME))                           # (kept: the view reads the blob's memory)
    word = blob.view.scheme
    assert word == 2 and word & 0xff == 2 and word >> 16 == 0
    hdr = open(os.path.join(ROOT, "include", "sjd_hip.h")).read()
    assert "2: coupled_jacobi" in hdr and "#define SJD_SCHEME_OF(word) ((int)((uint32_t)(word) & 0xffu))" in hdr


@pytest.mark.parametrize("lam", [1.0, 1.5, 4.0])
def test_the_other_schemes_words_are_todays(lam):
    """speculative_jacobi and jacobi, with and without a lenience factor: the blob's bytes are what the writer gave before the scheme existed --
    the scheme in bits 0-7, the factor's bf16 bits in 16-31 (0 for 1.0), nothing else in the word"""
    import sjd_amd._lib as L
    from sjd_amd.engine import SJDConfig, scheme_code
    never = _solo()                                                   # an engine no decode has configured
    for name, code in (("speculative_jacobi", 0), ("jacobi", 1)):
        if name == "jacobi" and lam != 1.0:
            continue                                                  # (refused: tests/test_lenience_cfg.py)
        eng = _solo()
        eng._check_config(SJDConfig(prefix_token_sampler_scheme=name, lenience=lam), [])
        blob = _filled(eng, scheme_code(name))
        bits = 0 if lam == 1.0 else int(np.float32(lam).view(np.uint32)) >> 16
        assert blob.view.scheme == code | (bits << 16)
        ref = _filled(never, code)
        ref.view.scheme = code | (bits << 16)
        assert bytes(blob.host.numpy().tobytes()) == bytes(ref.host.numpy().tobytes())
    assert ctypes.sizeof(L.IterParams) == 64 + 8 * L.MAX_WINDOW + 2 * 52 * L.MAX_WINDOW and L.IterParams.scheme.offset == 12


def test_exports_did_not_grow():
    import sjd_amd._lib as L
    assert len(L.EXPORTS) == 45


# ------------------------------------------------------------------------------------------------ the host's blob writer
class _Grammar:
    def window_rules(self, n):
        import sjd_amd.ops as ops
        return [ops.make_rule(top_k=100)] * n

    def fast_residual_rules(self, win, rules):
        return rules[:-1]

    def force_no_cfg(self):
        return False

    def grid(self):
        return None

    def push(self, tokens):
        pass


@pytest.mark.parametrize("greedy", [False, True])
def test_plan_puts_base_and_stride_where_stated(greedy):
    """PromptLoop + _fill_blob: the prefill iteration is the per-launch draw every scheme makes (code 1, the cursor's offsets); every window
    iteration carries code 2, word 0 = the base (the cursor right behind the prefill's draw), word 1 = the per-position stride
    sjd_philox_offset_increment(V, blocks), word 2 = 0 -- the same three words in every iteration: the host advances nothing"""
    import sjd_amd.ops as ops
    from sjd_amd.engine import SJDConfig, scheme_code
    from sjd_amd.window_loop import PromptLoop
    V, blocks, seed, off0, kv_base = 9216, 1024, 77, 4000, 5
    stride = ops.philox_step(V, blocks)
    assert stride == 4 * (-(-V // (4 * min(-(-V // 256), blocks) * 256))) and stride % 4 == 0
    cfg = SJDConfig(prefix_token_sampler_scheme=NAME, max_num_new_tokens=4, jacobi_loop_interval_l=0, jacobi_loop_interval_r=40, do_sample=not greedy)
    scheme = scheme_code(NAME)
    eng = _solo()
    eng._check_config(cfg, [])
    eng._rule_bytes, eng._rule_keep = {}, []
    loop, g = PromptLoop([11, 12, 13], kv_base, cfg, seed, off0), _Grammar()
    blob = _HostBlob()

    def iteration(m, tokens):
        n_rows, fresh, rules, win, resid, use_cfg, draws_rs, offs = loop.plan(cfg, g, None, V, blocks, greedy, scheme, True)
        eng._fill_blob(blob, n_rows, loop.kv_len, use_cfg, loop.launch_scheme(scheme), fresh, rules, resid or [], (blocks, seed) + offs)
        words = (blob.view.scheme, blob.view.philox_blocks, blob.view.philox_seed, tuple(blob.view.philox_offset))
        assert not draws_rs and resid == []
        loop.absorb(m, 0, tokens, tokens, n_rows if not loop.first else 3, cfg, g)
        return n_rows, words

    n, words = iteration(1, [21] * 16)
    k2 = 0 if greedy else stride                                     # (a greedy decode draws nothing: JL:127-129)
    assert n == 1 and words == (1, blocks, seed, (off0, off0 + k2, off0 + k2 + stride))
    base = off0 + k2
    assert loop.ph_off == base and loop.kv_len == kv_base + 3
    for m in (2, 4, 1):
        kv = loop.kv_len
        n, words = iteration(m, list(range(30, 46)))
        assert n == 4 and words == (2, blocks, seed, (base, stride, 0))
        assert loop.ph_off == base and loop.kv_len == kv + m           # the cursor does not move; positions do
    # hand-back: behind the noise of the last position that emitted a token (cache row kv_len - 1)
    assert loop.end_offset() == base + (0 if greedy else loop.kv_len * stride)
    # the other schemes: the cursor itself, as ever
    other = PromptLoop([11, 12, 13], kv_base, cfg, seed, off0)
    assert other.end_offset() == off0 and other.launch_scheme(0) == 0 and other.launch_scheme(1) == 1 and other.keyed(0, 9) is None


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("kind", ["solo", "batch"])
def test_lenience_is_refused(kind):
    from sjd_amd.engine import SJDConfig
    with pytest.raises(ValueError, match=r"^lenience=2.0 needs prefix_token_sampler_scheme='speculative_jacobi': coupled Jacobi verifies by token "
                                         r"equality, there is no acceptance probability to relax$"):
        _decode(kind, SJDConfig(lenience=2.0, prefix_token_sampler_scheme=NAME))
    with pytest.raises(AttributeError):                              # lenience 1: the config check passes, the decode goes on to its (absent) device
        _decode(kind, SJDConfig(lenience=1.0, prefix_token_sampler_scheme=NAME))


@pytest.mark.parametrize("kind", ["solo", "batch"])
def test_host_noise_is_refused(kind):
    from sjd_amd.engine import SJDConfig
    with pytest.raises(ValueError, match=r"^prefix_token_sampler_scheme='coupled_jacobi' needs in-kernel noise: K2 generates a row's noise from the "
                                         r"row's position, but noise_device='cpu' draws the noise on the host and hands it over as tensors; leave "
                                         r"noise_device=None$"):
        _decode(kind, SJDConfig(noise_device="cpu", prefix_token_sampler_scheme=NAME))
    with pytest.raises(AttributeError):                              # (the device's own generator is in-kernel noise)
        _decode(kind, SJDConfig(noise_device="cuda", prefix_token_sampler_scheme=NAME))


def test_noise_hook_of_the_solvers_is_refused():
    """model.sjd_noise_device / LlamaGenSolver(noise_device=...): the switch that makes a decode read noise tensors"""
    from sjd_amd.llamagen_solver import LlamaGenSolver
    from sjd_amd.scheduler.jacobi_iteration_lumina_mgpt import renew_sampler
    m = renew_sampler(type("M", (), {}))()
    m._init_new_params(prefix_token_sampler_scheme=NAME)
    with pytest.raises(ValueError, match="needs in-kernel noise: .* noise_device='cpu'"):
        LlamaGenSolver(m, 1000, 1.0, noise_device="cpu")
    solver = LlamaGenSolver(m, 1000, 1.0)
    solver.noise_device = "cpu"                                        # (set behind the constructor's back: generate() looks again, before the cache)
    with pytest.raises(ValueError, match="needs in-kernel noise"):
        solver.generate(torch.zeros(1, dtype=torch.long), 16)
    m.sjd_noise_device = "cpu"
    with pytest.raises(ValueError, match="needs in-kernel noise"):
        m._sample(torch.zeros(1, 4, dtype=torch.long), None, None, type("G", (), {"return_dict_in_generate": False})(), False, None)
    with pytest.raises(ValueError, match="coupled Jacobi verifies by token equality"):
        m._init_new_params(prefix_token_sampler_scheme=NAME, lenience=2.0)
    with pytest.raises(ValueError, match="coupled Jacobi verifies by token equality"):
        LlamaGenSolver(m, 1000, 1.0, lenience=1.5)


@pytest.mark.parametrize("other", ["speculative_jacobi", "jacobi"])
@pytest.mark.parametrize("first", [True, False])
def test_mixing_schemes_in_one_decode_many_is_refused(other, first):
    from sjd_amd.engine import SJDConfig
    cfgs = [SJDConfig(seed=1, prefix_token_sampler_scheme=NAME), SJDConfig(seed=2, prefix_token_sampler_scheme=other)]
    if not first:
        cfgs.reverse()
    a, b = cfgs[0].prefix_token_sampler_scheme, cfgs[1].prefix_token_sampler_scheme
    with pytest.raises(ValueError, match=rf"^prefix_token_sampler_scheme='coupled_jacobi' cannot be mixed with another scheme in one decode_many "
                                         rf"\(prompt 0 has '{a}', prompt 1 has '{b}'\)"):
        _decode("batch", cfgs)
    with pytest.raises(AttributeError):                              # both coupled: served
        _decode("batch", [SJDConfig(seed=1, prefix_token_sampler_scheme=NAME), SJDConfig(seed=2, prefix_token_sampler_scheme=NAME)])


@pytest.mark.parametrize("kind", ["solo", "batch"])
def test_greedy_is_allowed(kind):
    from sjd_amd.engine import SJDConfig
    with pytest.raises(AttributeError):                              # past the config check
        _decode(kind, SJDConfig(do_sample=False, prefix_token_sampler_scheme=NAME))


# ------------------------------------------------------------------------------------------------ the surface
def test_the_name_reaches_every_entry_point():
    from sjd_amd.engine import SJDConfig
    from sjd_amd.inference_solver import FlexARInferenceSolver
    from sjd_amd.llamagen_solver import LlamaGenSolver
    from sjd_amd.scheduler import jacobi_iteration_lumina_mgpt as JL, jacobi_iteration_anhole as JA, jacobi_iteration_emu3 as JE
    assert SJDConfig(prefix_token_sampler_scheme=NAME).prefix_token_sampler_scheme == NAME
    # renew_sampler: the attribute, and from there the SJDConfig of _sample and _sample_many
    cls = JL.renew_sampler(type("M", (), {}))
    m = cls()
    m._init_new_params(prefix_token_sampler_scheme=NAME)
    assert m.prefix_token_sampler_scheme == NAME
    src = inspect.getsource(JL.renew_sampler)
    assert src.count("prefix_token_sampler_scheme=self.prefix_token_sampler_scheme") == 2 and src.count("scheme_code(self.prefix_token_sampler_scheme)") == 2
    assert '("speculative_jacobi", "jacobi")' not in src

    class _Model:
        pass

    class _Pipe:                                                     # FlexARInferenceSolver is renewed as a pipeline: its model gets the name
        def __init__(self):
            self.model = _Model()
    assert JL.renew_pipeline_sampler(_Pipe(), prefix_token_sampler_scheme=NAME).model.prefix_token_sampler_scheme == NAME
    assert "renew_pipeline_sampler" in inspect.getsource(FlexARInferenceSolver) or hasattr(FlexARInferenceSolver, "generate")
    with pytest.raises(ValueError, match="coupled Jacobi verifies by token equality"):
        JL.renew_pipeline_sampler(_Pipe(), prefix_token_sampler_scheme=NAME, lenience=2.0)

    class _Fn:
        visual_tokens = [0]

    class _Proc:
        image_seq_length = 16

        def build_prefix_constrained_fn(self, h, w):
            return _Fn()
    model, _ = JE.renew_solver(_Model(), _Proc(), h=2, w=2, prefix_token_sampler_scheme=NAME)
    assert model.prefix_token_sampler_scheme == NAME
    # the Anole path renews with the same sampler: the keyword travels in **kwargs to its _init_new_params
    assert "renew_sampler(pipe_line.__class__)" in inspect.getsource(JA.renew_pipeline_sampler) and JA.renew_sampler is JL.renew_sampler
    # LlamaGenSolver reads the scheme of the renewed model
    assert LlamaGenSolver(m, 1000, 1.0).model.prefix_token_sampler_scheme == NAME
    # model_wrappers hand the keyword on
    loader = open(os.path.join(ROOT, "model_wrappers", "model_loader.py")).read()
    assert loader.count("prefix_token_sampler_scheme=prefix_token_sampler_scheme") == 3
    # the example
    spec = importlib.util.spec_from_file_location("llamagen_c2i_example", os.path.join(ROOT, "examples", "llamagen_c2i.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    assert ex.parse_args([]).scheme == "speculative_jacobi" and ex.parse_args(["--scheme", NAME]).scheme == NAME
    with pytest.raises(SystemExit):
        ex.parse_args(["--scheme", NAME, "--lenience", "2"])
    with pytest.raises(SystemExit):
        ex.parse_args(["--scheme", "vertical"])
    assert "prefix_token_sampler_scheme=a.scheme" in inspect.getsource(ex.main)


def test_decode_many_takes_the_name():
    from sjd_amd.engine import SJDConfig
    from sjd_amd.engine_batch import per_prompt_configs
    cfgs = [SJDConfig(seed=j, prefix_token_sampler_scheme=NAME) for j in range(3)]
    shared, per = per_prompt_configs(cfgs, 3)
    assert shared.prefix_token_sampler_scheme == NAME and per == cfgs
    assert "prefix_token_sampler_scheme" not in __import__("sjd_amd.engine_batch", fromlist=["x"])._PER_PROMPT_FIELDS
    assert dataclasses.fields(SJDConfig)[-1].name == "lenience"      # (no new config field: the scheme is a name)


# ------------------------------------------------------------------------------------------------ the loop, as a NumPy model
V_MODEL, N_TOKENS = 64, 48


def _table(seed):
    """prefix -> distribution: a fresh random row per distinct prefix (an order-infinity model: nothing about a row's distribution repeats),
    with exact zeros (top-k style support)"""
    rows = {}

    def dist_of(prefix):
        if prefix not in rows:
            g = np.random.default_rng([seed, len(prefix)] + list(prefix[-6:]))
            z = g.standard_normal(V_MODEL).astype(np.float32) * np.float32(2.0)
            z[g.permutation(V_MODEL)[:24]] = -np.inf
            e = np.exp(z - z.max()).astype(np.float32)
            rows[prefix] = (e / e.sum(dtype=np.float32)).astype(np.float32)
        return rows[prefix]
    return dist_of


def _noise(seed):
    return lambda t: np.random.default_rng([seed, 99, t]).exponential(size=V_MODEL).astype(np.float32)


def _fresh(seed):
    g = np.random.default_rng([seed, 7])
    return lambda k: g.integers(0, V_MODEL, size=k).tolist()


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_model_windows_give_the_same_sequence(seed):
    dist_of, noise_of = _table(seed), _noise(seed)
    runs = {w: CM.decode(dist_of, noise_of, 5, N_TOKENS, w, _fresh(seed + 10 * w)) for w in (1, 4, 16)}
    ar, steps1 = runs[1]
    assert steps1 == [1] * N_TOKENS                                  # window 1 is the autoregressive sample under that noise
    X = [5]
    for t in range(N_TOKENS):                                        # ... spelled out
        X.append(CM.race_draw(dist_of(tuple(X)), noise_of(t)))
    assert X[1:] == ar
    for w in (4, 16):
        seq, steps = runs[w]
        assert seq == ar, f"window {w}"
        assert sum(steps) == N_TOKENS and len(steps) <= N_TOKENS and min(steps) >= 1      # never more steps than tokens
    assert CM.decode(dist_of, _noise(seed + 100), 5, N_TOKENS, 16, _fresh(seed))[0] != ar   # other noise, other sample


def test_model_draw_and_accept():
    p = np.array([0.0, 0.5, 0.25, 0.25], dtype=np.float32)
    assert CM.race_draw(p, np.array([1e-9, 1.0, 0.5, 0.5], dtype=np.float32)) == 1      # 0.5 three times: the lowest index; no mass never wins
    assert CM.race_draw(p, np.array([1.0, 4.0, 0.5, 1.0], dtype=np.float32)) == 2
    assert CM.accept_len([9, 1, 2, 3], [1, 2, 3, 4]) == 4 and CM.accept_len([9, 1, 5, 3], [1, 2, 3, 4]) == 2 and CM.accept_len([9, 0], [1, 2]) == 1
    assert CM.accept_len([9], [1]) == 1
    calls = []
    assert CM.next_window(3, [4, 5, 6], 3, lambda k: calls.append(k) or [8] * k) == [3, 4, 5] and calls == [0]
    assert CM.next_window(3, [4], 4, lambda k: [8] * k) == [3, 4, 8, 8]
