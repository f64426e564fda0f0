"""GPU: lenient verification (SJDConfig.lenience, LOSSY and off by default) in K4 and both engines.

K4 on (p, q, lambda) is BY DEFINITION the exact K4 on (p, q') with q' = fp32(q / lambda) per element, so the kernel is held bit for bit against
itself: the lenient launch on (p, q) and the lambda = 1 launch on (p, q') -- q' divided on the CPU by NumPy, an IEEE fp32 division per element --
with the same state, the same noise (tensors, or the same Philox seed and offsets) must write the same m, rejected, n_prev, tokens and host
mirror.  The cases are the smallest at which the kernel branches: 2 / 16 / 64 rows, a residual row staged in LDS (V = 1024, full-width rule) and
in `scratch` (V = 184622), residual rules with top-k, with a temperature, forced; noise read and generated.  Every case ends in a rejection (the
last draft has p(x) = 0), so the residual resample always runs, at a row the noise picks.
"""
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

V_LDS, V_SCRATCH = 1024, 184622        # residual row of a full-width rule: in the workgroup's LDS (<= 38400 columns) / in `scratch`
SEQ = 4242


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _ops():
    import sjd_amd.ops as ops
    import sjd_amd._lib as L
    L.load()
    return ops, L


def _word(lam, scheme=0):
    from sjd_amd.engine import lenience_field
    return scheme | lenience_field(lam)


# ------------------------------------------------------------------------------------------------ inputs, once per (V, n)
_cache = {}


def _topk_softmax(z, k):
    kth = torch.topk(z, k)[0][..., -1, None]
    return torch.softmax(z.masked_fill(z < kth, -float("inf")), dim=-1)


def _inputs(V, n, dev):
    """target rows p (top-k: exact zeros), draft rows q (even rows full support, odd rows top-k), q[i] a perturbed p[i - 1]; drafts x_i ~ q[i];
    the LAST draft is an id with q > 0 and p = 0: rejected whatever lambda and the noise are.  Device copies are made once and never written."""
    key = (V, n)
    if key in _cache:
        return _cache[key]
    g = torch.Generator().manual_seed(1000 + V % 997 + n)
    k = 500 if V == V_LDS else 2000
    zl = torch.randn(n, V, generator=g) * 3.0
    zq = torch.roll(zl, 1, 0) + torch.randn(n, V, generator=g) * 1.5
    p = _topk_softmax(zl, k)
    q = torch.softmax(zq, dim=-1)
    q[1::2] = _topk_softmax(zq[1::2], k)
    win = torch.multinomial(q, 1, generator=g)[:, 0]
    last = torch.where((q[n - 1] > 0) & (p[n - 2] == 0))[0]
    assert last.numel() > 0
    win[n - 1] = last[int(torch.randint(0, last.numel(), (1,), generator=g))]
    Y = torch.multinomial(p, 1, generator=g)[:, 0]
    rs = torch.rand(n, V, generator=g)
    e2 = torch.empty(V).exponential_(generator=g)
    d = dict(V=V, n=n, p=p.numpy(), q=q.numpy(), win=win.tolist(), Y=Y.tolist(), p_dev=p.to(dev), rs_dev=rs.to(dev), e2_dev=e2.to(dev),
             scratch=torch.empty(V, device=dev), prev={})
    assert d["p"].dtype == np.float32 and d["q"].dtype == np.float32
    _cache[key] = d
    return d


def _prev(d, lam, dev):
    """q' = fp32(q / lam), one IEEE division per element on the CPU (1: q itself), as a device tensor"""
    if lam not in d["prev"]:
        qd = d["q"] if lam == 1.0 else d["q"] / np.float32(lam)
        assert qd.dtype == np.float32
        d["prev"][lam] = torch.from_numpy(np.ascontiguousarray(qd)).to(dev)
    return d["prev"][lam]


RULES = {
    "plain": dict(),
    "top-k": dict(top_k=50),
    "temperature": dict(temperature=0.7),
    "forced": dict(forced=777),
}


def _fill(pv, sv, n, word, rule, win, Y, q_src, philox):
    pv.n_rows, pv.scheme, pv.iter_seq = n, word, SEQ
    for j in range(n):
        pv.resid_rules[j] = rule
    if philox is not None:
        pv.philox_blocks, pv.philox_seed = philox, 20240607
        pv.philox_offset[0], pv.philox_offset[1], pv.philox_offset[2] = 0, 4096, 1 << 20
    for i in range(n):
        sv.win_tok[i], sv.tokens[i], sv.q_src[i] = int(win[i]), int(Y[i]), int(q_src[i])


def _result(view, n, mirror):
    return dict(m=int(view.m), rejected=int(view.rejected), n_prev=int(view.n_prev), tokens=[int(view.tokens[i]) for i in range(n)], mirror=mirror)


def run_k4(dev, d, prev, word, rule_kw, noise, q_src=None, win=None):
    """one launch of the one-slot K4 -> dict(m, rejected, n_prev, tokens, mirror bytes).  noise "tensor": rs / noise2 handed over
    (philox_blocks = 0); "philox": generated in the kernel"""
    ops, L = _ops()
    n, V = d["n"], d["V"]
    params, state = ops.DeviceBlob(L.IterParams, dev), ops.DeviceBlob(L.State, dev)
    philox = ops.philox_max_blocks(dev) if noise == "philox" else None
    _fill(params.view, state.view, n, word, ops.make_rule(**rule_kw), win or d["win"], d["Y"], q_src or list(range(n)), philox)
    params.upload()
    state.dev.copy_(state.host)
    assert prev.shape == d["p_dev"].shape == (n, V)
    rs, e2 = (d["rs_dev"], d["e2_dev"]) if philox is None else (None, None)
    ops.verify_accept(params, state, d["p_dev"], prev, rs, e2, d["scratch"], mirror=True)
    state.wait_mirror(seq=SEQ)                               # (the host spins on the sequence word K4 publishes behind the mirrored state)
    mirror = bytes(state._mirror.numpy().tobytes())
    state.download()
    assert mirror[:state.nbytes] == bytes(state.host.numpy().tobytes()), "K4's host mirror differs from the device state"
    return _result(state.view, n, mirror)


def _same(a, b):
    for k in ("m", "rejected", "n_prev", "tokens", "mirror"):
        assert a[k] == b[k], k


# ------------------------------------------------------------------------------------------------ K4 against itself
CASES = [(V_LDS, n) for n in (2, 16, 64)] + [(V_SCRATCH, 16)]


@pytest.mark.parametrize("noise", ["tensor", "philox"])
@pytest.mark.parametrize("lam", [1.5, 4.0])
@pytest.mark.parametrize("rule", list(RULES))
@pytest.mark.parametrize("V,n", CASES, ids=[f"V{v}-n{n}" for v, n in CASES])
def test_k4_lenient_is_the_exact_kernel_on_q_over_lambda(dev, V, n, rule, lam, noise):
    d = _inputs(V, n, dev)
    lenient = run_k4(dev, d, _prev(d, 1.0, dev), _word(lam), RULES[rule], noise)
    exact = run_k4(dev, d, _prev(d, lam, dev), _word(1.0), RULES[rule], noise)
    _same(lenient, exact)
    assert lenient["n_prev"] == n and 1 <= lenient["m"] < n and lenient["rejected"] == 1      # the last draft has p(x) = 0: the residual row ran
    if rule == "forced":
        assert lenient["tokens"][lenient["m"] - 1] == 777
    else:                                                   # the resampled id has residual mass: p > q / lambda there
        t, row = lenient["tokens"][lenient["m"] - 1], lenient["m"] - 1
        assert d["p"][row, t] > np.float32(d["q"][row + 1, t]) / np.float32(lam)


def test_k4_field_of_zero_and_of_one_are_the_exact_rule(dev):
    """bits 16-31 == 0 and == bf16(1.0) both mean lambda = 1"""
    d = _inputs(V_LDS, 16, dev)
    want = run_k4(dev, d, _prev(d, 1.0, dev), 0, RULES["plain"], "tensor")
    _same(want, run_k4(dev, d, _prev(d, 1.0, dev), 0x3f80 << 16, RULES["plain"], "tensor"))


def test_k4_the_factor_decides_an_accept(dev):
    """p(x) = 0.3, q(x) = 0.9, u = 0.5: 0.5 < 0.3 / 0.9 is false (reject), 0.5 < 2 x 0.3 / 0.9 is true (accept)"""
    ops, L = _ops()
    V, n, x = V_LDS, 2, 321
    p = torch.full((n, V), 0.7 / (V - 1))
    p[:, x] = 0.3
    q = torch.full((n, V), 0.1 / (V - 1))
    q[:, x] = 0.9
    d = dict(V=V, n=n, win=[5, x], Y=[11, 12], p_dev=p.to(dev), rs_dev=torch.full((n, V), 0.5, device=dev), e2_dev=torch.ones(V, device=dev),
             scratch=torch.empty(V, device=dev))
    exact = run_k4(dev, d, q.to(dev), _word(1.0), RULES["plain"], "tensor")
    assert (exact["m"], exact["rejected"]) == (1, 1) and exact["tokens"][0] != x             # the residual max(p - q, 0) is 0 at x
    lenient = run_k4(dev, d, q.to(dev), _word(2.0), RULES["plain"], "tensor")
    assert (lenient["m"], lenient["rejected"]) == (2, 0) and lenient["tokens"] == [x, 12]
    jacobi = run_k4(dev, d, q.to(dev), _word(1.0, scheme=1) | (0x4000 << 16), RULES["plain"], "tensor")      # scheme 1 ignores the field
    assert (jacobi["m"], jacobi["rejected"]) == (1, 0)


@pytest.mark.parametrize("noise", ["tensor", "philox"])
@pytest.mark.parametrize("lam", [1.5, 4.0])
@pytest.mark.parametrize("V", [V_LDS, V_SCRATCH])
def test_k4_implicit_one_hot_is_one_over_lambda_at_x(dev, V, lam, noise):
    """rows with q_src < 0 (fresh random drafts): the lenient kernel on the implicit one-hot == the lenient kernel on an explicit one-hot row"""
    n = 16
    d = _inputs(V, n, dev)
    g = torch.Generator().manual_seed(77)
    win = list(d["win"])
    fresh = [i for i in range(1, n) if i % 3 != 1]                                    # a mix of carried and fresh drafts, the last one fresh
    for i in fresh[:-1]:
        win[i] = int(torch.multinomial(torch.from_numpy(d["p"][i - 1]), 1, generator=g))      # p(x) > 0: accepted with min(1, lambda p(x))
    assert n - 1 in fresh and d["p"][n - 2, win[n - 1]] == 0
    explicit = _prev(d, 1.0, dev).clone()
    for i in fresh:
        explicit[i].zero_()
        explicit[i, win[i]] = 1.0
    q_src = [-1 if i in fresh else i for i in range(n)]
    for rule in ("plain", "top-k"):
        a = run_k4(dev, d, _prev(d, 1.0, dev), _word(lam), RULES[rule], noise, q_src=q_src, win=win)
        b = run_k4(dev, d, explicit, _word(lam), RULES[rule], noise, win=win)
        for k in ("m", "rejected", "n_prev", "tokens"):                                # (the mirrors differ in q_src, which is the point)
            assert a[k] == b[k], k
        assert a["rejected"] == 1


@pytest.mark.parametrize("V,ns", [(V_LDS, (2, 16, 64)), (V_SCRATCH, (2, 16, 16))], ids=["lds", "scratch"])
def test_k4_slots_each_slot_reads_its_own_factor(dev, V, ns):
    """sjd_verify_accept_slots, three slots whose blobs carry lambda = 1, 1.5, 4: every slot == its one-slot launch"""
    ops, L = _ops()
    lams, P, Lw = (1.0, 1.5, 4.0), 3, max(ns)
    params, state = ops.BlobArray(L.IterParams, P, dev), ops.BlobArray(L.State, P, dev)
    probs = torch.zeros(P, 2, Lw, V, device=dev)
    scratch = torch.empty(P, V, device=dev)
    zero_state = torch.full((P, 2, Lw, 2), -1, dtype=torch.int32, device=dev)
    blocks = ops.philox_max_blocks(dev)                      # (the slots form generates its noise: it has no tensor arguments)
    ds = [_inputs(V, n, dev) for n in ns]
    for s, (d, lam) in enumerate(zip(ds, lams)):
        probs[s, 0, :d["n"]] = d["p_dev"]
        probs[s, 1, :d["n"]] = _prev(d, 1.0, dev)
        _fill(params.blobs[s].view, state.blobs[s].view, d["n"], _word(lam), ops.make_rule(**RULES["top-k"]), d["win"], d["Y"], list(range(d["n"])), blocks)
    sl = ops.slots_of(params, state, probs, zero_state, scratch, 2)
    params.upload()
    state.dev.copy_(state.host)
    ops.verify_accept_slots(sl, params, state, probs, 0, scratch)
    state.wait_mirror()
    for s, (d, lam) in enumerate(zip(ds, lams)):
        got = _result(state.blobs[s].view, d["n"], None)
        one = run_k4(dev, d, _prev(d, 1.0, dev), _word(lam), RULES["top-k"], "philox")
        for k in ("m", "rejected", "n_prev", "tokens"):
            assert got[k] == one[k], (s, k)
        assert bytes(state.blobs[s].host.numpy().tobytes()) == one["mirror"][:state.nbytes], f"slot {s}: mirrored state"
        _same(one, run_k4(dev, d, _prev(d, lam, dev), _word(1.0), RULES["top-k"], "philox"))


# ------------------------------------------------------------------------------------------------ the limit
@pytest.mark.parametrize("noise", ["tensor", "philox"])
@pytest.mark.parametrize("n", [2, 16, 64])
def test_k4_huge_factor_accepts_every_draft_with_target_mass(dev, n, noise):
    """lambda = 2^100: min(1, lambda p / q) = 1 wherever p(x) > 0.  p strictly positive, every drafted q(x) >= 2^-20 (q' = q 2^-100 stays a normal
    fp32, p / q' neither underflows nor overflows): checked here on the CPU, then m == n on the GPU"""
    V, lam = V_LDS, 2.0 ** 100
    g = torch.Generator().manual_seed(31 + n)
    p = torch.softmax(torch.randn(n, V, generator=g) * 3.0, -1)
    q = torch.softmax(torch.randn(n, V, generator=g) * 3.0, -1)
    win = torch.zeros(n, dtype=torch.long)
    q_src = list(range(n))
    for i in range(1, n):
        ok = torch.where(q[i] >= 2.0 ** -20)[0]
        win[i] = ok[int(torch.randint(0, ok.numel(), (1,), generator=g))]
        if i % 4 == 3:                                       # some fresh drafts: q' = 2^-100 at x
            q_src[i] = -1
    pn, qn, w = p.numpy(), q.numpy(), win.tolist()
    assert (pn > 0).all()
    for i in range(1, n):
        qd = np.float32(1.0) if q_src[i] < 0 else qn[i, w[i]]
        assert qd >= np.float32(2.0 ** -20)
        qp = qd / np.float32(lam)
        ratio = pn[i - 1, w[i]] / qp
        assert qp >= np.finfo(np.float32).tiny and np.isfinite(ratio) and ratio >= 1.0
    d = dict(V=V, n=n, win=win.tolist(), Y=torch.multinomial(p, 1, generator=g)[:, 0].tolist(), p_dev=p.to(dev),
             rs_dev=torch.rand(n, V, generator=g).to(dev), e2_dev=torch.ones(V, device=dev), scratch=torch.empty(V, device=dev))
    got = run_k4(dev, d, q.to(dev), _word(lam), RULES["plain"], noise, q_src=q_src)
    assert (got["m"], got["rejected"], got["n_prev"]) == (n, 0, n)
    assert got["tokens"][:n - 1] == d["win"][1:] and got["tokens"][n - 1] == d["Y"][n - 1]       # every draft emitted, the last sample carried


# ------------------------------------------------------------------------------------------------ the engines, on a toy backbone
HG = WG = 4
N_IMG = (2 * WG + 1) * 2 * HG
P_LENS = (12, 9)
WINDOW, TOY_V, SEED = 16, 9216, 3
_toy = {}


def _model(dev):
    from tests.helpers import make_chameleon
    ops, _ = _ops()
    if "model" not in _toy:
        conf = dict(vocab_size=TOY_V, hidden_size=512, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
                    max_position_embeddings=512, rms_norm_eps=1e-5, rope_theta=10000.0)
        m = make_chameleon(conf, 23, 0.25, ops.HipWindowAttention(n_split=2), dtype=torch.bfloat16, device=dev)
        m.enable_fused(ops, gemm="sjd")
        _toy["model"] = m
    return _toy["model"]


def _prompt(j, dev):
    import sjd_amd.synthetic as synthetic
    from sjd_amd.engine import WindowSpec
    Pj = P_LENS[j]
    pr = torch.cat([synthetic.synthetic_prompt(Pj - 3, SEED + 17 * j, lo=8900, hi=9200), torch.tensor([[8197, 8804 + HG, 8804 + WG]])], dim=1)
    spec = WindowSpec(first_tokens=pr.to(dev).repeat(2, 1), first_positions=torch.stack([torch.arange(Pj), torch.tensor([1] * (Pj - 1) + [0])]).to(dev),
                      key_start=torch.tensor([0, Pj - 1], dtype=torch.int32), pos_offset=torch.tensor([0, -(Pj - 1)], dtype=torch.long), kv_base=0)
    return pr[0].tolist(), spec


def _config(**kw):
    from sjd_amd.engine import SJDConfig
    return SJDConfig(jacobi_loop_interval_l=3, jacobi_loop_interval_r=N_IMG - 10, max_num_new_tokens=WINDOW, guidance_scale=3.0, seed=SEED,
                     max_length=1 << 20, eos_token_ids=(8196,), **kw)


S_MAX = ((max(P_LENS) + N_IMG + 5 + 64 + 31) // 32) * 32


def _solo(dev, j, key, **kw):
    """prompt j alone through SJDEngine, with the seed decode_many gives it (cfg.seed + j); computed once per (j, key)"""
    from sjd_amd.engine import SJDEngine
    from sjd_amd.grammar import LuminaGrammar
    if ("solo", j, key) not in _toy:
        model = _model(dev)
        model.setup_cache(batch=2, s_max=S_MAX)
        eng = SJDEngine(model, TOY_V, dev, max_window=WINDOW, use_graph=True)
        prompt, spec = _prompt(j, dev)
        cfg = _config(**kw)
        seq, stats = eng.decode(prompt, spec, LuminaGrammar(2000, 10), dataclasses.replace(cfg, seed=cfg.seed + j))
        _toy["solo", j, key] = (seq, list(stats.matched), bool(torch.isfinite(eng.probs).all()), len(prompt))
    return _toy["solo", j, key]


def _batch(dev, key, **kw):
    from sjd_amd.engine_batch import SJDBatchEngine
    from sjd_amd.grammar import LuminaGrammar
    if ("batch", key) not in _toy:
        model = _model(dev)
        model.setup_cache(batch=4, s_max=S_MAX)
        eng = SJDBatchEngine(model, TOY_V, dev, 2, max_window=WINDOW, use_graph=True)
        ps = [_prompt(j, dev) for j in range(2)]
        res = eng.decode_many([p for p, _ in ps], [s for _, s in ps], [LuminaGrammar(2000, 10) for _ in range(2)], _config(**kw))
        _toy["batch", key] = ([(seq, list(st.matched)) for seq, st in res], bool(torch.isfinite(eng.probs_all).all()))
    return _toy["batch", key]


def test_engines_lenience_one_is_the_config_that_never_sets_the_field(dev):
    never, one = _solo(dev, 0, "never"), _solo(dev, 0, 1.0, lenience=1.0)
    assert never[:2] == one[:2] and never[0][-1] == 8196
    never, one = _batch(dev, "never"), _batch(dev, 1.0, lenience=1.0)
    assert never[0] == one[0] and all(seq[-1] == 8196 for seq, _ in never[0])


def test_engines_lenience_two_decodes_to_the_end_token(dev):
    seq, matched, finite, P = _solo(dev, 0, 2.0, lenience=2.0)
    assert seq[-1] == 8196 and 8196 not in seq[P:-1] and finite
    res, finite = _batch(dev, 2.0, lenience=2.0)
    assert finite
    for j, (s, _) in enumerate(res):
        assert s[-1] == 8196 and 8196 not in s[P_LENS[j]:-1]
    exact = _solo(dev, 0, 1.0, lenience=1.0)
    assert len(seq) == len(exact[0])                         # the grammar fixes the image's length: the same number of tokens, in fewer or as many forwards
    print(f"toy backbone, prompt 0: {len(exact[1])} forwards at lenience 1, {len(matched)} at lenience 2 (synthetic weights: no statement about quality)")


@pytest.mark.parametrize("lam", [1.0, 2.0])
def test_decode_many_prompt_equals_its_solo_run(dev, lam):
    res, _ = _batch(dev, lam, lenience=lam)
    for j in range(2):
        seq, matched, _, _ = _solo(dev, j, lam, lenience=lam)
        assert res[j][0] == seq, f"prompt {j}: token sequences differ"
        assert res[j][1] == matched, f"prompt {j}: accept lengths differ"
