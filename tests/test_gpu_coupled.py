"""GPU: coupled Jacobi decoding (prefix_token_sampler_scheme="coupled_jacobi", scheme code 2) -- K2's position-keyed noise, K4, both engines.

K2 in scheme 2 is held bit for bit against the kernel it extends: window row j at position t = kv_len + j must give the token, the fp32
probabilities and the mode that ONE-row launches of the scheme-0 K2 give on the same logits row with the generator at base + t * stride.  Nothing
has a tolerance.  The engines are replayed through the NumPy model of the loop (tests/coupled_model.py) with the noise sjd_philox_fill writes at the
per-position offsets."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

from tests import coupled_model as CM

pytestmark = pytest.mark.gpu

SEED, BASE = 20240607, 4 * 1000003         # (a base far from 0: the 64-bit offset arithmetic is exercised, a multiple of 4 as every torch offset)
LW = 16


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


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. the row-keyed draw
SHAPES = {"V8192": (8192, ()), "V65536-range": (65536, ((4, 8196),)), "V5003": (5003, ())}      # 5003: no multiple of 4 (scalar loads, unaligned rows)
_logits = {}


def _rows(shape, dev):
    """[2, LW, V] fp32 logits (cond, uncond), made once per shape and never written"""
    if shape not in _logits:
        V, _ = SHAPES[shape]
        g = torch.Generator().manual_seed(11 + V)
        _logits[shape] = (torch.randn(2, LW, V, generator=g) * 0.6).to(dev)        # (guided scores of std ~2: no row is a near one-hot)
    return _logits[shape]


def _rules(shape, n):
    """top-k 2000, top-p, a temperature with a top-k, and a forced row (row 2), cycling"""
    ops, _ = _ops()
    V, ranges = SHAPES[shape]
    kinds = [dict(top_k=2000), dict(top_p=0.9), dict(forced=(ranges[0][0] + 77) if ranges else 321), dict(top_k=500, temperature=0.7), dict(top_k=2000, top_p=0.95)]
    return [ops.make_rule(ranges=ranges, **kinds[j % len(kinds)]) for j in range(n)]


def _fill(pv, n, kv_len, use_cfg, scheme, rules, blocks, seed, off0, off1):
    pv.n_rows, pv.kv_len, pv.use_cfg, pv.scheme, pv.philox_blocks, pv.philox_seed = n, kv_len, int(use_cfg), scheme, blocks, seed
    pv.philox_offset[0], pv.philox_offset[1], pv.philox_offset[2] = off0, off1, 0
    for j, r in enumerate(rules):
        pv.rules[j] = r


_heads = {}


def _head(lg):
    """dense logits [2 k, rows, V] (cond, uncond of k prompts) -> an ops.HeadOut whose two fp32 planes sum to them exactly (plane 0: the
    bf16-rounded value, plane 1: the rest): partial rows in that order, the column window the whole vocabulary; made once per tensor"""
    ops, _ = _ops()
    key = (lg.data_ptr(), tuple(lg.shape))
    if key not in _heads:
        B, rows, V = lg.shape
        flat = lg.reshape(B * rows, V)
        prows = ((B * rows + 31) // 32) * 32
        data = torch.zeros(2, prows, V, dtype=torch.float32, device=lg.device)
        hi = flat.to(torch.bfloat16).float()
        data[0, :B * rows], data[1, :B * rows] = hi, flat - hi
        assert torch.equal(data[0, :B * rows] + data[1, :B * rows], flat)
        _heads[key] = (ops.HeadOut(ops.Partials(data, 2, V), 0, rows, torch.float32), lg)      # (the tensor is kept: its address is the key)
    return _heads[key][0]


def _k2(form, dev, lg, n, kv_len, use_cfg, scheme, rules, off0, off1, guidance=3.0, seed=SEED, row0=0, out_rows=LW):
    """one K2 launch over rows [row0, row0 + out_rows) of `lg` -> (tokens, probs, amax) of its first n rows"""
    ops, L = _ops()
    V = lg.shape[-1]
    params = ops.DeviceBlob(L.IterParams, dev)
    _fill(params.view, n, kv_len, use_cfg, scheme, rules, ops.philox_max_blocks(dev), seed, off0, off1)
    params.upload()
    probs = torch.full((out_rows, V), float("nan"), device=dev)
    tok = torch.full((out_rows,), -1, dtype=torch.int64, device=dev)
    am = torch.full((out_rows,), -1, dtype=torch.int64, device=dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    if form == "dense":
        ops.logits_to_probs_sample(lg[0, row0:row0 + out_rows], lg[1, row0:row0 + out_rows], guidance, params, None, probs, vp(tok), amax_out_ptr=vp(am))
    else:
        ops.logits_to_probs_sample_part(_head(lg), guidance, params, None, probs, vp(tok), amax_out_ptr=vp(am), row0=row0, urow_off=lg.shape[1])
    torch.cuda.synchronize()
    return tok[:n].clone(), probs[:n].clone(), am[:n].clone()


def _reference(form, dev, lg, n, kv_len, use_cfg, rules, stride, guidance=3.0, seed=SEED, base=BASE):
    """row j as a ONE-row launch of today's scheme-0 K2 with the generator at base + (kv_len + j) * stride"""
    out = [_k2(form, dev, lg, 1, 0, use_cfg, 0, [rules[j]], base + (kv_len + j) * stride, 0, guidance, seed, row0=j, out_rows=1) for j in range(n)]
    return tuple(torch.cat([o[i] for o in out]) for i in range(3))


def _same(got, want, what=""):
    assert torch.equal(got[0], want[0]), f"{what}: tokens {got[0].tolist()} != {want[0].tolist()}"
    assert torch.equal(_bits(got[1]), _bits(want[1])), f"{what}: probability bits"
    assert torch.equal(got[2], want[2]), f"{what}: amax"


@pytest.mark.parametrize("use_cfg", [True, False], ids=["cfg", "nocfg"])
@pytest.mark.parametrize("kv_len", [0, 77])
@pytest.mark.parametrize("n", [1, 5, 16])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("form", ["dense", "part"])
def test_k2_row_keyed_draw(dev, form, shape, n, kv_len, use_cfg):
    ops, _ = _ops()
    lg, rules = _rows(shape, dev), _rules(shape, n)
    stride = ops.philox_step(lg.shape[-1], ops.philox_max_blocks(dev))
    got = _k2(form, dev, lg, n, kv_len, use_cfg, 2, rules, BASE, stride)
    want = _reference(form, dev, lg, n, kv_len, use_cfg, rules, stride)
    _same(got, want, f"{form} {shape} n={n} kv_len={kv_len}")
    assert bool(torch.isfinite(got[1]).all()) and (got[0] >= 0).all()
    if n > 2:
        assert int(got[0][2]) == rules[2].forced


@pytest.mark.parametrize("shape", ["V8192", "V65536-range"])
def test_k2_slots_each_slot_reads_its_own_blob(dev, shape):
    """sjd_logits_to_probs_sample_part_slots_g, two slots: seed, base, kv_len, row count and guidance scale all differ"""
    ops, L = _ops()
    lg = _rows(shape, dev)
    V = lg.shape[-1]
    stride = ops.philox_step(V, ops.philox_max_blocks(dev))
    P, nb = 2, 2
    slots = [dict(seed=SEED, base=BASE, kv_len=77, n=16, g=3.0), dict(seed=SEED + 5, base=BASE + 4096, kv_len=3, n=5, g=1.5)]
    lgs = [lg, torch.flip(lg, dims=(1,)).contiguous()]                         # slot 1: the rows in reverse order
    params, state = ops.BlobArray(L.IterParams, P, dev), ops.BlobArray(L.State, P, dev)
    probs = torch.full((P, 2, LW, V), float("nan"), device=dev)
    zero_state = torch.full((P, 2, LW, 2), -1, dtype=torch.int32, device=dev)
    scratch = torch.empty(P, V, device=dev)
    rules = [_rules(shape, s["n"]) for s in slots]
    for i, s in enumerate(slots):
        _fill(params.blobs[i].view, s["n"], s["kv_len"], True, 2, rules[i], ops.philox_max_blocks(dev), s["seed"], s["base"], stride)
        params.blobs[i].view.batch_rows = nb
    params.upload()
    head = _head(torch.cat(lgs))                                      # partial rows: slot 0 cond, slot 0 uncond, slot 1 cond, slot 1 uncond
    sl = ops.slots_of(params, state, probs, zero_state, scratch, nb)
    guid = torch.tensor([s["g"] for s in slots], dtype=torch.float32, device=dev)
    ops.logits_to_probs_sample_part_slots(sl, head, guid, params, probs, 0, "tokens", "amax", state, zero_state, nb)
    torch.cuda.synchronize()
    state.download()
    for i, s in enumerate(slots):
        n, st = s["n"], state.blobs[i].view
        got = (torch.tensor(list(st.tokens[:n]), device=dev), probs[i, 0, :n], torch.tensor(list(st.amax[:n]), device=dev))
        want = _reference("part", dev, lgs[i], n, s["kv_len"], True, rules[i], stride, guidance=s["g"], seed=s["seed"], base=s["base"])
        _same(got, want, f"slot {i}")
    assert not torch.equal(probs[0, 0, :5], probs[1, 0, :5])


def test_k2_graph_replay_into_poisoned_outputs(dev):
    ops, L = _ops()
    shape, n, kv_len = "V65536-range", 16, 77
    lg, rules = _rows(shape, dev), _rules(shape, n)
    V = lg.shape[-1]
    stride = ops.philox_step(V, ops.philox_max_blocks(dev))
    params = ops.DeviceBlob(L.IterParams, dev)
    _fill(params.view, n, kv_len, True, 2, rules, ops.philox_max_blocks(dev), SEED, BASE, stride)
    params.upload()
    probs = torch.zeros(LW, V, device=dev)
    tok, am = torch.zeros(LW, dtype=torch.int64, device=dev), torch.zeros(LW, dtype=torch.int64, device=dev)
    launch = lambda: ops.logits_to_probs_sample(lg[0], lg[1], 3.0, params, None, probs, ctypes.c_void_p(tok.data_ptr()), amax_out_ptr=ctypes.c_void_p(am.data_ptr()))
    launch()                                                          # eager warm-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        launch()
    want = _reference("dense", dev, lg, n, kv_len, True, rules, stride)
    for kv in (kv_len, 5):                                            # the second replay: the blob changed under the captured launch, as in a decode
        params.view.kv_len = kv
        params.upload()
        probs.fill_(float("nan"))
        tok.fill_(-7)
        am.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        if kv != kv_len:
            want = _reference("dense", dev, lg, n, kv, True, rules, stride)
        _same((tok[:n], probs[:n], am[:n]), want, f"replay kv_len={kv}")


# ------------------------------------------------------------------------------------------------ 2. same position, same token
def test_same_position_same_token(dev):
    ops, _ = _ops()
    V = 8192
    by_pos = (torch.randn(2, 16, V, generator=torch.Generator().manual_seed(5)) * 0.5).to(dev)      # positions 40 .. 55
    stride = ops.philox_step(V, ops.philox_max_blocks(dev))
    rule = ops.make_rule(top_k=2000)
    later = torch.zeros_like(by_pos)
    later[:, :11] = by_pos[:, 5:]                                     # the launch at kv_len 45: rows 0 .. 10 are positions 45 .. 55
    for form in ("dense", "part"):
        a = _k2(form, dev, by_pos, 16, 40, True, 2, [rule] * 16, BASE, stride)
        b = _k2(form, dev, later, 11, 45, True, 2, [rule] * 11, BASE, stride)
        assert torch.equal(a[0][5:], b[0]) and torch.equal(_bits(a[1][5:]), _bits(b[1])) and torch.equal(a[2][5:], b[2])
        # today's per-launch noise on the same inputs: the same distributions, other tokens -- a draft matches its re-sample by luck only
        a0 = _k2(form, dev, by_pos, 16, 40, True, 0, [rule] * 16, BASE, stride)
        b0 = _k2(form, dev, later, 11, 45, True, 0, [rule] * 11, BASE, stride)
        assert torch.equal(_bits(a0[1][5:]), _bits(b0[1])) and torch.equal(_bits(a0[1]), _bits(a[1]))
        assert not torch.equal(a0[0][5:], b0[0])


# ------------------------------------------------------------------------------------------------ 3. K4
K4_CASES = {"accept all": (8, None), "reject at row 1": (8, 1), "reject mid-window": (16, 7), "n = 1": (1, None)}


@pytest.mark.parametrize("lenience_bits", [0, 0x4000], ids=["plain", "lenience bits set"])
@pytest.mark.parametrize("case", list(K4_CASES))
def test_k4_is_scheme_1(dev, case, lenience_bits):
    ops, L = _ops()
    n, reject = K4_CASES[case]
    V, seq = 1024, 99
    g = torch.Generator().manual_seed(3 + n)
    p = torch.softmax(torch.randn(LW, V, generator=g), -1).to(dev)
    q = torch.softmax(torch.randn(LW, V, generator=g), -1).to(dev)
    Y = torch.randint(0, V, (LW,), generator=g).tolist()
    win = [17] + Y[:LW - 1]                                           # every draft equals the sample of the row before it
    if reject is not None:
        win[reject] = (Y[reject - 1] + 1) % V
    out = {}
    for scheme in (1, 2):
        params, state = ops.DeviceBlob(L.IterParams, dev), ops.DeviceBlob(L.State, dev)
        pv, sv = params.view, state.view
        pv.n_rows, pv.scheme, pv.iter_seq, pv.philox_blocks, pv.philox_seed = n, scheme | (lenience_bits << 16), seq, ops.philox_max_blocks(dev), SEED
        pv.philox_offset[0], pv.philox_offset[1], pv.philox_offset[2] = BASE, 12, 0
        for j in range(LW):
            pv.resid_rules[j] = ops.make_rule(top_k=50)
            sv.win_tok[j], sv.tokens[j], sv.q_src[j] = win[j], Y[j], j
        sv.m, sv.rejected, sv.n_prev = -5, -5, -5
        params.upload()
        state.dev.copy_(state.host)
        pc, qc = p.clone(), q.clone()
        ops.verify_accept(params, state, pc, qc, None, None, torch.empty(V, device=dev), mirror=True)
        state.wait_mirror(seq=seq)
        mirror = bytes(state._mirror.numpy().tobytes())
        state.download()
        assert mirror[:state.nbytes] == bytes(state.host.numpy().tobytes())
        assert torch.equal(_bits(pc), _bits(p)) and torch.equal(_bits(qc), _bits(q))      # the probability buffers are read only
        out[scheme] = (mirror, int(sv.m), int(sv.rejected), int(sv.n_prev), [int(sv.tokens[j]) for j in range(LW)])
    assert out[1] == out[2]
    _, m, rejected, n_prev, tokens = out[2]
    assert (m, rejected, n_prev) == ((n if reject is None else reject) if n > 1 else 1, 0, n) and tokens == Y      # no residual, no token rewritten


# ------------------------------------------------------------------------------------------------ 4. the engines, teacher-forced
class _Rec:
    """the engines' hook: per iteration the distributions K2 wrote, the tokens it drew and K4's accept count (read from the device state once the
    iteration's kernels are done), and -- iteration 0 -- the observer noise of the first-token draw"""

    def __init__(self, state_of):
        self.state_of, self.items = state_of, {}

    def __call__(self, *a):
        j, d = (0, a[0]) if len(a) == 1 else a
        n = d["n_rows"]
        st = self.state_of(j).download()
        self.items.setdefault(j, []).append(dict(first=d["first"], n=n, ctx=list(d["ctx"]), probs=d["probs"][:n].cpu().numpy().copy(),
                                                noise=d["noise"][:n].cpu().numpy().copy(), tokens=[int(st.tokens[i]) for i in range(n)], m=int(st.m),
                                                scheme=d["scheme"]))


def _replay(dev, items, prompt, seq, matched, cfg, seed, kv_base, V, fresh_gen):
    """the recorded iterations of ONE prompt through the NumPy loop; the noise of window row j is what sjd_philox_fill writes for a [1, V]
    exponential at base + (kv_len + j) * stride, base = the generator's offset behind the first-token draw"""
    ops, _ = _ops()
    stride = ops.philox_step(V, ops.philox_max_blocks(dev))
    base = stride                                                     # a freshly seeded generator (offset 0) plus the prefill's [1, V] draw
    fresh = lambda k: (cfg.img_vocab_lo + torch.randint(0, cfg.img_vocab_n, (1, k), generator=fresh_gen)[0]).tolist()
    model = CM.CoupledReplay(prompt, fresh, eos=cfg.eos_token_ids, max_length=cfg.max_length)
    kv_len = kv_base
    for it in items:
        assert it["ctx"] == model.X and it["scheme"] == 2
        n = it["n"]
        if it["first"]:
            noise = it["noise"]                                       # the first draw is the per-launch draw of every scheme
            expect = ops.philox_fill(V, seed, 0, dev).cpu().numpy()[None]
        else:
            noise = np.stack([ops.philox_fill(V, seed, base + (kv_len + j) * stride, dev).cpu().numpy() for j in range(n)])
            expect = noise
        assert (it["noise"] == expect).all(), "the observers' noise is not the per-position noise"
        win, Y, m = model.step(n, it["probs"], noise)
        assert Y == it["tokens"], f"kv_len {kv_len}: drawn tokens differ"
        if n > 1:
            assert m == it["m"], f"kv_len {kv_len}: accept count"
        kv_len += len(prompt) if it["first"] else m
    assert model.X == seq and model.matched == matched and model.finished
    return model


_toy = {}
HG = WG = 4
N_IMG = (2 * WG + 1) * 2 * HG
P_LENS = (12, 9)
TOY_V, TOY_SEED = 9216, 3


def _lumina(dev):
    from tests.helpers import make_chameleon
    ops, _ = _ops()
    if "lumina" not in _toy:                                          # the toy Lumina backbone of tests/gpu_loop_check.py
        conf = dict(vocab_size=TOY_V, hidden_size=512, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
                    max_position_embeddings=512, rms_norm_eps=1e-5, rope_theta=10000.0)
        m = make_chameleon(conf, 23, 0.25, ops.HipWindowAttention(n_split=2), dtype=torch.bfloat16, device=dev)
        m.enable_fused(ops, gemm="sjd")
        _toy["lumina"] = m
    return _toy["lumina"]


def _lumina_prompt(j, dev):
    import sjd_amd.synthetic as synthetic
    from sjd_amd.engine import WindowSpec
    Pj = P_LENS[j]
    pr = torch.cat([synthetic.synthetic_prompt(Pj - 3, TOY_SEED + 17 * j, lo=8900, hi=9200), torch.tensor([[8197, 8804 + HG, 8804 + WG]])], dim=1)
    spec = WindowSpec(first_tokens=pr.to(dev).repeat(2, 1), first_positions=torch.stack([torch.arange(Pj), torch.tensor([1] * (Pj - 1) + [0])]).to(dev),
                      key_start=torch.tensor([0, Pj - 1], dtype=torch.int32), pos_offset=torch.tensor([0, -(Pj - 1)], dtype=torch.long), kv_base=0)
    return pr[0].tolist(), spec


def _lumina_cfg(window=16, scheme="coupled_jacobi"):
    from sjd_amd.engine import SJDConfig
    return SJDConfig(jacobi_loop_interval_l=3, jacobi_loop_interval_r=N_IMG - 10, max_num_new_tokens=window, guidance_scale=3.0, seed=TOY_SEED,
                     max_length=1 << 20, eos_token_ids=(8196,), prefix_token_sampler_scheme=scheme)


S_MAX = ((max(P_LENS) + N_IMG + 5 + 64 + 31) // 32) * 32


def _lumina_solo(dev, j, window=16, record=True):
    from sjd_amd.engine import SJDEngine
    from sjd_amd.grammar import LuminaGrammar
    key = ("solo", j, window)
    if key not in _toy:
        model = _lumina(dev)
        model.setup_cache(batch=2, s_max=S_MAX)
        eng = SJDEngine(model, TOY_V, dev, max_window=window, use_graph=True)
        rec = _Rec(lambda _j: eng.state)
        if record:
            eng.hook = rec
        prompt, spec = _lumina_prompt(j, dev)
        cfg = dataclasses.replace(_lumina_cfg(window), seed=TOY_SEED + j)
        seq, stats = eng.decode(prompt, spec, LuminaGrammar(2000, 10), cfg)
        _toy[key] = (prompt, seq, list(stats.matched), rec.items.get(0), cfg)
    return _toy[key]


def test_engine_lumina_solo_replays_through_the_model(dev):
    prompt, seq, matched, items, cfg = _lumina_solo(dev, 0)
    assert seq[-1] == 8196 and len(items) == len(matched)
    _replay(dev, items, prompt, seq, matched, cfg, cfg.seed, 0, TOY_V, torch.Generator().manual_seed(cfg.seed))
    assert max(matched[1:]) > 1, "no draft was ever accepted: the scheme would be plain Jacobi under fresh noise"


def test_engine_lumina_batch_replays_and_equals_solo(dev):
    from sjd_amd.engine_batch import SJDBatchEngine
    from sjd_amd.grammar import LuminaGrammar
    model = _lumina(dev)
    model.setup_cache(batch=4, s_max=S_MAX)
    eng = SJDBatchEngine(model, TOY_V, dev, 2, max_window=16, use_graph=True)
    rec = _Rec(lambda j: next(s for s in eng.slots if s.prompt_index == j).state)
    eng.hook = rec
    ps = [_lumina_prompt(j, dev) for j in range(2)]
    cfg = _lumina_cfg()
    res = eng.decode_many([p for p, _ in ps], [s for _, s in ps], [LuminaGrammar(2000, 10) for _ in range(2)], cfg)
    for j, (seq, st) in enumerate(res):
        _replay(dev, rec.items[j], ps[j][0], seq, list(st.matched), cfg, cfg.seed + j, 0, TOY_V, torch.Generator().manual_seed(cfg.seed + j))
        _, solo_seq, solo_matched, _, _ = _lumina_solo(dev, j)
        assert seq == solo_seq, f"prompt {j}: the batch decodes other tokens than the prompt alone"
        assert list(st.matched) == solo_matched, f"prompt {j}: accept counts"


def test_engine_llamagen_solo_and_batch(dev):
    """the toy LlamaGen backbone of tests/gpu_loop_check.py: one prompt through SJDEngine, two through SJDBatchEngine (the first token of each
    given, so that both engines start from the same context)"""
    import sjd_amd.ops as ops
    from sjd_amd.engine import SJDConfig, SJDEngine, WindowSpec
    from sjd_amd.engine_batch import SJDBatchEngine
    from sjd_amd.grammar import TopKTopPGrammar
    from tests.helpers import make_llamagen
    latent, window, V, T = 8, 8, 16384, 1
    N = latent * latent
    args = dict(dim=128, n_layer=2, n_head=2, vocab_size=V, block_size=N, cls_token_num=1, model_type="c2i", num_classes=1000)
    model = make_llamagen(args, 17, 0.25, ops.HipWindowAttention(n_split=2), dtype=torch.bfloat16, device=dev)
    model.enable_fused(ops, gemm="sjd", max_rows=64)
    s_max = ((T + N + 64 + 31) // 32) * 32
    zeros = torch.zeros(2, dtype=torch.int32, device=dev)
    cfg = SJDConfig(jacobi_loop_interval_l=1, jacobi_loop_interval_r=N - window - 2, max_num_new_tokens=window, guidance_scale=4.0, seed=7,
                    prefix_token_sampler_scheme="coupled_jacobi", max_length=N, img_vocab_lo=0, img_vocab_n=V)
    firsts, labels = [1234, 4321], [207, 3]

    def prefill(rows, label):
        if hasattr(model.attn, "params"):
            model.attn.params = None                                  # (kv_len by value, as LlamaGenSolver.prefill)
        cond = torch.tensor([label, model.num_classes], device=dev)
        model.forward_embeds(model.embed_condition(cond), torch.zeros(2, 1, dtype=torch.long, device=dev), 0, zeros)

    def spec(first):
        return WindowSpec(first_tokens=torch.tensor([[first], [first]], device=dev), first_positions=torch.full((2, 1), T, dtype=torch.long, device=dev),
                          key_start=zeros, pos_offset=torch.zeros(2, dtype=torch.long), kv_base=T)
    solo = []
    for j in range(2):
        model.setup_cache(batch=2, s_max=s_max)
        prefill(2, labels[j])
        eng = SJDEngine(model, V, dev, max_window=window, use_graph=True)
        rec = _Rec(lambda _j: eng.state)
        eng.hook = rec
        c = dataclasses.replace(cfg, seed=cfg.seed + j)
        seq, stats = eng.decode([firsts[j]], spec(firsts[j]), TopKTopPGrammar(1000, 1.0), c)
        assert len(seq) == N
        _replay(dev, rec.items[0], [firsts[j]], seq, list(stats.matched), c, c.seed, T, V, torch.Generator().manual_seed(c.seed))
        solo.append((seq, list(stats.matched)))
    model.setup_cache(batch=4, s_max=s_max)
    for j in range(2):                                                # every slot's conditioning row, through a view of its batch rows
        from sjd_amd.engine_batch import _CacheView
        full = model.cache
        model.cache = _CacheView(full, 2 * j, 2 * j + 2)
        try:
            prefill(2, labels[j])
        finally:
            model.cache = full
    eng = SJDBatchEngine(model, V, dev, 2, max_window=window, use_graph=True)
    rec = _Rec(lambda j: next(s for s in eng.slots if s.prompt_index == j).state)
    eng.hook = rec
    res = eng.decode_many([[f] for f in firsts], [spec(f) for f in firsts], [TopKTopPGrammar(1000, 1.0) for _ in range(2)], cfg)
    for j, (seq, st) in enumerate(res):
        _replay(dev, rec.items[j], [firsts[j]], seq, list(st.matched), cfg, cfg.seed + j, T, V, torch.Generator().manual_seed(cfg.seed + j))
        assert (seq, list(st.matched)) == solo[j], f"prompt {j}: the batch decodes other tokens than the prompt alone"


# ------------------------------------------------------------------------------------------------ 5. window invariance, end to end
STUB_V, STUB_P, STUB_N = 1024, 4, 72


class _Stub:
    """a first-order model on the dense-logits path: logits = table[input token] + row[position] -- a row has the same bits wherever it stands in
    a window, which the 16-bit kernels of a transformer do not promise between row counts"""

    def __init__(self, dev):
        g = torch.Generator().manual_seed(41)
        # (the position's row dominates: a draft often survives a corrected input token, so windows > 1 do accept drafts)
        self.table = (torch.randn(STUB_V, STUB_V, generator=g) * 0.7).to(dev)
        self.row = (torch.randn(STUB_P + STUB_N + 64, STUB_V, generator=g) * 3.0).to(dev)

    def forward_window(self, tokens, positions, kv_len, key_start, **kw):
        return self.table[tokens] + self.row[positions]


def _stub_decode(dev, window, scheme, seed, gen_seed=None):
    from sjd_amd.engine import SJDConfig, SJDEngine, WindowSpec
    from sjd_amd.grammar import TopKTopPGrammar
    if "stub" not in _toy:
        _toy["stub"] = _Stub(dev)
    # (the draft window closes 18 tokens before the end for every window size, as in the reference's configs: the loop sizes a window by the length
    #  BEFORE the last iteration, so a window that reaches max_length may emit a token past it -- a property of the schedule, not of a scheme)
    eng = SJDEngine(_toy["stub"], STUB_V, dev, max_window=window, n_batch=1, use_graph=False, narrow_head=False)
    prompt = [5, 6, 7, 8]
    spec = WindowSpec(first_tokens=torch.tensor([prompt], device=dev), first_positions=torch.arange(STUB_P, device=dev)[None],
                      key_start=torch.zeros(1, dtype=torch.int32), pos_offset=torch.zeros(1, dtype=torch.long), kv_base=0)
    cfg = SJDConfig(jacobi_loop_interval_l=0, jacobi_loop_interval_r=STUB_N - 18, max_num_new_tokens=window, guidance_scale=1.0, do_cfg=False, seed=seed,
                    prefix_token_sampler_scheme=scheme, max_length=STUB_P + STUB_N, img_vocab_lo=0, img_vocab_n=STUB_V)
    if gen_seed is not None:
        torch.cuda.manual_seed(gen_seed)
    seq, stats = eng.decode(prompt, spec, TopKTopPGrammar(200, 1.0), cfg)
    return seq, stats


def test_window_invariance_end_to_end(dev):
    runs = {w: _stub_decode(dev, w, "coupled_jacobi", 3) for w in (1, 4, 16)}
    ar = runs[1][0]
    assert len(ar) == STUB_P + STUB_N and runs[1][1].nfe == STUB_N
    for w in (4, 16):
        seq, stats = runs[w]
        assert seq == ar, f"window {w}: the sequence of a seed depends on the draft window"
        assert stats.nfe <= STUB_N
        print(f"stub model, window {w}: {stats.nfe} forwards for {STUB_N} tokens")
    assert runs[16][1].nfe < STUB_N, "window 16 never accepted a draft"
    assert _stub_decode(dev, 16, "coupled_jacobi", 4)[0] != ar               # another seed, another sample
    spec = {w: _stub_decode(dev, w, "speculative_jacobi", 3)[0] for w in (1, 4, 16)}
    assert spec[1] != spec[4] and spec[4] != spec[16] and spec[1] != spec[16]   # today's scheme: the window decides the sample


def test_window_invariance_on_the_transformer_toy_is_reported_only(dev):
    """16-bit kernels may differ in low bits between row counts, so equality is NOT asserted here: the first diverging index is printed"""
    a, b = _lumina_solo(dev, 0, 16)[1], _lumina_solo(dev, 0, 4, record=False)[1]
    first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None)
    print(f"toy Lumina backbone, windows 16 and 4: first diverging index {first} of {len(a)} / {len(b)} tokens (None: identical)")
    assert a[-1] == 8196 and b[-1] == 8196


# ------------------------------------------------------------------------------------------------ 6. the generator is handed back
def test_generator_hand_back(dev):
    ops, _ = _ops()
    gen = torch.cuda.default_generators[dev.index]
    stride = ops.philox_step(STUB_V, ops.philox_max_blocks(dev))
    seq, stats = _stub_decode(dev, 16, "coupled_jacobi", None, gen_seed=555)       # seed None: the decode consumes the device's default generator
    base = 0 + stride                                                 # offset 0 behind manual_seed, then the prefill's [1, V] first-token draw
    last_position = len(seq) - 2                                      # the cache row whose draw is the last token of the sequence
    assert gen.get_offset() == base + (last_position + 1) * stride
    again, _ = _stub_decode(dev, 4, "coupled_jacobi", None, gen_seed=555)          # freshly seeded: the same sample (through another window)
    assert again == seq and gen.get_offset() == base + (last_position + 1) * stride
    after = torch.empty(1, STUB_V, device=dev).exponential_()         # a later draw: noise no position of the decode used
    used = torch.stack([ops.philox_fill(STUB_V, 555, base + t * stride, dev) for t in range(STUB_P - 1, last_position + 1)])
    assert not (used == after).all(dim=1).any()
