"""CPU: the per-prompt SJD state machine (sjd_amd.window_loop.PromptLoop) against the reference loop (oracle/loop.py, OL.run), and the call
order / graph keys of the launch side both engines share (sjd_amd.engine.WindowLauncher) -- no device anywhere.

The model is a deterministic toy without a cache: the fp32 logits of a window row are a fixed hash of (the row's token, kv_len + row), so the
forward is a pure function of (window ids, kv_len, row) and drafts that follow an accepted token stay valid (full accepts happen).  The
oracle runs once per case and its hooks record, per iteration, the window, the corrected tokens, the modes of p, m and the rejection flag;
PromptLoop.plan must then name the same window / rows / kv_len, and fed the recorded read-back PromptLoop.absorb must end in the same
sequence, accept lengths and generator position."""
import zlib

import numpy as np
import pytest
import torch

from oracle import loop as OL
from oracle import sjd_oracle as O

V, IMG_LO, IMG_N, TOP_K, P_LEN, BLOCKS = 64, 4, 32, 3, 5, 2
GRID = (P_LEN, 5, IMG_LO, IMG_LO + IMG_N)          # image starts behind the prompt, 5 tokens per row + a line token


def _forward(win, kv_len):
    out = np.empty((len(win), V), dtype=np.float32)
    for i, t in enumerate(win):                      # mostly the position, a little the token: neighbouring drafts depend weakly on each other
        h = [zlib.crc32(np.asarray(k, dtype=np.int64).tobytes()) for k in ([kv_len + i], [int(t), kv_len + i])]
        out[i] = np.random.default_rng(h[0]).standard_normal(V) * 4.0 + np.random.default_rng(h[1]).standard_normal(V) * 0.7
    return out, None


def _case(scheme="speculative_jacobi", window=16, r=40, max_length=P_LEN + 48, eos=(), do_sample=True, init="random", seed=1):
    return dict(jacobi_loop_interval_l=1, jacobi_loop_interval_r=r, max_num_new_tokens=window, guidance_scale=3.0, seed=seed, do_cfg=False,
                prefix_token_sampler_scheme=scheme, img_vocab_lo=IMG_LO, img_vocab_n=IMG_N, max_length=max_length, eos_token_ids=tuple(eos),
                multi_token_init_scheme=init, do_sample=do_sample)


CASES = {
    # (seeds chosen on the oracle alone so that every trace holds a rejection and a full accept: the first test below asserts it)
    "spec-w16": _case(seed=3),
    "spec-w4": _case(window=4),
    "jacobi-w16": _case(scheme="jacobi", seed=3),
    "jacobi-w4": _case(scheme="jacobi", window=4, seed=2),
    "shrinking-window": _case(r=21, max_length=P_LEN + 30, seed=11),     # n = r_abs - cur_len below the window, then 1
    "eos-in-accepted-run": _case(eos=(28,), seed=7),                     # 28: the last token of a fully accepted window of 10
    "greedy": _case(do_sample=False),
    "repeat_horizon": _case(init="repeat_horizon"),
    "sample_horizon": _case(init="sample_horizon"),
}
_TRACES = {}


def _oracle(name):
    """(prompt, final sequence, OL.Trace, per-iteration records) of a case: the oracle runs once, the replays share the result unchanged"""
    if name not in _TRACES:
        kw = CASES[name]
        prompt = [40 + i for i in range(P_LEN)]
        recs = []

        def hook(kind, d):
            if kind == "sampled":
                recs.append(dict(win=list(d["win"]), Yc=[int(t) for t in d["Y"]], modes=[int(t) for t in np.argmax(d["P"], axis=-1)]))
            else:
                recs[-1]["Yc"] = [int(t) for t in d["Yc"]]
        X, tr = OL.run(prompt, _forward, lambda c, n: O.llamagen_rules(c, n, TOP_K, 1.0), OL.LoopConfig(**kw), V, hook=hook, grid_fn=lambda c: GRID)
        for rec, m, rej in zip(recs, tr.matched, tr.rejected):
            rec["m"], rec["rejected"] = m, rej
        _TRACES[name] = (prompt, X, tr, recs)
    return _TRACES[name]


class _Grammar:
    """sjd_amd.grammar.TopKTopPGrammar with the toy's image geometry (made at call time: the package import stays out of collection)"""

    def __new__(cls):
        from sjd_amd.grammar import TopKTopPGrammar

        class G(TopKTopPGrammar):
            def grid(self):
                return GRID
        return G(TOP_K, 1.0)


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_traces_hold_rejections_and_full_accepts(name):
    """a trace without a rejection (or without a full accept) would let the replay below pass without exercising that split"""
    _, X, tr, recs = _oracle(name)
    kw = CASES[name]
    rows = [1 if i == 0 else len(r["win"]) for i, r in enumerate(recs)]
    partial = [i for i, r in enumerate(recs) if rows[i] > 1 and r["m"] < rows[i]]
    full = [i for i, r in enumerate(recs) if rows[i] > 1 and r["m"] == rows[i]]
    assert partial and full, (tr.matched, rows)
    if kw["prefix_token_sampler_scheme"] == "speculative_jacobi":
        assert any(tr.rejected)
        assert any(r["rejected"] and r["m"] == 1 for r in recs), "a rejection at row 1"
    assert max(rows) == kw["max_num_new_tokens"] and len(tr.matched) < len(X) - P_LEN + 1
    if name == "shrinking-window":
        assert {2, 1} <= set(rows[1:]) and any(1 < n < 16 for n in rows) and rows[-1] == 1
    if kw["eos_token_ids"]:
        assert X[-1] in kw["eos_token_ids"] and len(X) < kw["max_length"] and tr.matched[-1] > 1, "EOS as the last token of an accepted run"
    else:
        assert len(X) >= kw["max_length"]


@pytest.mark.parametrize("generator", ["global", "own"])
@pytest.mark.parametrize("name", list(CASES))
def test_prompt_loop_replays_the_oracle(name, generator):
    import sjd_amd.ops as ops
    from sjd_amd.engine import SJDConfig
    from sjd_amd.window_loop import PromptLoop
    prompt, X_ref, tr, recs = _oracle(name)
    cfg = SJDConfig(**CASES[name])
    greedy, scheme = not cfg.do_sample, 0 if cfg.prefix_token_sampler_scheme == "speculative_jacobi" else 1
    gram = _Grammar()
    loop = PromptLoop(prompt, 0, cfg, ph_seed=cfg.seed, ph_off=8)
    gram.start(loop.X)
    cpu_gen = None
    if generator == "global":
        OL.set_seed(cfg.seed)                                        # as the oracle (and SJDEngine.decode) seed the global generator
    else:
        torch.manual_seed(12345)                                     # the global generator must not matter
        cpu_gen = torch.Generator().manual_seed(cfg.seed)
    cursor, kv_len, draws = 8, 0, {"nV": 0, "1V": 0}
    for i, rec in enumerate(recs):
        assert not loop.finished
        n_rows, fresh, rules, win, resid, use_cfg, draws_rs, offs = loop.plan(cfg, gram, cpu_gen, V, BLOCKS, greedy, scheme, False)
        assert win == rec["win"] and n_rows == (1 if i == 0 else len(rec["win"])) and loop.kv_len == kv_len
        assert len(rules) == n_rows and len(fresh) <= n_rows - 1 and not use_cfg
        assert draws_rs == (scheme == 0 and n_rows > 1) and (resid is not None and len(resid) == (n_rows - 1 if draws_rs else 0))
        step = ops.philox_step(n_rows * V, BLOCKS)                   # the oracle's [n, V] draws in the device layout
        k2 = 0 if greedy else step
        assert offs == (cursor, cursor + k2, cursor + k2 + step)
        k = loop.absorb(rec["m"], int(rec["rejected"]), rec["Yc"], rec["Yc"] if greedy else rec["modes"], len(rec["win"]), cfg, gram)
        assert k == len(tr.final[i])
        draws["nV"] += (0 if greedy else 1) + (1 if draws_rs else 0)
        draws["1V"] += 1 if rec["rejected"] else 0
        cursor += k2 + (step if draws_rs else 0) + (ops.philox_step(V, BLOCKS) if rec["rejected"] else 0)
        kv_len += rec["m"]
        assert loop.ph_off == cursor and loop.kv_len == kv_len
    assert loop.finished and loop.X == X_ref and loop.stats.matched == tr.matched and loop.stats.nfe == len(tr.matched)
    assert draws["1V"] == sum(tr.rejected) and draws["nV"] == sum((0 if greedy else 1) + (1 if scheme == 0 and i and len(r["win"]) > 1 else 0)
                                                                   for i, r in enumerate(recs))


def test_finished_prompt_rides_along_with_a_forced_row():
    import sjd_amd.ops as ops
    from sjd_amd.engine import SJDConfig
    from sjd_amd.window_loop import PromptLoop
    cfg = SJDConfig(**_case(max_length=P_LEN + 1))
    gram = _Grammar()
    loop = PromptLoop([1, 2, 3, 4, 5], 0, cfg, ph_off=0)
    gram.start(loop.X)
    loop.plan(cfg, gram, torch.Generator().manual_seed(0), V, BLOCKS, False, 0, False)
    assert loop.absorb(1, 0, [7], [9], 5, cfg, gram) == 1 and loop.finished and loop.kv_len == 5 and loop.stats.matched == [5] and loop.last_amax == 9
    off = loop.ph_off
    n_rows, fresh, rules, win, resid, use_cfg, draws_rs, offs = loop.plan(cfg, gram, None, V, BLOCKS, False, 0, True)
    assert (n_rows, fresh, win, resid, use_cfg, draws_rs) == (1, [], None, [], False, False) and rules[0].forced == 0
    assert loop.absorb(1, 0, [3], [3], 1, cfg, gram) == 0 and loop.X[-1] == 7 and loop.stats.nfe == 1
    assert loop.ph_off == off + ops.philox_step(V, BLOCKS)          # (the dummy row's draw keeps blob and generator consistent)
    with pytest.raises(RuntimeError, match="residual distribution .* is empty .* JL:237"):
        PromptLoop([1], 0, cfg).absorb(1, 2, [3], [3], 1, cfg, gram)


# ------------------------------------------------------------------------------------------------ the launch side, without a device
def _fake_launcher(use_graph=False):
    from sjd_amd.engine import WindowLauncher

    class Fake(WindowLauncher):
        def __init__(self):
            self.use_graph, self.calls = use_graph, []
            self.reset_graphs()

        def _forward_body(self, cols):
            self.calls.append(("forward", cols))
            return ("logits", cols)

        def _sample_body(self, cur, logits, cols):
            self.calls.append(("sample", cur, logits, cols))

        def _graph_key(self, kind, cols, cur=None):
            return (kind, cols, cur)
    return Fake()


def test_launch_order_one_stage_and_two_stage():
    f = _fake_launcher()
    assert f._launch_window(1, (0, 32)) == ("logits", (0, 32))
    assert f.calls == [("forward", (0, 32)), ("sample", 1, ("logits", (0, 32)), (0, 32))]
    f.calls.clear()
    logits = f._launch_forward(None)
    assert f.calls == [("forward", None)] and logits == ("logits", None)
    f._launch_sample(0, logits, None)                                # (the residual rules went up in between)
    assert f.calls == [("forward", None), ("sample", 0, ("logits", None), None)]
    assert f._graphs == {} and f.captured_column_windows() == []


def test_graph_keys_of_both_engines():
    from sjd_amd.engine import SJDEngine
    from sjd_amd.engine_batch import SJDBatchEngine

    class Attn:
        regime = "colsplit"

    class Backbone:
        attn = Attn()
    solo = SJDEngine.__new__(SJDEngine)
    solo.backbone, solo.hook, solo._philox, solo._guidance, solo._greedy = Backbone(), None, True, 3.0, False
    cols = (0, 8224)
    assert solo._graph_key("fwd", cols) == ("fwd", cols, "colsplit")
    assert solo._graph_key("win", cols, 1) == ("win", cols, 1, 3.0, False, True, "colsplit", False)
    assert solo._graph_key("smp", cols, 1) == ("smp", 1, 3.0, cols, False, True, "colsplit", False)
    batch = SJDBatchEngine.__new__(SJDBatchEngine)
    batch.backbone, batch.hook, batch._guidance, batch._mixed_guidance, batch._greedy = Backbone(), object(), 4.0, False, True
    assert batch._graph_key("fwd", None) == ("fwd", None)
    assert batch._graph_key("win", None, 0) == ("win", None, 0, 4.0, True, True)
    assert batch._graph_key("smp", None, 0) == ("smp", 0, None, "colsplit", 4.0, True, True)      # the regime: whose forward buffer it bakes in
    batch._mixed_guidance = True
    assert batch._graph_key("win", cols, 1)[3] == "per-slot array"
    for eng in (solo, batch):                                        # what tools and tests read: [0] the kind, [1] the column window
        for kind in ("fwd", "win"):
            k = eng._graph_key(kind, cols, 0)
            assert k[0] == kind and k[1] == cols
