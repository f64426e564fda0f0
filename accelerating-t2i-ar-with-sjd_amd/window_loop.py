"""The per-prompt SJD state machine: the reference's `_sample` loop (scheduler/jacobi_iteration_lumina_mgpt.py:912-1249) as host-side integer
bookkeeping, once for SJDEngine.decode and for every slot of SJDBatchEngine.decode_many.

`plan` names everything an iteration's launch needs -- rows, fresh ids, rules, window, residual rules, the device generator's offsets -- and
`absorb` takes what K4 read back: it advances the generator cursor, splits the tokens into emitted / carried, sets the next window length
and tests for the end.  Nothing here touches a device: tests/test_window_loop.py holds the class to the CPU oracle (oracle/loop.py).
"""
from dataclasses import dataclass, field
from typing import List

import torch

from . import ops
from .grammar import spatial_fresh_tokens

COUPLED = 2          # engine.SCHEME_CODES["coupled_jacobi"]: K2 keys a row's noise by its position (include/sjd_hip.h)


@dataclass
class DecodeStats:
    nfe: int = 0
    tokens: int = 0
    seconds: float = 0.0
    wall_seconds: float = 0.0
    timed_nfe: int = 0
    timed_region_reached: bool = True   # False: bench mode, but the decode ended before the timed region opened (stats cover the whole decode)
    kv_len: int = 0                # KV length at the end of the timed region (whole decode when none)
    kv_len_start: int = 0          # ... at its start
    total_tokens: int = 0          # whole decode (lead-in + warm-up + timed + continuation)
    total_seconds: float = 0.0
    timed_host_seconds: float = 0.0    # host_seconds / sync_seconds at the end of the timed region
    timed_sync_seconds: float = 0.0
    host_seconds: float = 0.0      # host bookkeeping + RNG launches before the window step is enqueued
    sync_seconds: float = 0.0      # time blocked in the per-iteration state read-back
    matched: List[int] = field(default_factory=list)


class PromptLoop:
    """One prompt's decode state: the accepted ids X (P of them the prompt), the next window length n, the KV rows kv_len, the drafts carried
    out of the last window with the modes of their distributions, and the cursor (ph_seed, ph_off) of the prompt's device generator."""

    def __init__(self, prompt, kv_base, cfg, ph_seed=0, ph_off=0):
        self.X = [int(t) for t in prompt]
        self.P = len(self.X)
        self.l_abs, self.r_abs = self.P + cfg.jacobi_loop_interval_l, self.P + cfg.jacobi_loop_interval_r   # JL:1025
        self.n, self.kv_len, self.cur_len, self.n_prev, self.m_prev = 1, kv_base, self.P, 1, 1
        self.carried, self.carried_amax, self.last_amax = [], [], None
        self.first, self.finished = True, False
        self.ph_seed, self.ph_off = ph_seed, ph_off
        # the coupled scheme (code 2): the offset of position 0's noise -- the generator's right behind the prefill's first-token draw, fixed for
        # the whole decode -- and the step from one position to the next; None until the prefill iteration was absorbed / in the other schemes
        self.ph_base, self.ph_stride = None, 0
        self.n_rows, self.ph_step, self.k2_step, self.ph_row, self.draws_rs = 1, 0, 0, 0, False      # the last plan's
        self.stats = DecodeStats()

    def plan(self, cfg, grammar, cpu_gen, V, ph_blocks, greedy, scheme, do_cfg):
        """-> (n_rows, fresh, rules, win, resid, use_cfg, draws_rs, offsets) of the next iteration.  cpu_gen: the generator of the fresh ids
        (None: the GLOBAL CPU generator, JL:505).  win: the window's ids, all known here (carried ones came with the last read-back).  resid:
        the residual rules when the grammar can name them without a replay -- the whole iteration then goes out as one graph -- or None: two
        stages, they are computed while the forward runs (K4 is their only reader).  offsets: the device generator's before the multinomial,
        the rand and the residual multinomial (ph_blocks None: the noise is not generated in the kernels, no offsets).  A finished prompt
        that rides along gets a dummy one-row window: a forced row (K2 reads no logits), result ignored."""
        resid = []
        if self.finished:
            n_rows, fresh, win, rules, use_cfg = 1, [], None, [ops.make_rule(forced=0)], False
        else:
            if self.first:                                                           # prefill: every prompt token (JL:344-350)
                n_rows, fresh, win = 1, [], list(self.X)
                torch.randint(0, cfg.img_vocab_n, (1, 0), generator=cpu_gen)
            else:
                n_rows, X, carried = self.n, self.X, self.carried
                a = max(0, min(self.n_prev - self.m_prev, n_rows - 1))               # JL:633-639, 657-662
                lo = cfg.img_vocab_lo
                fresh = [lo + t for t in torch.randint(0, cfg.img_vocab_n, (1, n_rows - 1 - a), generator=cpu_gen)[0].tolist()]   # img_vocab[rand] (JL:509)
                if cfg.multi_token_init_scheme != "random":                          # spatial init (JL:516-594): copy / re-draw from the left
                    fresh = spatial_fresh_tokens(cfg.multi_token_init_scheme, fresh, len(X) + a, carried[a - 1] if a else X[-1],
                                                 self.carried_amax[a - 1] if a else self.last_amax, grammar.grid())
                win = [X[-1]] + carried[:a] + fresh
            rules = grammar.window_rules(n_rows)
            if scheme == 0 and n_rows > 1:
                resid = grammar.fast_residual_rules(win, rules)
            use_cfg = do_cfg and not grammar.force_no_cfg()                          # JL:1086-1096
        self.n_rows, self.draws_rs = n_rows, n_rows > 1 and scheme == 0
        if ph_blocks is None:
            return n_rows, fresh, rules, win, resid, use_cfg, self.draws_rs, None
        if scheme == COUPLED and not self.first:
            # position-keyed noise: K2 takes row j's from offset base + (kv_len + j) * stride (word 0 the base, word 1 the stride, word 2 unused);
            # nothing is consumed per iteration, the cursor stays where the prefill left it
            if self.ph_base is None:
                self.ph_base, self.ph_stride = self.ph_off, 0 if greedy else ops.philox_step(V, ph_blocks)
            self.ph_step = self.k2_step = self.ph_row = 0
            return n_rows, fresh, rules, win, resid, use_cfg, False, (self.ph_base, ops.philox_step(V, ph_blocks), 0)
        # what torch would consume: an [n, V] multinomial (greedy: sampling_logits2tokens draws nothing, JL:127-129), an [n, V] rand and --
        # only after a rejection -- the [1, V] residual multinomial
        self.ph_step = step = ops.philox_step(n_rows * V, ph_blocks)
        self.k2_step = k2 = 0 if greedy else step
        self.ph_row = ops.philox_step(V, ph_blocks) if self.draws_rs else 0
        off = self.ph_off
        return n_rows, fresh, rules, win, resid, use_cfg, self.draws_rs, (off, off + k2, off + k2 + step)

    def launch_scheme(self, scheme):
        """the scheme code of the NEXT iteration's blob.  The coupled scheme's prefill iteration carries code 1: its one row is the first-token draw,
        which stays the per-launch draw at the generator's own offset that every scheme makes (K4 short-circuits at n <= 1 whatever the code)."""
        return 1 if scheme == COUPLED and self.ph_base is None else scheme

    def keyed(self, scheme, kv_len):
        """(base, stride, kv_len) of a coupled window iteration, None for anything else (the engines' observer noise)"""
        return (self.ph_base, self.ph_stride, kv_len) if scheme == COUPLED and self.ph_base is not None else None

    def end_offset(self):
        """where the prompt's device generator is left when the decode ends: the cursor, or -- coupled -- behind the noise of the last position that
        emitted a token (cache row kv_len - 1), base + kv_len * stride, so that no later draw of the generator reuses noise a token came from.  It
        depends on the emitted sequence alone, not on the window.  (A greedy decode drew nothing: the stride is 0 and the base comes back.)"""
        return self.ph_off if self.ph_base is None else self.ph_base + self.kv_len * self.ph_stride

    def absorb(self, m_dev, rejected, tokens, amax, win_len, cfg, grammar):
        """The read-back of the planned iteration: K4's accept length and rejection flag, the corrected tokens and the modes of the target
        rows (greedy: the tokens themselves), the rows the forward was given (the prompt's in iteration 0).  Returns the number of tokens
        appended to X."""
        if self.finished:
            self.ph_off += self.k2_step               # (the dummy row's draw: keeps blob and generator consistent; never observed)
            return 0
        if rejected > 1:
            raise RuntimeError("SJD verify: the residual distribution max(p - q, 0) is empty under the residual grammar rule "
                               "(the reference's torch.multinomial raises on the NaN probabilities at JL:237)")
        n_rows = self.n_rows
        if self.draws_rs:
            self.ph_off += self.k2_step + self.ph_step + (self.ph_row if rejected else 0)
        else:
            self.ph_off += self.k2_step
        if n_rows <= 1:
            m = win_len                               # is_prefilling_phase short-circuit (JL:344-350)
            emitted, self.carried, self.carried_amax, self.last_amax = [tokens[0]], [], [], amax[0]
        else:
            m = m_dev
            emitted, self.carried, self.carried_amax, self.last_amax = tokens[:m], tokens[m:n_rows], amax[m:n_rows], amax[m - 1]
        self.stats.matched.append(m)
        cur_len, X = self.cur_len, self.X
        self.n = min(cfg.max_num_new_tokens, self.r_abs - cur_len) if (self.l_abs <= cur_len < self.r_abs) else 1     # JL:1142-1144 (old cur_len)
        X.extend(emitted)
        grammar.push(emitted)
        self.kv_len += m                              # KV rollback: rows of rejected drafts are overwritten by the next window
        self.n_prev, self.m_prev = n_rows, (1 if n_rows <= 1 else m)
        self.first = False
        self.stats.nfe += 1
        self.finished = X[-1] in cfg.eos_token_ids or len(X) >= cfg.max_length      # JL:1200-1201
        self.cur_len = len(X)
        return len(emitted)
