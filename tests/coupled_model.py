"""NumPy model of coupled Jacobi decoding (prefix_token_sampler_scheme="coupled_jacobi"): the race draw, the equality accept
and the re-guess of fresh rows, with the noise of a draw keyed by the POSITION of the row that draws it.

    draw      token = lowest-index argmax_c fp32(p[c] / e[c]) over the columns with p[c] > 0          (K2's exponential race)
    accept    m = the first i >= 1 with window[i] != Y[i - 1], else n                                  (K4, schemes 1 and 2)
    re-guess  window' = [last emitted | the samples carried out of the last window | fresh ids]         (K5)

Position t is the cache row of the window row: row j of a window that starts at `kv_len` stands at t = kv_len + j, and its noise is
noise_of(t), whatever window or iteration it is drawn in.  The token a position emits is then a function of that position's distribution alone,
and the loop is a fixed-point iteration on the autoregressive sample under that noise.

Two users: tests/test_coupled_cfg.py runs `decode` on a random prefix -> distribution table (no device), tests/test_gpu_coupled.py replays the
engines' recorded iterations through `CoupledReplay`, row by row.
"""
import numpy as np


def race_draw(p, e):
    """lowest-index argmax of fp32(p / e) over p > 0 (a column without mass scores 0, as in K2); p, e: fp32 [V]"""
    p, e = np.asarray(p, dtype=np.float32), np.asarray(e, dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(p > 0, p / e, np.float32(0.0)).astype(np.float32)
    return int(np.argmax(r))                                 # (np.argmax returns the first of equal maxima)


def accept_len(window, Y):
    """K4, token equality: the number of tokens the iteration emits -- drafts window[1:] against the samples Y of the rows before them"""
    n = len(window)
    for i in range(1, n):
        if int(window[i]) != int(Y[i - 1]):
            return i
    return n


def next_window(last, carried, n, fresh):
    """K5: [last emitted | carried samples | fresh ids]; fresh(k) -> k ids (called even for k = 0: the engine's generator is)"""
    a = max(0, min(len(carried), n - 1))
    return [int(last)] + [int(t) for t in carried[:a]] + [int(t) for t in fresh(n - 1 - a)]


def decode(dist_of, noise_of, first_token, n_tokens, window, fresh):
    """The whole loop on a model given as a function: dist_of(tuple of the tokens so far) -> fp32 [V], the distribution of the next token;
    noise_of(t) -> fp32 [V], the Exp(1) noise of position t (the position of the LAST token of that prefix; first_token stands at 0).
    -> (the n_tokens tokens behind first_token, the accept count of every step)."""
    X, carried, steps = [int(first_token)], [], []
    while len(X) - 1 < n_tokens:
        n = min(window, n_tokens - (len(X) - 1))
        win = next_window(X[-1], carried, n, fresh)
        t0 = len(X) - 1
        Y = [race_draw(dist_of(tuple(X + win[1:j + 1])), noise_of(t0 + j)) for j in range(n)]
        m = accept_len(win, Y)
        X.extend(Y[:m])
        carried = Y[m:]
        steps.append(m)
    return X[1:], steps


class CoupledReplay:
    """One prompt's loop, fed the engine's recorded iterations: `step` takes the rows' distributions as the engine's K2 wrote them and the rows'
    noise, and returns what the model draws, accepts and emits; the window ids are the model's own (its carried samples, the fresh ids of
    `fresh`), so a wrong draw anywhere shows as a wrong window later.  eos / max_length end the decode as the engine's loop does."""

    def __init__(self, prompt, fresh, eos=(), max_length=1 << 30):
        self.X, self.P = [int(t) for t in prompt], len(prompt)
        self.carried, self.fresh, self.eos, self.max_length = [], fresh, tuple(eos), max_length
        self.first, self.finished, self.matched = True, False, []

    def step(self, n_rows, probs, noise):
        """probs, noise: fp32 [n_rows, V] -> (window, Y, m).  The first call is the prefill iteration: one row, the prompt's last."""
        assert not self.finished
        if self.first:
            self.fresh(0)
            win = list(self.X)
        else:
            win = next_window(self.X[-1], self.carried, n_rows, self.fresh)
        assert n_rows == (1 if self.first else len(win))
        Y = [race_draw(probs[j], noise[j]) for j in range(n_rows)]
        m = 1 if n_rows <= 1 else accept_len(win, Y)
        self.X.extend(Y[:m])
        self.carried = [] if n_rows <= 1 else Y[m:]
        self.matched.append(len(win) if self.first else m)
        self.first = False
        self.finished = self.X[-1] in self.eos or len(self.X) >= self.max_length
        return win, Y, m
