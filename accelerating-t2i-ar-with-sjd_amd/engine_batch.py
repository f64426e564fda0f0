"""Several prompts per GPU in ONE window forward (the reference decodes one prompt per process).

A draft-window forward is a pure weight stream: 13 GB of weights for 32 activation rows.  Two prompts (2 x B_cfg x L = 64 rows)
cost the same stream, so decoding them together almost doubles the accepted tokens per second of a GPU; up to eight prompts (256 rows; the rate is flat beyond four: DESIGN.md 10b;
G1's sub-tiled kernel) fit in one forward: 963 / 1292 tokens/s per MI355X for two / four Lumina 768px prompts against 561 for one.  Every prompt ("slot")
IS the state machine `SJDEngine.decode` runs (window_loop.PromptLoop: a slot is one plus its device handles) -- its own window, accept
length, KV length, grammar, device generator and CPU generator for the fresh ids -- so each slot takes the decisions its solo run would
take on the same logits; only the transformer forward is shared, launched through the graph cache both engines use
(engine.WindowLauncher):

   host    per slot: n, fresh ids, rules, residual rules, its generator's seed / offsets -> its blob of a contiguous sjd_iter_params
           ARRAY (batch_rows = B_cfg: the kernels K1 / K3 / F2 pick the blob of a batch row, i.e. every prompt has its own kv_len and
           n_rows), one H2D for all
   graph   K5 per slot (window ids of that slot's batch rows), ONE backbone.forward_window over all slots' rows with the output head as
           split-K partials over the union of the slots' column windows, K2 (PART, in-kernel noise) + K4 per slot (own probability
           buffers); ONE hipGraph when every slot's grammar names its residual rules up front (SJDEngine's two-stage launch otherwise)
   host    one stream wait (every K4 wrote its state into pinned host memory), per-slot bookkeeping

A slot that reaches its end token keeps riding along with a one-row dummy window (its tokens are ignored) until every slot is done.
"""
import dataclasses
import time
from typing import List

import os
import torch

from . import _lib as L
from . import launch_shapes as LS
from . import ops
from .engine import SJDConfig, WindowLauncher, WindowSpec, cached_column_window, check_reduce_timeouts, scheme_code
from .window_loop import PromptLoop


class _CacheView:
    """The KV cache rows of one slot (batch rows [lo, hi)) presented as a StaticKVCache to the backbone's prefill."""

    def __init__(self, cache, lo, hi):
        self.k, self.v, self.s_max = cache.k[:, lo:hi], cache.v[:, lo:hi], cache.s_max


class _Slot(PromptLoop):
    """A prompt's state machine plus the slot's device handles (params, state, probs, ...): an admission starts the machine again
    (PromptLoop.__init__) on the same handles."""

    def __init__(self):
        pass


# what the prompts of one decode_many may NOT differ in: the window iterations run in lock-step through one set of launches, one scheme, one noise
# source.  guidance_scale and seed are per prompt (temperature / top-p / top-k already are: they live in each prompt's grammar); do_cfg may differ
# as long as "CFG on" (below) does not.
_PER_PROMPT_FIELDS = ("guidance_scale", "seed", "do_cfg")
_CFG_ON = "do_cfg and guidance_scale != 1"


def _cfg_on(c):
    return bool(c.do_cfg and (c.guidance_scale != 1))


def per_prompt_configs(cfg, n_prompts):
    """decode_many's `cfg` -> (the config every shared field is read from, None | the N per-prompt configs).  A sequence must hold one SJDConfig
    per prompt; every field except guidance_scale / seed / do_cfg must agree, and so must "CFG on" (it fixes the batch rows per slot)."""
    if isinstance(cfg, SJDConfig):
        return cfg, None
    cfgs = list(cfg)
    if len(cfgs) != n_prompts:
        raise ValueError(f"decode_many got {len(cfgs)} configs for {n_prompts} prompts: pass one SJDConfig, or one per prompt")
    for j, c in enumerate(cfgs):
        if not isinstance(c, SJDConfig):
            raise ValueError(f"config of prompt {j} is {type(c).__name__}, not an SJDConfig")
    names = [c.prefix_token_sampler_scheme for c in cfgs]
    if "coupled_jacobi" in names and len(set(names)) > 1:
        j = next(k for k, nm in enumerate(names) if nm != names[0])
        raise ValueError(f"prefix_token_sampler_scheme='coupled_jacobi' cannot be mixed with another scheme in one decode_many (prompt 0 has {names[0]!r}, "
                         f"prompt {j} has {names[j]!r}): the host keeps one noise bookkeeping for the lock-step iterations -- a position-keyed "
                         "base and stride per prompt, or a cursor that advances per iteration")
    for f in dataclasses.fields(SJDConfig):
        if f.name in _PER_PROMPT_FIELDS:
            continue
        for j, c in enumerate(cfgs[1:], 1):
            if getattr(c, f.name) != getattr(cfgs[0], f.name):
                raise ValueError(f"SJDConfig.{f.name} must agree across the prompts of one decode_many, but prompt 0 has "
                                 f"{getattr(cfgs[0], f.name)!r} and prompt {j} has {getattr(c, f.name)!r}")
    for j, c in enumerate(cfgs[1:], 1):
        if _cfg_on(c) != _cfg_on(cfgs[0]):
            raise ValueError(f"'{_CFG_ON}' (CFG on / off: the batch rows of a slot) must agree across the prompts of one decode_many, but it is "
                             f"{_cfg_on(cfgs[0])} for prompt 0 and {_cfg_on(c)} for prompt {j}: mixing CFG-on and CFG-off prompts is not served")
    return cfgs[0], cfgs


class SJDBatchEngine(WindowLauncher):
    def __init__(self, backbone, vocab_size, device, n_prompts, max_window=16, n_batch=2, use_graph=True, narrow_head=True, head_partials=True):
        bargs = getattr(backbone, "args", None)
        if getattr(bargs, "swin_norm", False) or getattr(bargs, "model_parallel_size", 1) != 1:
            raise ValueError("SJDBatchEngine does not serve swin-norm backbones (swin_norm=True or model_parallel_size > 1, the 30B-class "
                             "Chameleon form): decode them one prompt at a time with SJDEngine / FlexARInferenceSolver")
        rows = n_prompts * n_batch * max_window
        to = 128 if rows <= 128 else 256                                 # the max_rows a refusal names: the set packed for that many rows
        why, detail = LS.serves_rows(backbone, rows, head=True) or (None, None)          # (launch_shapes.py: what a packed backbone serves, and why not)
        if getattr(backbone, "weights", None) == "e4m3":                 # enable_fused(weights=..., max_rows=...)
            if not getattr(backbone, "_max_rows_given", False):
                raise ValueError("SJDBatchEngine does not serve a backbone packed with enable_fused(weights='e4m3'): 8-bit weights serve one prompt per "
                                 "forward (at most 64 window rows) in this version -- decode with SJDEngine, or pack with weights=None")
            if why == "max_rows":
                raise ValueError(f"the backbone was packed for windows of at most max_rows={detail} rows, but n_prompts * n_batch * max_window = "
                                 f"{rows}: call enable_fused(ops, gemm='sjd', weights='e4m3', max_rows={to}), or use fewer prompts per forward")
        # a stream without a wide form on a Chameleon-family backbone ("mxfp4", "e2m3" and their twins): packed for 64 rows, always.  (A LlamaGen backbone's
        # 4-bit copy serves the max_rows it was packed for -- kernel G1wq4 above 64 -- and is refused below like any other LlamaGen backbone.)
        stream = LS.stream_of(getattr(backbone, "weights", None))[0]
        if stream is not None and rows > stream.max_rows <= 64 and not ("llamagen" in stream.has and LS.is_llamagen(backbone)):
            raise ValueError(f"a backbone packed with enable_fused(weights={backbone.weights!r}) serves at most {stream.max_rows} window rows per forward (kernels "
                             f"{stream.kernels} have no wide form), but n_prompts * n_batch * max_window = {rows}: use fewer prompts per forward, or weights='e4m3' "
                             "with max_rows=128 / 256")
        L.load()                                   # fail loudly if the HIP extension is missing
        if max_window > L.MAX_WINDOW:
            raise ValueError(f"max_window {max_window} > {L.MAX_WINDOW}")
        if rows > LS.WINDOW_MAX_ROWS:
            raise ValueError("the window forward (G1, F1-F3) serves at most 256 rows: n_prompts * n_batch * max_window <= 256")
        # a LlamaGen window forward leaves the HIP path above the row count the weights were packed for (LlamaGenBackbone.forward_window) and
        # would fall onto ATen silently: not bit-identical to the oracle replays, and no head partials for K2
        if why == "unfused":
            raise ValueError("SJDBatchEngine serves a LlamaGen backbone on the fused HIP path only: call "
                             f"model.enable_fused(ops, gemm='sjd', max_rows=...) first ({rows} window rows per forward here"
                             + ("; head_dim 100: with pad_head_dim=True, padded_batch=True)" if getattr(backbone, "head_dim", 0) == 100 else ")"))
        # (a head_dim-100 backbone stored 128 wide is packed for more than 64 rows on request only: the refusals name both arguments)
        padded = ", pad_head_dim=True, padded_batch=True" if getattr(backbone, "_head_pad", None) else ""
        if LS.is_llamagen(backbone) and getattr(backbone, "weights", None) is not None:
            padded += f", weights={backbone.weights!r}"
        if why == "fp16":
            raise ValueError(f"the backbone was packed for fp16 windows of at most {detail} rows, but n_prompts * n_batch * max_window = {rows}: "
                             f"call enable_fused(ops, gemm='sjd', max_rows=256, untuned_fp16=True{padded}), or use fewer prompts per forward")
        if why == "max_rows":
            raise ValueError(f"the backbone was packed for windows of at most max_rows={detail} rows, but "
                             f"n_prompts * n_batch * max_window = {rows}: call enable_fused(ops, gemm='sjd', max_rows={to}{padded})")
        # 129..256 window rows run on kernel G1w (csrc/sjd_gemm_wide.h): the uncompressed packing, LS.WIDE_TILES column tiles per workgroup
        # for every projection AND the output head.  Anything else used to fall onto the library-GEMM prefill path silently
        # (slower, not bit-identical to the oracle replays) or to fail at the first forward: say so here instead.
        if why == "12-bit":
            raise ValueError(f"{rows} window rows per forward need the uncompressed packing: enable_fused(ops, gemm='sjd', compress=False) "
                             "(the 12-bit stream serves up to 128 rows)")
        if why == "tiles":
            raise ValueError(f"{rows} window rows per forward run on kernel G1w with {LS.WIDE_TILES} column tiles per workgroup; set "
                             f"model.G1_CFG = dict(model.G1_CFG_256ROW) before enable_fused -- offending launch shapes: {detail}")
        self.backbone, self.V, self.device = backbone, int(vocab_size), torch.device(device)
        self.P, self.nb, self.Lmax, self.B = n_prompts, n_batch, max_window, n_prompts * n_batch
        self.use_graph, self.narrow_head = use_graph, narrow_head
        dev = self.device
        self.params = ops.BlobArray(L.IterParams, self.P, dev)
        self.state = ops.BlobArray(L.State, self.P, dev)
        self.params.view = self.params.blobs[0].view          # what HipWindowAttention's profiling hook looks at
        self.slots = []
        # every slot's buffers at one stride: K5 / K2 / K4 of ALL slots are one launch each (round 6, sjd_slots in include/sjd_hip.h)
        self.probs_all = torch.zeros(self.P, 2, self.Lmax, self.V, dtype=torch.float32, device=dev)
        self.zero_state_all = torch.full((self.P, 2, self.Lmax, 2), -1, dtype=torch.int32, device=dev)
        self.scratch_all = torch.empty(self.P, self.V, dtype=torch.float32, device=dev)
        self.state.mirror_array()
        self.slot_launches = os.environ.get("SJD_SLOT_LAUNCHES", "1") != "0"       # 0: one K5 / K2 / K4 launch per slot (rounds 3-5; A/B aid)
        self._slots_desc = ops.slots_of(self.params, self.state, self.probs_all, self.zero_state_all, self.scratch_all, n_batch)
        for i in range(self.P):
            s = _Slot()
            s.params, s.state = self.params.blobs[i], self.state.blobs[i]
            s.params.view.batch_rows = n_batch
            s.probs = self.probs_all[i]
            s.zero_state = self.zero_state_all[i]        # see SJDEngine.zero_state
            s.noise = s.rs = s.noise2 = None        # only for observers (the parity tests' hook): K2 / K4 generate their noise
            s.scratch = self.scratch_all[i]
            s.tokens_ptr = s.state.field_ptr("tokens")
            s.amax_ptr = s.state.field_ptr("amax")
            self.slots.append(s)
        self.input_ids = torch.zeros(self.B, self.Lmax, dtype=torch.int64, device=dev)
        self.arange = torch.arange(self.Lmax, device=dev)
        self.positions = torch.zeros(self.B, self.Lmax, dtype=torch.int64, device=dev)      # window position ids, written by K5
        self.key_start = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.pos_offset = torch.zeros(self.B, dtype=torch.int64, device=dev)
        nb_params, off = L.ctypes.sizeof(L.IterParams), L.IterParams.kv_len.offset
        assert nb_params % 4 == 0
        # device view of every slot's params->kv_len, repeated for the slot's batch rows
        self.kv_len_dev = self.params.dev.view(torch.int32)[off // 4::nb_params // 4]
        self.row_slot = torch.arange(self.B, device=dev) // n_batch
        self._guidance = 3.0
        # one guidance scale per SLOT, for a decode_many whose prompts differ in it: K2's slot launch reads the device array (captured graphs point
        # at it, so it exists before the first capture), an admission writes the slot's element of the pinned twin and uploads it behind the blob
        self._guid_host = torch.zeros(self.P, dtype=torch.float32, pin_memory=True)
        self._guid_dev = torch.zeros(self.P, dtype=torch.float32, device=dev)
        self._mixed_guidance = False
        # K2 reads the output head's split-K partials (no fp32 logits tensor) when the backbone can produce them
        self.head_partials = bool(head_partials) and getattr(backbone, "supports_head_partials", False)
        self._dbg = None                       # [B, L, V] logits as K2 derived them; allocated only for observers (hook)
        self.hook = None                       # test hook: called per slot and iteration with that slot's device tensors
        self._rule_bytes, self._rule_keep, self._cols_cache = {}, [], {}
        self.reset_graphs()

    def _per_slot(self, fn):
        """fn(i, slot) for every slot, one after the other on the current stream.  (Round 6 measured the alternative -- the slots' K5 / K2 + K4
        launches as parallel branches of the iteration's hipGraph, forked onto side streams and rejoined: eight prompts 7.2 -> 8.5 ms per step,
        four 4.7 -> 5.5; a fork / join pair costs more than the 5-28 us launches it overlaps.  profiles/r6_slot_fanout_ab.txt)"""
        for i, s in enumerate(self.slots):
            fn(i, s)

    def _forward_body(self, cols):
        def k5(i, s):
            lo, hi = i * self.nb, (i + 1) * self.nb
            ops.reguess(s.params, s.state, self.input_ids[lo:hi], pos_offset=self.pos_offset[lo:hi], positions_out=self.positions[lo:hi])
        if self.slot_launches:
            ops.reguess_slots(self._slots_desc, self.params, self.state, self.input_ids, self.pos_offset, self.positions, self.nb)
        else:
            self._per_slot(k5)
        positions = self.positions
        if self.head_partials:
            return self.backbone.forward_window(self.input_ids, positions, -1, self.key_start, cols=cols, head_partials=True)
        if cols is None:
            return self.backbone.forward_window(self.input_ids, positions, -1, self.key_start)
        return self.backbone.forward_window(self.input_ids, positions, -1, self.key_start, cols=cols)

    def _sample_body(self, cur, logits, cols):
        """K2 + K4 per slot, noise generated in the kernels.  With the output head as split-K partials every slot's K2 reads ITS rows of
        the one G1 launch over the union column window (cond rows of batch row 2i, uncond rows of 2i + 1)."""
        part = isinstance(logits, ops.HeadOut)
        dbg = None
        if part and self.hook is not None:
            if self._dbg is None:
                self._dbg = torch.zeros(self.B, self.Lmax, self.V, dtype=torch.float32, device=self.device)
            dbg = self._dbg
            dbg.zero_()
        wide = part and not ops.head_slots_ok(logits)          # a head wide enough for K2a: it runs in front of every slot's own K2
        def k2_k4(i, s):
            tok_out, amax_out = self._k2_out(s)
            if part:              # (different scales: K2a reads the slot's element of the engine's array -- a wide head, see below)
                g = self._guid_dev[i:i + 1] if self._mixed_guidance else self._guidance
                ops.logits_to_probs_sample_part(logits, g, s.params, None, s.probs[cur], tok_out, amax_out_ptr=amax_out,
                                                dbg=None if dbg is None else dbg[i * self.nb:(i + 1) * self.nb], row0=i * self.nb * self.Lmax,
                                                urow_off=self.Lmax if self.nb > 1 else 0, zero_state=s.zero_state[cur])
            else:
                lc = logits[i * self.nb]
                lu = logits[i * self.nb + 1] if self.nb > 1 else None
                ops.logits_to_probs_sample(lc, lu, self._guidance, s.params, None, s.probs[cur], tok_out, col0=cols[0] if cols else 0,
                                           amax_out_ptr=amax_out)
                s.zero_state[cur].fill_(-1)
            ops.verify_accept(s.params, s.state, s.probs[cur], s.probs[1 - cur], None, None, s.scratch, mirror=True)
        if self.slot_launches and part and not wide:
            # one K2 and one K4 launch for all slots (a workgroup per (row, slot) / per slot): eight prompts 8 x (28 + 24) us -> one of each
            greedy = getattr(self, "_greedy", False)
            sl = self._slots_desc
            if dbg is not None:
                sl = ops.slots_of(self.params, self.state, self.probs_all, self.zero_state_all, self.scratch_all, self.nb, dbg=dbg)
            g = self._guid_dev if self._mixed_guidance else self._guidance
            ops.logits_to_probs_sample_part_slots(sl, logits, g, self.params, self.probs_all, cur, "amax" if greedy else "tokens",
                                                  "tokens" if greedy else "amax", self.state, self.zero_state_all, self.nb, dbg=dbg)
            ops.verify_accept_slots(sl, self.params, self.state, self.probs_all, cur, self.scratch_all)
            return
        if not wide:                                               # (a wide head: K2a takes the scale by pointer)
            self._refuse_mixed_guidance_per_slot()
        self._per_slot(k2_k4)

    def _guidance_key(self):
        """the guidance part of a graph key: the scale itself (baked into the captured launches), or -- prompts with different scales -- a constant:
        the captured K2 reads the engine's array, whatever it holds"""
        return "per-slot array" if self._mixed_guidance else self._guidance

    def _graph_key(self, kind, cols, cur=None):
        """the key of this iteration's forward ("fwd"), one-stage ("win") or two-stage sample ("smp") graph.  A sample graph bakes in the
        forward graph's buffer it was captured on, and every K1 regime's forward owns its own: the regime is part of that key."""
        if kind == "fwd":
            return ("fwd", cols)
        own = (self._guidance_key(), self.hook is not None, getattr(self, "_greedy", False))
        return ("win", cols, cur) + own if kind == "win" else ("smp", cur, cols, self._k1_regime()) + own

    def _refuse_mixed_guidance_per_slot(self, why=None):
        """Different guidance scales in one batch are served by the ONE K2 launch over all slots (sjd_logits_to_probs_sample_part_slots_g) and,
        for a head window wide enough for K2a (LlamaGen's 16384 columns, Emu3), by K2a in front of every slot's K2 (sjd_head_combine_g): both read
        the engine's array.  The one-slot K2 over a NARROW head (SJD_SLOT_LAUNCHES=0) or over dense logits bakes one scalar into its graphs:
        refused, never decoded with the first prompt's value (cut line)."""
        if self._mixed_guidance:
            raise ValueError("prompts with different guidance scales need K2 as one launch over all slots or K2a in front of it, but this engine "
                             "launches K2 per slot over " + (why or "a narrow head window (SJD_SLOT_LAUNCHES=0)") + ": decode prompts of one "
                             "guidance scale per decode_many on this configuration")

    # ------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def decode_many(self, prompts: List[List[int]], specs: List[WindowSpec], grammars, cfg, seeds=None,
                    warmup_iters=0, timed_iters=None, on_timed_start=None, on_timed_end=None, detokenize=None):
        """cfg: one SJDConfig for all prompts (seed = cfg.seed + prompt index unless `seeds` is given), or a sequence of N, one per prompt: prompt
        j then decodes with cfg[j].guidance_scale and cfg[j].seed (as given: no index is added) -- exactly what it would decode alone with that
        config; the other fields must agree (per_prompt_configs).  Temperature, top-p and top-k are per prompt through `grammars`.  Returns
        [(sequence, DecodeStats)] in prompt order; with timed_iters the stats cover window iterations [warmup_iters, warmup_iters + timed_iters).

        len(prompts) may exceed the number of slots (continuous batching): a slot whose prompt reached its end token is handed the next
        prompt of the list -- state machine, grammar and generators re-created, its KV rows reused from 0, its prompt prefilled eagerly
        over its own batch rows -- while the other slots keep their windows; the captured window graphs are unaffected.  Only when the
        list is exhausted does a finished slot ride along with a one-row dummy window.

        detokenize: None, or a callable (the finished prompt's sequence, a 1-d LongTensor on the device) -> image tensor.  It is called when a
        prompt reaches its end, before the slot is handed the next prompt, eagerly on ONE side stream the engine owns (detok_stream): an event
        recorded on the decode stream, the side stream waits for it, the callable runs under torch.cuda.stream(side).  The decode stream never
        waits for the side stream, so the convolutions run under the window forwards of the other slots; the captured graphs hold none of the
        callable's buffers (it allocates under the side stream, from the allocator's pool of that stream, and the ids it reads are a tensor of
        their own per prompt, marked record_stream -- a refilled slot writes nowhere near them).  The side stream is synchronised once, at the
        end.  The return value is then (results, images): images[j] is prompt j's (None for a prompt a timed run never finished), and
        detok_events[j] the event recorded behind its callable.  A callable whose library searches its kernels on the first call of a shape
        (MIOpen convolutions: seconds) is best called once before decode_many (LlamaGenSolver.generate does)."""
        # GenerationConfig(do_sample=False): K2's MODE of p goes where its draw would (state.tokens; the draw lands in state.amax and is ignored),
        # nothing is consumed from a slot's generator for it, the verify step's draws follow at once (SJDEngine.decode, JL:124-129)
        N = len(prompts)
        cfg, cfgs = per_prompt_configs(cfg, N)
        # prompts that all share one scale (a list of equal configs included) take the scalar launches and graph keys of a single config
        self._mixed_guidance = cfgs is not None and len({float(c.guidance_scale) for c in cfgs}) > 1
        if not self.head_partials:
            self._refuse_mixed_guidance_per_slot("dense logits (the backbone hands out no head partials)")
        self._greedy = greedy = not getattr(cfg, "do_sample", True)
        assert len(specs) == len(grammars) == N and N >= self.P
        self._check_config(cfg, grammars)
        dev, nb = self.device, self.nb
        ph_blocks = ops.philox_max_blocks(dev)
        default_gen = torch.cuda.default_generators[dev.index if dev.index is not None else torch.cuda.current_device()]
        scheme = scheme_code(cfg.prefix_token_sampler_scheme)
        do_cfg = cfg.do_cfg and (cfg.guidance_scale != 1)
        self._guidance = float(cfg.guidance_scale)
        prompt_seed = lambda j: cfgs[j].seed if cfgs is not None else (None if cfg.seed is None else cfg.seed + j)
        attn = getattr(self.backbone, "attn", None)
        full_cache = self.backbone.cache
        results = [None] * N
        pre_seeds = None
        if seeds is None and any(prompt_seed(j) is None for j in range(N)) and any(getattr(sp, "cond_embeds", None) is not None for sp in specs):
            # no seed: the N per-prompt seeds are drawn from the default generator UP FRONT, in prompt order -- a prompt's first token (drawn at
            # its admission) then depends neither on the number of slots nor on which slot finished first
            pre_seeds = [int(t) for t in torch.randint(0, 2 ** 62, (N,), device=dev, generator=default_gen).tolist()]
        next_prompt = 0
        emitted_total = 0                 # tokens appended to any prompt's sequence so far (the timed region counts its increase)
        cur = 0

        def admit(i, buf):
            """prompt `next_prompt` -> slot i: iteration 0 (JL:344-350 short-circuit), a prefill over the slot's own batch rows whose
            distribution lands in probs[buf]"""
            nonlocal next_prompt
            j, s = next_prompt, self.slots[i]
            next_prompt += 1
            s.prompt_index = j
            seed = seeds[j] if seeds is not None else prompt_seed(j)
            guidance = float(cfgs[j].guidance_scale) if cfgs is not None else self._guidance
            if self._mixed_guidance:            # the slot's scale goes up stream-ordered, like its blob below: no synchronisation of its own
                self._guid_host[i] = guidance
                L.check(L.load().sjd_upload_async(self._guid_dev.data_ptr() + 4 * i, self._guid_host.data_ptr() + 4 * i, 4, ops._stream()),
                        "sjd_upload_async")
            cond = getattr(specs[j], "cond_embeds", None)
            self.key_start[i * nb:(i + 1) * nb].copy_(specs[j].key_start.to(device=dev, dtype=torch.int32))
            first_tok = None
            if cond is not None:
                # LlamaGen: the conditioning rows go into the slot's cache rows [0, T) through the ATen prefill (as the solo path's), the
                # first image token comes from the last row's logits, drawn from the PROMPT's generator (seed + j, or its up-front seed)
                from .llamagen_solver import sample as _lg_sample
                sk = dict(specs[j].cond_sampling or {})
                scale = float(sk.pop("cfg_scale", guidance))
                T = cond.shape[1]
                if specs[j].kv_base != T:
                    raise ValueError(f"WindowSpec.cond_embeds has {T} rows but kv_base = {specs[j].kv_base}: the window starts behind the conditioning")
                self.backbone.cache = _CacheView(full_cache, i * nb, (i + 1) * nb)
                try:
                    lg = self.backbone.forward_embeds(cond.to(dev), torch.arange(T, device=dev)[None].repeat(cond.shape[0], 1), 0,
                                                      self.key_start[i * nb:(i + 1) * nb])
                finally:
                    self.backbone.cache = full_cache
                if nb > 1 and scale > 1.0:
                    lg = lg[1:2] + (lg[0:1] - lg[1:2]) * scale
                else:
                    lg = lg[0:1]
                g0 = torch.Generator(dev).manual_seed(seed if seed is not None else pre_seeds[j])
                first_tok = int(_lg_sample(lg, generator=g0, **sk)[0][0, 0])
            if seed is None and pre_seeds is not None:
                s.gen = torch.Generator(dev).manual_seed(pre_seeds[j])
            elif seed is None:
                # no seed given: every slot needs its OWN Philox stream.  Sharing the device's default generator (round 3) handed every slot
                # the same (seed, offset) pair -- identical prompts in a batch then drew identical noise.  A per-slot seed is
                # drawn FROM the default generator instead: it advances with every admission, and torch.manual_seed still reproduces a run.
                slot_seed = int(torch.randint(0, 2 ** 62, (1,), device=dev, generator=default_gen).item())
                s.gen = torch.Generator(dev).manual_seed(slot_seed)
            else:
                s.gen = torch.Generator(dev).manual_seed(seed)
            PromptLoop.__init__(s, prompts[j] if first_tok is None else [first_tok], specs[j].kv_base, cfg, int(s.gen.initial_seed()), int(s.gen.get_offset()))
            s.cpu_gen = None if seed is None else torch.Generator().manual_seed(seed)     # the prompt's "global CPU generator" (JL:505)
            s.grammar = grammars[j]
            s.grammar.start(s.X)
            s.harvested, s.t_admit = False, time.perf_counter()
            self.pos_offset[i * nb:(i + 1) * nb].copy_(specs[j].pos_offset.to(device=dev, dtype=torch.int64))
            _, _, rules, _, _, use_cfg, _, offs = s.plan(cfg, s.grammar, s.cpu_gen, self.V, ph_blocks, greedy, scheme, do_cfg)
            self._fill_blob(s.params, 1, s.kv_len, use_cfg, s.launch_scheme(scheme), [], rules, [], (ph_blocks, s.ph_seed) + offs)
            s.params.upload()
            if self.hook is not None:
                self._observer_noise(s, s.gen, s.ph_off, 1, False)
            if first_tok is None:
                tokens, positions = specs[j].first_tokens.to(dev), specs[j].first_positions.to(dev)
            else:                                # the window starts as the solo path's: the first image token at position T
                tokens = torch.full((nb, 1), first_tok, dtype=torch.long, device=dev)
                positions = torch.full((nb, 1), specs[j].kv_base, dtype=torch.long, device=dev)
            self._calibrate_fp8(tokens, positions, self.key_start[i * nb:(i + 1) * nb])      # (an fp8 cache nobody calibrated: once per backbone)
            self.backbone.cache = _CacheView(full_cache, i * nb, (i + 1) * nb)
            try:
                logits = self.backbone.forward_window(tokens, positions, s.kv_len, self.key_start[i * nb:(i + 1) * nb])
            finally:
                self.backbone.cache = full_cache
            lc, lu = self._prefill_sample(s, logits, guidance, buf, nb)
            if self.hook is not None:
                self.hook(j, dict(first=True, n_rows=1, logits_c=lc, logits_u=lu, use_cfg=use_cfg, rules=rules, resid=[],
                                  noise=s.noise[:1], rs=s.rs[:1], noise2=s.noise2[0], probs=s.probs[buf], prev_probs=s.probs[1 - buf],
                                  ctx=list(s.X), scheme=scheme))
            s.win_len = tokens.shape[1]

        def read_back(s, win_len):
            """a slot's host bookkeeping after the state download (iteration 0: win_len = the rows of its prefill)"""
            nonlocal emitted_total
            st = s.state.view
            tok = st.tokens
            k = s.absorb(int(st.m), int(st.rejected), tok, tok if greedy else st.amax, win_len, cfg, s.grammar)
            emitted_total += k
            if k and self.hook is not None:
                s.gen.set_offset(s.ph_off)

        images, self.detok_events = [None] * N, [None] * N
        if detokenize is not None and getattr(self, "detok_stream", None) is None:
            self.detok_stream = torch.cuda.Stream(device=dev)      # one extra stream: the process uses two of its hardware queues

        def detok(s):
            """the finished prompt of slot s -> its image, on the side stream, ordered behind everything the decode stream has been given"""
            side, main = self.detok_stream, torch.cuda.current_stream(dev)
            ids = torch.tensor(s.X, dtype=torch.long, device=dev)
            ready = torch.cuda.Event()
            ready.record(main)
            side.wait_event(ready)
            ids.record_stream(side)
            with torch.cuda.stream(side):
                images[s.prompt_index] = detokenize(ids)
                done = torch.cuda.Event()
                done.record(side)
            self.detok_events[s.prompt_index] = done

        def harvest(s):
            s.harvested = True
            s.stats.wall_seconds = time.perf_counter() - s.t_admit
            s.stats.tokens, s.stats.timed_nfe, s.stats.kv_len = len(s.X) - s.P, s.stats.nfe, s.kv_len
            s.gen.set_offset(s.end_offset())                       # leave the generator where the reference's draws would have left it (coupled: behind the last position)
            results[s.prompt_index] = (s.X, s.stats)

        # ---------------- iteration 0 of the first P prompts ----------------
        if attn is not None and hasattr(attn, "params"):
            attn.params = None
        for i in range(self.P):
            admit(i, cur)
        self.state.wait_mirror()
        for s in self.slots:
            read_back(s, s.win_len)
        cur = 1 - cur
        if attn is not None and hasattr(attn, "params"):
            attn.params = self.params                          # windows: kv_len / n_rows of every prompt from its blob

        # ---------------- window iterations, all slots in lock-step ----------------
        it = 0
        timed_started = False
        t0 = time.perf_counter()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        tok0 = emitted_total
        host_s = sync_s = 0.0
        while True:
            # finished prompts leave, queued prompts enter (eager prefill; the window graphs hold none of the buffers it allocates)
            for i, s in enumerate(self.slots):
                if s.finished and not s.harvested:
                    harvest(s)
                    if detokenize is not None:
                        detok(s)
                    if next_prompt < N:
                        if attn is not None and hasattr(attn, "params"):
                            attn.params = None
                        admit(i, 1 - cur)
                        self.state.wait_mirror()
                        read_back(s, s.win_len)
                        if attn is not None and hasattr(attn, "params"):
                            attn.params = self.params
            if all(s.finished for s in self.slots):
                if any(not s.harvested for s in self.slots):
                    continue                                    # (a prompt that ended in its prefill iteration)
                break
            if timed_iters is not None and it == warmup_iters:
                timed_started = True
                if on_timed_start is not None:
                    on_timed_start()
                tok0 = emitted_total
                host_s = sync_s = 0.0
                t0 = time.perf_counter()
                ev0.record()
            t_h = time.perf_counter()
            rule_lists, metas, slow = [], [], []
            for s in self.slots:
                # (a finished slot rides along with a dummy one-row window: PromptLoop.plan)
                n_rows, fresh, rules, win, resid, use_cfg, _, offs = s.plan(cfg, s.grammar, s.cpu_gen, self.V, ph_blocks, greedy, scheme, do_cfg)
                if not s.finished:
                    rule_lists.append(rules)
                    if resid is None:                          # the grammar cannot name the residual rules before the launch
                        slow.append((s, win, len(metas)))
                self._fill_blob(s.params, n_rows, s.kv_len, use_cfg, s.launch_scheme(scheme), fresh, rules, resid or [], (ph_blocks, s.ph_seed) + offs)
                metas.append([n_rows, rules, resid, use_cfg])
            self.params.upload()
            cols = cached_column_window(self, rule_lists) if rule_lists else None      # the union of the slots' output-head column windows
            if self.hook is not None:
                for s in self.slots:
                    self._observer_noise(s, s.gen, s.ph_off, s.n_rows, s.draws_rs, keyed=s.keyed(scheme, s.kv_len))
            host_s += time.perf_counter() - t_h
            if slow:                                            # two stages: the missing residual rules are computed under the forward
                logits = self._launch_forward(cols)
                t_h = time.perf_counter()
                for s, win, k in slow:
                    metas[k][2] = s.grammar.residual_rules(win)
                    self._upload_resid(s.params, metas[k][2])
                host_s += time.perf_counter() - t_h
                self._launch_sample(cur, logits, cols)
            else:
                logits = self._launch_window(cur, cols)
            metas = [tuple(mt) for mt in metas]
            if self.hook is not None:
                part = isinstance(logits, ops.HeadOut)
                for i, (s, (n_rows, rules, resid, use_cfg)) in enumerate(zip(self.slots, metas)):
                    if s.finished:
                        continue
                    if part:                                   # the logits exactly as K2 derived them
                        lg = self._dbg[i * nb:(i + 1) * nb, :n_rows]
                    else:
                        lg = logits[i * nb:(i + 1) * nb, :n_rows]
                        if cols is not None:
                            full = torch.zeros(nb, n_rows, self.V, dtype=logits.dtype, device=dev)
                            full[:, :, cols[0]:cols[1]] = lg
                            lg = full
                    self.hook(s.prompt_index, dict(first=False, n_rows=n_rows, logits_c=lg[0], logits_u=lg[1] if nb > 1 else None,
                                                   use_cfg=use_cfg, rules=rules, resid=resid, noise=s.noise[:n_rows], rs=s.rs[:n_rows],
                                                   noise2=s.noise2[0], probs=s.probs[cur], prev_probs=s.probs[1 - cur], ctx=list(s.X),
                                                   scheme=scheme))
            t_s = time.perf_counter()
            self.state.wait_mirror()                              # the single sync of the iteration
            sync_s += time.perf_counter() - t_s
            for s, mt in zip(self.slots, metas):
                read_back(s, mt[0])
            cur = 1 - cur
            it += 1
            if timed_iters is not None and it == warmup_iters + timed_iters:
                break
        ev1.record()
        if detokenize is not None:
            self.detok_stream.synchronize()                    # the one wait for the side stream
        torch.cuda.synchronize()
        check_reduce_timeouts()                    # (a reducing projection that gave up a wait: wrong numbers must not become tokens -- ADVICE r3)
        if on_timed_end is not None and (timed_started or timed_iters is None):      # never an unmatched barrier (SJDEngine.decode)
            on_timed_end()
        seconds = ev0.elapsed_time(ev1) / 1000.0
        for s in self.slots:                                   # prompts still in flight when a timed run stops
            if not s.harvested:
                harvest(s)
        self.run_stats = dict(seconds=seconds, wall_seconds=time.perf_counter() - t0, iterations=it,
                              timed_iterations=(it - warmup_iters) if timed_iters is not None else it,
                              tokens=emitted_total - tok0, host_seconds=host_s, sync_seconds=sync_s, prompts_started=next_prompt,
                              timed_region_reached=bool(timed_started or timed_iters is None))
        out = []
        for r in results:
            if r is None:                                      # never admitted (a timed run that stopped early)
                out.append(None)
                continue
            X, st = r
            st.seconds, st.host_seconds, st.sync_seconds = seconds, host_s, sync_s
            out.append((X, st))
        if detokenize is not None:
            return out, images
        return out
