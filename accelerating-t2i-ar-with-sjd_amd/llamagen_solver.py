"""Mirror of reference llamagen/llamagen_solver.py: LlamaGenSolver, renew_llamagen, MaxlenCriteria and the baseline AR
sampler pieces (prefill / sample / top_k_top_p_filtering, which also produce the FIRST image token of the SJD path
from the global RNG, LS:75-104)."""
import torch
from torch.nn import functional as F

from . import launch_shapes as LS
from .engine import check_coupled, lenience_field
from .scheduler.logit_processor_3dim import TopKLogitsWarper, TopPLogitsWarper3d


def top_k_top_p_filtering(logits, top_k: int = 0, top_p: float = 1.0, filter_value: float = -float("Inf"), min_tokens_to_keep: int = 1):
    """Behaviour of reference LS:34-72 (used once per image, for the first token): keep the k largest logits, then the
    smallest descending-sorted prefix whose probability mass exceeds top_p (the token that crosses the threshold is kept)."""
    V = logits.size(-1)
    if top_k > 0:
        k = min(max(top_k, min_tokens_to_keep), V)
        kth = logits.topk(k, dim=-1).values[..., -1:]
        logits.masked_fill_(logits < kth, filter_value)
    if top_p < 1.0:
        order = logits.argsort(dim=-1, descending=True)
        mass = logits.gather(-1, order).softmax(dim=-1).cumsum(dim=-1)
        drop_sorted = torch.zeros_like(mass, dtype=torch.bool)
        drop_sorted[..., 1:] = mass[..., :-1] > top_p          # shifted by one: the crossing token survives
        if min_tokens_to_keep > 1:
            drop_sorted[..., :min_tokens_to_keep] = False
        drop = torch.zeros_like(drop_sorted).scatter(-1, order, drop_sorted)
        logits.masked_fill_(drop, filter_value)
    return logits


def sample(logits, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, sample_logits=True, noise_device=None, generator=None):
    """Behaviour of reference LS:75-84: last row / temperature -> filtering -> softmax -> one draw from the GLOBAL generator of the
    logits' device (noise_device="cpu": draw on the CPU generator instead -- replays the reference's CPU run on a GPU backbone).
    generator: draw from this torch.Generator instead (one per prompt when several prompts share a forward); None = the global one."""
    dev = logits.device
    if noise_device is not None:
        logits = logits.float().to(noise_device)
    last = logits[:, -1, :] / max(temperature, 1e-5)
    if top_k > 0 or top_p < 1.0:
        last = top_k_top_p_filtering(last, top_k=top_k, top_p=top_p)
    probs = last.softmax(dim=-1)
    if not sample_logits:
        idx = probs.argmax(dim=-1, keepdim=True)
    elif generator is None:
        idx = torch.multinomial(probs, num_samples=1)
    else:
        idx = torch.multinomial(probs, num_samples=1, generator=generator)
    return idx.to(dev), probs.to(dev)


def logits_to_probs(logits, temperature: float = 1.0, top_p: float = 1.0, top_k: int = None, **kwargs):
    """reference LS:86-91"""
    logits = logits / max(temperature, 1e-5)
    if (top_k or 0) > 0 or top_p < 1.0:
        logits = top_k_top_p_filtering(logits, top_k=top_k or 0, top_p=top_p)
    return logits.softmax(dim=-1)


def _ar_forward(model, tokens, pos, kv_len, key_start):
    """one AR step of the baseline decoder: a 1-row window through the same backbone (K3 append + K1 attention)"""
    if hasattr(model.attn, "params"):
        model.attn.params = None                      # kv_len by value: no SJD iteration blob in the plain AR loop
    return model.forward_window(tokens, pos, kv_len, key_start)


@torch.no_grad()
def generate(model, cond, max_new_tokens, emb_masks=None, cfg_scale=1.0, cfg_interval=-1, **sampling_kwargs):
    """The reference's plain auto-regressive LlamaGen decoder (LS:144-194: prefill + decode_n_tokens, one token per forward, every
    token drawn from the GLOBAL generator).  It is the non-SJD baseline `test_llamagen.py:20` imports next to the solver; here it
    runs on the same backbone and kernels (static cache, K1 with a 1-row window).  Returns LongTensor [B, max_new_tokens]."""
    if model.model_type == 'c2i':
        cond_combined = torch.cat([cond, torch.ones_like(cond) * model.num_classes]) if cfg_scale > 1.0 else cond
        T = 1
    elif model.model_type == 't2i':
        cond_combined = torch.cat([cond, torch.zeros_like(cond) + model.cls_embedding.uncond_embedding]) if cfg_scale > 1.0 else cond
        T = cond.shape[1]
    else:
        raise Exception("please check model type")
    B, dev = cond.shape[0], cond.device
    if B != 1:
        raise NotImplementedError("one prompt per call (the static cache rows of the CFG pair belong to one prompt)")
    Bc = cond_combined.shape[0]
    model.setup_cache(batch=Bc, s_max=((T + max_new_tokens + 32 + 31) // 32) * 32)
    for e in getattr(model, "_sjd_engines", {}).values():
        e.reset_graphs()
    if emb_masks is not None:
        assert emb_masks.shape[0] == B and emb_masks.shape[-1] == T                                     # LS:169-170
        masks = torch.cat([emb_masks, emb_masks]) if cfg_scale > 1.0 else emb_masks
        ks = (masks.long().cumsum(-1) == 0).sum(-1).to(device=dev, dtype=torch.int32)                  # masked (left-padded) cond rows
    else:
        ks = torch.zeros(Bc, dtype=torch.int32, device=dev)
    if getattr(model, "attn", None) is None:
        from . import ops
        model.attn = ops.HipWindowAttention()
    emb = model.embed_condition(cond_combined)
    pos = torch.arange(T, device=dev)[None].repeat(Bc, 1)
    if hasattr(model.attn, "params"):
        model.attn.params = None
    logits = model.forward_embeds(emb, pos, 0, ks)                                                       # prefill (LS:95-104)

    def combine(lg, use_cfg):
        if cfg_scale > 1.0:
            c, u = torch.split(lg, len(lg) // 2, dim=0)
            return u + (c - u) * cfg_scale if use_cfg else c
        return lg

    seq = torch.empty((B, max_new_tokens), dtype=torch.long, device=dev)
    tok = sample(combine(logits, True), **sampling_kwargs)[0]
    seq[:, 0:1] = tok
    cfg_flag = True
    for i in range(max_new_tokens - 1):                                                                  # decode_n_tokens (LS:123-142)
        if cfg_interval > -1 and i > cfg_interval:
            cfg_flag = False
        x = tok.view(-1, 1).repeat(Bc // B, 1)
        p_ = torch.full((Bc, 1), T + i, dtype=torch.long, device=dev)
        lg = _ar_forward(model, x, p_, T + i, ks)
        tok = sample(combine(lg, cfg_flag), **sampling_kwargs)[0]
        seq[:, i + 1:i + 2] = tok
    return seq


_PER_PROMPT_ARGS = ("cfg_scale", "temperature", "top_k", "top_p")


def per_prompt_values(name, value, n_prompts):
    """generate()'s cfg_scale / temperature / top_k / top_p: a number -> None (one value for every prompt, as ever); a sequence or 1-d tensor ->
    its n_prompts Python numbers, one per prompt.  Raises ValueError for a wrong length and for a sequence with one prompt per call."""
    if isinstance(value, torch.Tensor):
        if value.ndim == 0:
            return None
        value = value.flatten().tolist()
    elif hasattr(value, "tolist") and getattr(value, "ndim", 0) >= 1:          # numpy
        value = value.tolist()
    if not isinstance(value, (list, tuple)):
        return None
    if n_prompts <= 1:
        raise ValueError(f"{name} was given as a sequence of {len(value)} values, but generate() got one prompt: a value per prompt needs "
                         "several prompts per call (pass a number)")
    if len(value) != n_prompts:
        raise ValueError(f"{name} has {len(value)} values for {n_prompts} prompts: pass one number, or one per prompt")
    return list(value)


class MaxlenCriteria:
    """reference LS:341-347"""

    def __init__(self, max_seq_length):
        self.max_seq_length = max_seq_length

    def __call__(self, input_ids, scores, **kwargs):
        return input_ids.shape[-1] >= self.max_seq_length


def renew_llamagen(model_class):
    class WrappedLLamaGen(model_class):
        """reference LS:196-339.  The static KV cache already lives in the backbone; assign_kvcache/assign_past_key_values
        (the DynamicCache bridge) have no counterpart because rollback is a length update."""

        def _init_new_params(self, *args, **kwargs):
            self.is_encoder_decoder = False

        def clear_kvcache(self):
            if self.cache is not None:
                self.cache.k.zero_()
                self.cache.v.zero_()

    return WrappedLLamaGen


class LlamaGenSolver:
    """reference LS:349-470"""

    def __init__(self, model, image_top_k, image_top_p, noise_device=None, prompts_per_forward=None, lenience=1.0):
        self.model = model
        # LOSSY, off by default: SJDConfig.lenience of every generate() -- the verify step accepts a draft with min(1, lenience * p / q).  1.0 is
        # the exact rule (a model renewed with a lenience of its own then keeps that); anything else is refused here unless it is a finite bf16
        # value >= 1 on the speculative scheme
        if lenience == 1.0:
            lenience = getattr(model, "lenience", 1.0)
        lenience_field(lenience, getattr(model, "prefix_token_sampler_scheme", "speculative_jacobi"))
        self.lenience = float(lenience)
        # generate() with several prompts: how many share one window forward (None: as many as the kernels' row limit allows)
        self.prompts_per_forward = prompts_per_forward
        self.image_top_k = image_top_k
        self.image_top_p = image_top_p
        # None: every draw on the model's device, as the reference does.  "cpu": the first-token draw and the SJD noise streams come
        # from CPU generators (the golden fixtures were produced by CPU runs of the reference)
        # (a model renewed with prefix_token_sampler_scheme='coupled_jacobi' generates its noise in K2, by position: no host noise stream)
        check_coupled(getattr(model, "prefix_token_sampler_scheme", "speculative_jacobi"), noise_device)
        self.noise_device = noise_device

    def create_logits_processor(self, top_k=None, top_p=None, temperature=None):
        """top_k / top_p / temperature: one prompt's own values (generate() with a value per prompt); None: the solver's, temperature 1"""
        from transformers.generation.logits_process import LogitsProcessorList, TemperatureLogitsWarper
        procs = [TopKLogitsWarper(top_k=self.image_top_k if top_k is None else int(top_k)),
                 TopPLogitsWarper3d(top_p=self.image_top_p if top_p is None else float(top_p))]
        if temperature is not None and float(temperature) != 1.0:          # ahead of top-p: the order of `sample` (and of the kernels)
            procs.insert(0, TemperatureLogitsWarper(float(temperature)))
        return LogitsProcessorList(procs)

    @torch.no_grad()
    def prefill(self, cond_combined, cfg_scale, **sampling_kwargs):
        """reference LS:95-104 + 396-419: conditioning rows -> cache rows [0,T); first image token from the GLOBAL RNG."""
        model = self.model
        emb = model.embed_condition(cond_combined)
        Bc, T = emb.shape[0], emb.shape[1]
        pos = torch.arange(T, device=emb.device)[None].repeat(Bc, 1)
        ks = getattr(model, "_sjd_key_start", None)
        ks = torch.zeros(Bc, dtype=torch.int32, device=emb.device) if ks is None else torch.as_tensor(ks, dtype=torch.int32, device=emb.device)
        if hasattr(model.attn, "params"):
            model.attn.params = None
        logits = model.forward_embeds(emb, pos, 0, ks)
        if cfg_scale > 1.0:
            cond_logits, uncond_logits = torch.split(logits, len(logits) // 2, dim=0)
            logits = uncond_logits + (cond_logits - uncond_logits) * cfg_scale
        return sample(logits, noise_device=self.noise_device, **sampling_kwargs)[0], T

    @torch.no_grad()
    def generate(self, cond, max_new_tokens, emb_masks=None, cfg_scale=1.0, cfg_interval=-1, vq_model=None, qzshape=None, **sampling_kwargs):
        """cond with N > 1 prompts: cfg_scale, temperature, top_k and top_p each take a number (as ever) or N values, one per prompt
        (_generate_many).

        vq_model: None -> the ids, LongTensor [N, max_new_tokens], as ever.  A detokenizers.LlamaGenVQ -> (ids, images): images uint8
        [N, H, W, 3] on the model's device, image j = to_uint8(vq_model.decode_code(ids[j], (1, e_dim, h, w))).  qzshape: (e_dim, h, w) or
        (N, e_dim, h, w) of the latent; default: the codebook's width and a square of max_new_tokens codes.  With N > 1 every image is
        decoded on the batch engine's side stream as soon as its prompt ends, under the window forwards of the others."""
        model = self.model
        scheme_name = getattr(model, "prefix_token_sampler_scheme", "speculative_jacobi")
        check_coupled(scheme_name, self.noise_device)              # (the model may have been renewed since the solver was built)
        lenience_field(self.lenience, scheme_name)
        if vq_model is not None:
            qzshape = self._qzshape(vq_model, qzshape, cond.shape[0], max_new_tokens)
        if cond.shape[0] > 1:
            return self._generate_many(cond, max_new_tokens, emb_masks, cfg_scale, vq_model=vq_model, qzshape=qzshape, **sampling_kwargs)
        for name in _PER_PROMPT_ARGS:
            per_prompt_values(name, cfg_scale if name == "cfg_scale" else sampling_kwargs.get(name), 1)
        if model.model_type == 'c2i':
            cond_combined = torch.cat([cond, torch.ones_like(cond) * model.num_classes]) if cfg_scale > 1.0 else cond
            T = 1
        elif model.model_type == 't2i':
            cond_combined = torch.cat([cond, torch.zeros_like(cond) + model.cls_embedding.uncond_embedding]) if cfg_scale > 1.0 else cond
            T = cond.shape[1]
        else:
            raise Exception("please check model type")
        Bc = cond_combined.shape[0]
        s_max = ((T + max_new_tokens + model.max_num_new_tokens + 32 + 31) // 32) * 32
        model.setup_cache(batch=Bc, s_max=s_max)
        for e in getattr(model, "_sjd_engines", {}).values():
            e.reset_graphs()
        if emb_masks is not None:
            # left-padded caption masks: the masked conditioning rows are a hidden key prefix (LS:403-412)
            masks = torch.cat([emb_masks, emb_masks]) if cfg_scale > 1.0 else emb_masks
            model._sjd_key_start = (masks.long().cumsum(-1) == 0).sum(-1).to(torch.int32)
        else:
            model._sjd_key_start = None
        model.sjd_noise_device = self.noise_device
        model.lenience = self.lenience
        next_token, T = self.prefill(cond_combined, cfg_scale, **sampling_kwargs)
        from transformers import GenerationConfig
        generation_config = GenerationConfig(max_new_tokens=T + max_new_tokens, max_length=T + max_new_tokens, temperature=1.0,
                                             top_k=None, do_sample=True, return_dict_in_generate=False)
        outputs = model._sample(input_ids=next_token, logits_processor=self.create_logits_processor(),
                                stopping_criteria=[MaxlenCriteria(max_new_tokens)], generation_config=generation_config,
                                synced_gpus=False, streamer=None, logits_warper=None, use_cache=True,
                                attention_mask=torch.ones((1, T + 1), device=cond.device), past_key_values=None,
                                cache_position=T + 1)
        generated = outputs[:, -max_new_tokens:]
        model.clear_kvcache()
        if vq_model is not None:
            from .detokenizers import to_uint8
            return generated, to_uint8(vq_model.decode_code(generated.reshape(-1), (1,) + qzshape))
        return generated

    @staticmethod
    def _qzshape(vq_model, qzshape, n_prompts, max_new_tokens):
        """generate()'s qzshape -> (e_dim, h, w) of one image's latent"""
        if qzshape is None:
            side = int(round(max_new_tokens ** 0.5))
            qzshape = (vq_model.quantize.embedding.weight.shape[1], side, side)
        qzshape = tuple(int(x) for x in qzshape)
        if len(qzshape) == 4:
            if qzshape[0] != n_prompts:
                raise ValueError(f"qzshape {qzshape} is for {qzshape[0]} images, but generate() got {n_prompts} prompts")
            qzshape = qzshape[1:]
        if len(qzshape) != 3 or qzshape[1] * qzshape[2] != max_new_tokens:
            raise ValueError(f"qzshape {qzshape}: (e_dim, h, w) with h * w = max_new_tokens = {max_new_tokens}")
        return qzshape

    def slots_for(self, n_prompts, n_batch):
        """prompts per window forward: prompts_per_forward, or what the row limit allows: 256 rows; an fp16 backbone that was not packed for them
        (enable_fused(max_rows=256, untuned_fp16=True)) keeps its 128"""
        model = self.model
        slots = self.prompts_per_forward or max(1, LS.llamagen_row_limit(model) // (n_batch * model.max_num_new_tokens))
        return max(1, min(int(slots), n_prompts))

    def _generate_many(self, cond, max_new_tokens, emb_masks=None, cfg_scale=1.0, vq_model=None, qzshape=None, **sampling_kwargs):
        """N > 1 prompts (class ids [N], or caption embeddings [N, T, C] with emb_masks [N, T]): slots_for(N) of them share every window
        forward (SJDBatchEngine), the rest enter as slots finish.  Returns LongTensor [N, max_new_tokens] in prompt order.

        cfg_scale / temperature / top_k / top_p as numbers mean what they mean for one prompt: the settings of the FIRST image token's draw (the
        windows use the sampler's guidance_scale and the solver's image_top_k / image_top_p).  Given as N values, value j is prompt j's setting
        for its whole decode: its first draw AND its windows (guidance scale in K2, temperature / top-k / top-p in its rules), so a batch may
        mix them; prompt j then equals what it gives decoded alone with those settings and seed + j."""
        from .engine import WindowSpec
        model = self.model
        N, dev = cond.shape[0], cond.device
        scales = per_prompt_values("cfg_scale", cfg_scale, N)
        per = {k: per_prompt_values(k, sampling_kwargs[k], N) for k in _PER_PROMPT_ARGS[1:] if k in sampling_kwargs}
        per = {k: v for k, v in per.items() if v is not None}
        if getattr(model, "_ops", None) is None:
            raise ValueError(f"generate() with {N} prompts runs on the fused HIP path only: call model.enable_fused(ops, gemm='sjd', "
                             "max_rows=128 or 256) first, or generate one prompt per call")
        if self.noise_device is not None:
            raise ValueError(f"generate() with {N} prompts draws its noise in the kernels: noise_device={self.noise_device!r} is served for "
                             "one prompt per call only (use noise_device=None)")
        do_cfg = bool(model.do_cfg) and (model.guidance_scale != 1)
        for j, sc in enumerate([cfg_scale] if scales is None else scales):
            if do_cfg != (sc > 1.0):
                raise ValueError(f"cfg_scale {sc}" + ("" if scales is None else f" of prompt {j}") + " at prefill must match do_cfg / guidance_scale "
                                 f"of the sampler (do_cfg={do_cfg}): a batch is CFG-on or CFG-off as a whole")
        nb = 2 if do_cfg else 1
        if model.model_type == 'c2i':
            T = 1
        elif model.model_type == 't2i':
            T = cond.shape[1]
        else:
            raise Exception("please check model type")
        if emb_masks is not None:
            assert emb_masks.shape[0] == N and emb_masks.shape[-1] == T
        slots = self.slots_for(N, nb)
        s_max = ((T + max_new_tokens + model.max_num_new_tokens + 32 + 31) // 32) * 32
        model.setup_cache(batch=slots * nb, s_max=s_max)
        for e in getattr(model, "_sjd_engines", {}).values():
            e.reset_graphs()
        model._sjd_key_start = None
        model.sjd_noise_device = None
        model.lenience = self.lenience
        specs = []
        for j in range(N):
            c = cond[j:j + 1]
            if model.model_type == 'c2i':
                cc = torch.cat([c, torch.ones_like(c) * model.num_classes]) if nb > 1 else c
            else:
                cc = torch.cat([c, torch.zeros_like(c) + model.cls_embedding.uncond_embedding]) if nb > 1 else c
            if emb_masks is not None:            # left-padded caption masks: every prompt its own hidden key prefix (LS:403-412)
                ks = (emb_masks[j:j + 1].long().cumsum(-1) == 0).sum(-1).to(torch.int32).repeat(nb)
            else:
                ks = torch.zeros(nb, dtype=torch.int32)
            specs.append(WindowSpec(first_tokens=None, first_positions=None, key_start=ks, pos_offset=torch.zeros(nb, dtype=torch.long),
                                    kv_base=T, cond_embeds=model.embed_condition(cc),
                                    cond_sampling=dict(sampling_kwargs, cfg_scale=cfg_scale if scales is None else float(scales[j]),
                                                       **{k: v[j] for k, v in per.items()})))
        from transformers import GenerationConfig
        generation_config = GenerationConfig(max_new_tokens=T + max_new_tokens, max_length=T + max_new_tokens, temperature=1.0,
                                             top_k=None, do_sample=True, return_dict_in_generate=False)
        procs = [self.create_logits_processor(**{k: v[j] for k, v in per.items()}) for j in range(N)]
        detok = None
        if vq_model is not None:
            from .detokenizers import to_uint8
            detok = lambda ids: to_uint8(vq_model.decode_code(ids[-max_new_tokens:], (1,) + qzshape))[0]
            # one image of this shape BEFORE the queue starts: the convolution library searches its kernels on the first call of a shape, which
            # takes seconds; here it runs on an idle device and not on the side stream next to the window forwards
            detok(torch.zeros(max_new_tokens, dtype=torch.long, device=dev))
        outputs = model._sample_many(specs, procs, [MaxlenCriteria(max_new_tokens)], generation_config, slots,
                                     guidance_scales=None if scales is None else [float(x) for x in scales], detokenize=detok)
        if detok is not None:
            outputs, images = outputs
        generated = outputs[:, -max_new_tokens:]
        model.clear_kvcache()
        if detok is not None:
            return generated, torch.stack(images)
        return generated
