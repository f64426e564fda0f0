"""A guidance scale (and sampler settings, and a seed) PER PROMPT in the several-prompt engine.

  1. kernel K2, slot form with a device array of scales (sjd_logits_to_probs_sample_part_slots_g): every slot bit for bit what the EXISTING
     one-slot entry point (sjd_logits_to_probs_sample_part, scalar) gives that slot alone with its scale -- probabilities, tokens, argmax rows,
     zero states; both slot orders of the scales, both probability-buffer parities, CFG on in some slots and off in others, every slot its
     own row count, V = 16384 and a vocabulary that is no multiple of 32;
  2. an array of one repeated value against today's scalar slot launch;
  3. SJDBatchEngine.decode_many with one SJDConfig per prompt, six prompts on four slots (slots are refilled and change their scale mid-run):
     every prompt decodes what it decodes with its own single config; the window graphs do not multiply with the scales;
  4. LlamaGenSolver.generate with five class ids and five cfg_scale values.

The equalities are measured against the single-config / scalar code path, never against the per-prompt path itself.  In 3 and 4 the reference
decode of prompt j runs at the SAME number of slots (every slot decoding prompt j with prompt j's seed): the window forward picks its GEMM
kernel by the row count, and only equal kernels promise equal logits bits (tests/test_gpu_llamagen_batch.py compares first tokens only across
slot counts for the same reason).
"""
import ctypes

import pytest
import torch

import sjd_amd._lib as L
import sjd_amd.ops as ops
from tests.helpers import make_llamagen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALES = [1.0, 1.5, 3.0, 7.5, 0.0, -2.0, 4.0, 2.25]
ROWS = [16, 9, 1, 12, 16, 5, 2, 13]
USE_CFG = [1, 1, 0, 1, 1, 0, 1, 1]


# ------------------------------------------------------------------------------------------------ 1 / 2: the kernel
def _rules(V, i):
    """row rules of slot i: a range window with top-k and a temperature, a forced row, an open row with top-k / top-p"""
    lo, hi = 4 + 32 * i, min(V - 3, 8196)
    body = ops.make_rule(((lo, hi),), -1, 2000, None, temperature=1.0 + 0.25 * (i % 3))
    open_ = ops.make_rule((), -1, 50 + i, 0.9)
    forced = ops.make_rule(((lo, hi),), hi - 1 - i, 2000, None)
    return [(body, open_, body, forced)[(r + i) % 4] for r in range(16)]


def _k2_buffers(n_slots, V, Lmax, dev):
    params, state = ops.BlobArray(L.IterParams, n_slots, dev), ops.BlobArray(L.State, n_slots, dev)
    state.mirror_array()
    return dict(params=params, state=state, probs=torch.zeros(n_slots, 2, Lmax, V, device=dev),
                zst=torch.full((n_slots, 2, Lmax, 2), -1, dtype=torch.int32, device=dev), scratch=torch.empty(n_slots, V, device=dev))


def _k2_fill(b, n_slots, V, it, blocks):
    for i in range(n_slots):
        p = b["params"].blobs[i].view
        n = ROWS[(i + it) % 8]
        p.n_rows, p.kv_len, p.use_cfg, p.scheme, p.batch_rows = n, 12 + i, USE_CFG[i], 0, 2
        for j, r in enumerate(_rules(V, i)):
            p.rules[j] = r
        p.philox_blocks, p.philox_seed = blocks, 1000 + i
        p.philox_offset[0] = 40 * it
    b["params"].upload()


def _head(n_slots, V, Lmax, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    hidden, n_chunks = 1024, 3
    prows = ops._prows(n_slots * 2 * Lmax)
    part = ops.Partials(torch.randn(n_chunks, prows, V, generator=g, device=dev) * 1.5, n_chunks, V)
    sumsq = hidden / 4 * (0.5 + torch.rand(4, prows, generator=g, device=dev))
    return ops.HeadOut(part, 0, Lmax, torch.bfloat16, row_norm=(sumsq, hidden, 1e-5))


def _k2_one_slot_scalar(head, scale, b, i, cur, Lmax, V, dev):
    """the EXISTING entry point, one slot, its scalar: sjd_logits_to_probs_sample_part (called directly: no K2a in front of it)"""
    hp = ops._head_partials(head, Lmax, V, torch.device(dev), None, i * 2 * Lmax, Lmax, b["zst"][i, cur])
    s0 = b["state"].blobs[i]
    L.check(L.load().sjd_logits_to_probs_sample_part(ctypes.byref(hp), float(scale), Lmax, V, b["params"].blobs[i].ptr, None,
                                                    ctypes.c_void_p(b["probs"][i, cur].data_ptr()), s0.field_ptr("tokens"), s0.field_ptr("amax"),
                                                    ops._stream()), "sjd_logits_to_probs_sample_part")


def _same(a, b, what):
    assert torch.equal(a["probs"].view(torch.int32), b["probs"].view(torch.int32)), f"{what}: probabilities"
    assert torch.equal(a["zst"], b["zst"]), f"{what}: zero states"
    assert torch.equal(a["state"].dev, b["state"].dev), f"{what}: tokens / argmax rows"


@pytest.mark.parametrize("V", [16384, 9001])
@pytest.mark.parametrize("n_slots", [1, 2, 5, 8])
def test_k2_slot_guidance_array_equals_scalar_launch_per_slot(n_slots, V):
    dev, Lmax = DEV, 16
    head = _head(n_slots, V, Lmax, dev, 100 * n_slots + V)
    blocks = ops.philox_max_blocks(torch.device(dev))
    for order in (1, -1):                       # both slot orders of the scales: a slot that read its neighbour's would be seen
        scales = SCALES[:n_slots][::order]
        a, b = _k2_buffers(n_slots, V, Lmax, dev), _k2_buffers(n_slots, V, Lmax, dev)
        garr = torch.tensor(scales, dtype=torch.float32, device=dev)
        sl = ops.slots_of(b["params"], b["state"], b["probs"], b["zst"], b["scratch"], 2)
        for it in range(3):                     # parities 0, 1, 0: the third launch meets the zero state the first one left
            cur = it & 1
            _k2_fill(a, n_slots, V, it, blocks)
            _k2_fill(b, n_slots, V, it, blocks)
            for i in range(n_slots):
                _k2_one_slot_scalar(head, scales[i], a, i, cur, Lmax, V, dev)
            ops.logits_to_probs_sample_part_slots(sl, head, garr, b["params"], b["probs"], cur, "tokens", "amax", b["state"], b["zst"], 2)
            torch.cuda.synchronize()
            _same(a, b, f"order {order}, launch {it}")
            assert float(b["probs"][:, cur].sum()) > n_slots - 0.5
            assert int((b["zst"][:, cur, 0] >= 0).sum()) >= n_slots, "the zero state was written"
        if n_slots > 1:                         # the scales matter: the same launch with the array reversed gives other numbers where CFG is on
            c = _k2_buffers(n_slots, V, Lmax, dev)
            _k2_fill(c, n_slots, V, 0, blocks)
            slc = ops.slots_of(c["params"], c["state"], c["probs"], c["zst"], c["scratch"], 2)
            ops.logits_to_probs_sample_part_slots(slc, head, garr.flip(0).contiguous(), c["params"], c["probs"], 0, "tokens", "amax", c["state"],
                                                  c["zst"], 2)
            a0 = _k2_buffers(n_slots, V, Lmax, dev)
            _k2_fill(a0, n_slots, V, 0, blocks)
            for i in range(n_slots):
                _k2_one_slot_scalar(head, scales[i], a0, i, 0, Lmax, V, dev)
            torch.cuda.synchronize()
            assert not torch.equal(a0["probs"][0, 0], c["probs"][0, 0])


@pytest.mark.parametrize("n_slots,V", [(5, 16384), (8, 9001)])
def test_k2_slot_guidance_array_of_one_value_equals_scalar_slot_launch(n_slots, V):
    dev, Lmax = DEV, 16
    head = _head(n_slots, V, Lmax, dev, 7 * n_slots + V)
    blocks = ops.philox_max_blocks(torch.device(dev))
    a, b = _k2_buffers(n_slots, V, Lmax, dev), _k2_buffers(n_slots, V, Lmax, dev)
    sla = ops.slots_of(a["params"], a["state"], a["probs"], a["zst"], a["scratch"], 2)
    slb = ops.slots_of(b["params"], b["state"], b["probs"], b["zst"], b["scratch"], 2)
    garr = torch.full((n_slots,), 3.0, dtype=torch.float32, device=dev)
    for it in range(2):
        _k2_fill(a, n_slots, V, it, blocks)
        _k2_fill(b, n_slots, V, it, blocks)
        ops.logits_to_probs_sample_part_slots(sla, head, 3.0, a["params"], a["probs"], it, "tokens", "amax", a["state"], a["zst"], 2)
        ops.logits_to_probs_sample_part_slots(slb, head, garr, b["params"], b["probs"], it, "tokens", "amax", b["state"], b["zst"], 2)
        torch.cuda.synchronize()
        _same(a, b, f"launch {it}")


def test_k2_slot_guidance_array_is_checked():
    head = _head(2, 9001, 16, DEV, 3)
    b = _k2_buffers(2, 9001, 16, DEV)
    sl = ops.slots_of(b["params"], b["state"], b["probs"], b["zst"], b["scratch"], 2)
    for bad in (torch.zeros(3, device=DEV), torch.zeros(2, dtype=torch.float64, device=DEV), torch.zeros(2)):
        with pytest.raises(ValueError, match="per-slot guidance"):
            ops.logits_to_probs_sample_part_slots(sl, head, bad, b["params"], b["probs"], 0, "tokens", "amax", b["state"], b["zst"], 2)


# ------------------------------------------------------------------------------------------------ 2b: K2a with the scale in device memory
@pytest.mark.parametrize("scale", [7.5, 0.0, -2.0])
def test_k2a_guidance_from_device_memory_equals_scalar(scale):
    """sjd_head_combine_g against the existing sjd_head_combine with that value: the guided scores, then K2 behind both, bit for bit; the
    scale is read from the MIDDLE of an array whose neighbours hold other values"""
    dev, Lmax, V = DEV, 16, 16384
    head = _head(1, V, Lmax, dev, 11)
    blocks = ops.philox_max_blocks(torch.device(dev))
    a, b = _k2_buffers(1, V, Lmax, dev), _k2_buffers(1, V, Lmax, dev)
    _k2_fill(a, 1, V, 1, blocks)                    # nine rows of the sixteen
    _k2_fill(b, 1, V, 1, blocks)
    garr = torch.tensor([123.0, scale, -55.0], dtype=torch.float32, device=dev)
    hp = ops._head_partials(head, Lmax, V, torch.device(dev), None, 0, Lmax, None)
    assert ops.head_combine_ok(hp)
    za, zb = torch.full((Lmax, V), -7.0, device=dev), torch.full((Lmax, V), -7.0, device=dev)
    L.check(L.load().sjd_head_combine(ctypes.byref(hp), float(scale), Lmax, V, a["params"].blobs[0].ptr, ctypes.c_void_p(za.data_ptr()), ops._stream()), "K2a")
    L.check(L.load().sjd_head_combine_g(ctypes.byref(hp), ctypes.c_void_p(garr.data_ptr() + 4), Lmax, V, b["params"].blobs[0].ptr,
                                        ctypes.c_void_p(zb.data_ptr()), ops._stream()), "K2a, pointer form")
    torch.cuda.synchronize()
    assert torch.equal(za.view(torch.int32), zb.view(torch.int32))
    # (bf16-rounded scores: a few of the 262144 may BE the fill value) every row of the window was written, none beyond it
    assert float((za[:ROWS[1]] == -7.0).float().mean()) < 0.01 and (za[ROWS[1]:] == -7.0).all()
    for s_, g in ((a, float(scale)), (b, garr[1:2])):
        s0 = s_["state"].blobs[0]
        ops.logits_to_probs_sample_part(head, g, s_["params"].blobs[0], None, s_["probs"][0, 0], s0.field_ptr("tokens"), amax_out_ptr=s0.field_ptr("amax"),
                                        row0=0, urow_off=Lmax, zero_state=s_["zst"][0, 0])
    torch.cuda.synchronize()
    _same(a, b, "K2 behind K2a")
    narrow = _head(1, 9001, Lmax, dev, 12)
    with pytest.raises(ValueError, match="wide enough for K2a"):
        ops.logits_to_probs_sample_part(narrow, garr[1:2], b["params"].blobs[0], None, torch.zeros(Lmax, 9001, device=dev), b["state"].blobs[0].field_ptr("tokens"))


# ------------------------------------------------------------------------------------------------ 3: the engine
# vocabulary 4096: K2 of all slots is ONE launch (the array form under test); 16384 (LlamaGen's): the head is wide enough for K2a, which runs in
# front of every slot's own K2 and takes the slot's element of the array by pointer
def _toy_args(vocab):
    return dict(dim=128, n_layer=2, n_head=2, vocab_size=vocab, block_size=256, cls_token_num=1, model_type="c2i", num_classes=1000)


TOY_C2I = _toy_args(16384)
P_SCALES = [1.5, 3.0, 4.0, 7.5, 2.0, 5.5]
P_TEMPS = [1.0, 0.8, 1.0, 1.25, 0.9, 1.0]
P_TOP_P = [1.0, 0.95, 0.9, 1.0, 1.0, 0.85]
P_SEEDS = [7, 1234, 99, 5, 42, 31337]
N_SLOTS, WINDOW, NTOK = 4, 16, 128          # 128 image tokens per prompt: every slot is refilled well before the others end
_toy = {}


def _model(vocab):
    if ("model", vocab) not in _toy:
        m = make_llamagen(_toy_args(vocab), 17, 0.25, ops.HipWindowAttention(n_split=2), dtype=torch.bfloat16, device=DEV)
        m.enable_fused(ops, gemm="sjd", max_rows=128)
        m.setup_cache(batch=2 * N_SLOTS, s_max=((1 + 256 + 64 + 31) // 32) * 32)
        _toy["model", vocab] = m
    return _toy["model", vocab]


def _spec(model, j):
    from sjd_amd.engine import WindowSpec
    cond = torch.tensor([(207 + 101 * j) % 1000, model.num_classes], device=DEV)
    return WindowSpec(first_tokens=None, first_positions=None, key_start=torch.zeros(2, dtype=torch.int32), pos_offset=torch.zeros(2, dtype=torch.long),
                      kv_base=1, cond_embeds=model.embed_condition(cond),
                      cond_sampling=dict(temperature=P_TEMPS[j], top_k=1000, top_p=P_TOP_P[j], sample_logits=True))


def _grammar(j):
    from sjd_amd.grammar import TopKTopPGrammar
    g = TopKTopPGrammar(1000, P_TOP_P[j])
    g.temperature = P_TEMPS[j]
    return g


def _config(j, vocab):
    """(img_vocab_lo / img_vocab_n: the fresh draft ids must lie inside the toy's vocabulary -- the default range ends at 8196)"""
    from sjd_amd.engine import SJDConfig
    return SJDConfig(jacobi_loop_interval_l=1, jacobi_loop_interval_r=NTOK - WINDOW - 2, max_num_new_tokens=WINDOW, guidance_scale=P_SCALES[j],
                     seed=P_SEEDS[j], max_length=NTOK, img_vocab_lo=0, img_vocab_n=min(8192, vocab))


def _engine(vocab, use_graph):
    from sjd_amd.engine_batch import SJDBatchEngine
    eng = SJDBatchEngine(_model(vocab), vocab, DEV, N_SLOTS, max_window=WINDOW, use_graph=use_graph)
    assert eng.head_partials and eng.slot_launches
    return eng


def _solo_references(vocab):
    """prompt j with its own SINGLE config (the existing path: scalar guidance, scalar graph keys), every slot of the same engine geometry
    decoding that one prompt with that one seed; computed once per vocabulary"""
    if ("solo", vocab) not in _toy:
        eng = _engine(vocab, True)
        solo = []
        for j in range(len(P_SCALES)):
            res = eng.decode_many([[] for _ in range(N_SLOTS)], [_spec(_model(vocab), j) for _ in range(N_SLOTS)], [_grammar(j) for _ in range(N_SLOTS)],
                                  _config(j, vocab), seeds=[P_SEEDS[j]] * N_SLOTS)
            assert all(r[0] == res[0][0] and r[1].matched == res[0][1].matched for r in res), "the slots of one solo run agree"
            solo.append((list(res[0][0]), list(res[0][1].matched)))
        assert len({tuple(s) for s, _ in solo}) == len(solo)
        _toy["solo", vocab] = solo
    return _toy["solo", vocab]


class _Spy:
    """records the `guidance` argument of the two K2 wrappers of ops while a decode runs"""

    def __enter__(self):
        self.slots, self.one, self._real = [], [], (ops.logits_to_probs_sample_part_slots, ops.logits_to_probs_sample_part)
        ops.logits_to_probs_sample_part_slots = lambda sl, head, g, *a, **k: (self.slots.append(g), self._real[0](sl, head, g, *a, **k))[1]
        ops.logits_to_probs_sample_part = lambda head, g, *a, **k: (self.one.append(g), self._real[1](head, g, *a, **k))[1]
        return self

    def __exit__(self, *exc):
        ops.logits_to_probs_sample_part_slots, ops.logits_to_probs_sample_part = self._real


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("vocab", [4096, 16384], ids=["slot-launch", "wide-head-k2a"])
def test_decode_many_one_config_per_prompt(vocab, use_graph):
    solo = _solo_references(vocab)
    n = len(P_SCALES)
    eng = _engine(vocab, use_graph)
    with _Spy() as spy:
        res = eng.decode_many([[] for _ in range(n)], [_spec(_model(vocab), j) for j in range(n)], [_grammar(j) for j in range(n)],
                              [_config(j, vocab) for j in range(n)])
    if vocab == 4096:
        assert spy.slots and not spy.one and all(isinstance(g, torch.Tensor) and g.numel() == N_SLOTS for g in spy.slots), \
            "K2 ran as the slot launch that reads the scales from the array"
    else:
        assert spy.one and not spy.slots and all(isinstance(g, torch.Tensor) and g.numel() == 1 for g in spy.one), "K2a took the scale by pointer"
    for j, (seq, stats) in enumerate(res):
        assert len(seq) == NTOK
        assert seq[0] == solo[j][0][0], f"prompt {j}: first image token"
        assert seq == solo[j][0], f"prompt {j}: token sequences differ"
        assert stats.matched == solo[j][1], f"prompt {j}: accept lengths differ"
    if use_graph:
        win = [k for k in eng._graphs if isinstance(k, tuple) and k[0] == "win"]
        assert win, "the iterations were captured"
        # one graph per (column window, probability-buffer parity) -- six distinct scales add none
        assert len(win) <= 2 * len(eng.captured_column_windows()), win


def test_decode_many_list_of_equal_configs_is_the_single_config_path():
    """prompts that share one scale take the scalar launch and the scalar graph keys; per-prompt seeds still hold"""
    j, vocab = 2, 4096
    solo = _solo_references(vocab)[j]
    eng = _engine(vocab, True)
    with _Spy() as spy:
        res = eng.decode_many([[] for _ in range(N_SLOTS)], [_spec(_model(vocab), j) for _ in range(N_SLOTS)], [_grammar(j) for _ in range(N_SLOTS)],
                              [_config(j, vocab) for _ in range(N_SLOTS)])
    assert spy.slots and all(g == P_SCALES[j] for g in spy.slots)
    assert all(seq == solo[0] and st.matched == solo[1] for seq, st in res)


def test_decode_many_refuses_mixed_scales_on_per_slot_k2_over_a_narrow_head():
    vocab = 4096
    eng = _engine(vocab, False)
    eng.slot_launches = False
    n = N_SLOTS
    with pytest.raises(ValueError, match="different guidance scales.*SJD_SLOT_LAUNCHES=0"):
        eng.decode_many([[] for _ in range(n)], [_spec(_model(vocab), j) for j in range(n)], [_grammar(j) for j in range(n)], [_config(j, vocab) for j in range(n)])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 4: LlamaGenSolver.generate
def _solver(seed=7):
    from llamagen.llamagen_solver import LlamaGenSolver, renew_llamagen
    from scheduler.jacobi_iteration_lumina_mgpt import renew_sampler
    model = make_llamagen(TOY_C2I, 17, 0.25, ops.HipWindowAttention(n_split=2), dtype=torch.bfloat16, device=DEV)
    model.enable_fused(ops, gemm="sjd", max_rows=256)
    jac = dict(jacobi_loop_interval_l=1, jacobi_loop_interval_r=NTOK - 16 - 2, max_num_new_tokens=16, guidance_scale=4.0, seed=seed,
               multi_token_init_scheme='random', do_cfg=True, image_top_k=1000, text_top_k=10, prefix_token_sampler_scheme='speculative_jacobi')
    model.__class__ = renew_llamagen(model.__class__)
    model._init_new_params(**jac)
    model.__class__ = renew_sampler(model.__class__)
    model._init_new_params(**jac)
    return model, LlamaGenSolver(model=model, image_top_k=1000, image_top_p=1.0)


def test_solver_generate_cfg_scale_per_prompt():
    labels, scales = [207, 1, 980, 417, 88], [1.5, 3.0, 4.0, 7.5, 2.0]
    model, solver = _solver()
    kw = dict(temperature=1.0, top_k=1000, top_p=1.0, sample_logits=True)
    got = solver.generate(torch.tensor(labels, device=DEV), NTOK, None, cfg_scale=scales, **kw).cpu()
    assert got.shape == (5, NTOK)
    for j, (lab, sc) in enumerate(zip(labels, scales)):
        # the batch path with the SCALAR cfg_scale[j] (today's code: the windows take the sampler's guidance_scale), five slots as above, every
        # slot decoding class `lab`; row j carries seed + j -- prompt j's seed
        model.guidance_scale = sc
        ref = solver.generate(torch.tensor([lab] * 5, device=DEV), NTOK, None, cfg_scale=sc, **kw).cpu()
        assert int(got[j, 0]) == int(ref[j, 0]), f"prompt {j}: first image token"
        assert torch.equal(got[j], ref[j]), f"prompt {j} (cfg_scale {sc})"
    assert len({tuple(r.tolist()) for r in got}) == 5
    with pytest.raises(ValueError, match="cfg_scale has 4 values for 5 prompts"):
        solver.generate(torch.tensor(labels, device=DEV), NTOK, None, cfg_scale=scales[:4], **kw)


def test_solver_generate_sampler_settings_per_prompt():
    """temperature, top_k and top_p per prompt (with the scales): value j governs prompt j's first draw AND its windows.  The reference of
    row j is today's scalar call on a solver whose image_top_k / image_top_p are prompt j's, its window processors built HERE with prompt
    j's temperature in front (the scalar `temperature` reaches the first draw only)."""
    from transformers.generation.logits_process import LogitsProcessorList, TemperatureLogitsWarper
    from llamagen.llamagen_solver import LlamaGenSolver
    from scheduler.logit_processor_3dim import TopKLogitsWarper, TopPLogitsWarper3d
    labels, scales = [207, 1, 980, 417, 88], [1.5, 3.0, 4.0, 7.5, 2.0]
    temps, top_ks, top_ps = [1.0, 0.8, 1.25, 0.9, 1.0], [1000, 300, 2000, 50, 1000], [1.0, 0.95, 0.9, 1.0, 0.85]
    model, solver = _solver()
    got = solver.generate(torch.tensor(labels, device=DEV), NTOK, None, cfg_scale=scales, temperature=temps, top_k=torch.tensor(top_ks),
                          top_p=tuple(top_ps), sample_logits=True).cpu()
    assert got.shape == (5, NTOK) and len({tuple(r.tolist()) for r in got}) == 5
    for j, lab in enumerate(labels):
        ref_solver = LlamaGenSolver(model=model, image_top_k=top_ks[j], image_top_p=top_ps[j])
        ref_solver.create_logits_processor = lambda j=j: LogitsProcessorList(
            ([TemperatureLogitsWarper(temps[j])] if temps[j] != 1.0 else []) + [TopKLogitsWarper(top_k=top_ks[j]), TopPLogitsWarper3d(top_p=top_ps[j])])
        model.guidance_scale = scales[j]
        ref = ref_solver.generate(torch.tensor([lab] * 5, device=DEV), NTOK, None, cfg_scale=scales[j], temperature=temps[j], top_k=top_ks[j],
                                  top_p=top_ps[j], sample_logits=True).cpu()
        assert torch.equal(got[j], ref[j]), f"prompt {j}: T {temps[j]}, top-k {top_ks[j]}, top-p {top_ps[j]}, cfg_scale {scales[j]}"
