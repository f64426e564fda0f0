"""Decoded images from the batch engine and the Lumina solver on the GPU.

  * SJDBatchEngine.decode_many(detokenize=): a finished prompt's image is decoded on the engine's side stream while the other slots keep
    decoding.  Five prompts on two slots (every slot is refilled), window 16, CFG, 16 image tokens per prompt (a 4 x 4 latent):
    the ids are those of the run without the callable, every image is the callable applied to the prompt's ids afterwards on the default
    stream, the images come back in prompt order although the prompts end out of order, and a callable that first idles on the side stream
    still reads the ids of ITS prompt (a refilled slot cannot reach them);
  * LlamaGenSolver.generate with several labels and vq_model=;
  * FlexARInferenceSolver.generate_ids(decode=True) with a tiny Chameleon backbone and a tiny ChameleonVQ.
"""
import json
import os

import numpy as np
import pytest
import torch

import sjd_amd.ops as ops
from tests.helpers import make_chameleon, make_llamagen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VOCAB, EOS = 16384, 16383
TOY_C2I = dict(dim=512, n_layer=2, n_head=8, vocab_size=VOCAB, block_size=256, cls_token_num=1, model_type="c2i", num_classes=1000)
N_SLOTS, WINDOW, N_PROMPTS = 2, 16, 5
_toy = {}


def _vq():
    """a LlamaGen decoder at toy width (three levels: 4 pixels per code) whose codebook holds the backbone's whole vocabulary -- every id the
    decode can emit, EOS included, is a valid code -- with synthetic weights, fp32 on the device"""
    if "vq" not in _toy:
        import sjd_amd.synthetic as synthetic
        from sjd_amd.detokenizers import LlamaGenVQ
        vq = LlamaGenVQ(codebook_size=VOCAB, codebook_embed_dim=8, z_channels=32, ch=32, ch_mult=(1, 2, 2)).eval()
        _toy["vq"] = synthetic.fill_state_dict_conv(vq, seed=11).to(DEV)
    return _toy["vq"]


def _model():
    if "model" not in _toy:
        m = make_llamagen(TOY_C2I, 17, 0.25, ops.HipWindowAttention(n_split=2), dtype=torch.bfloat16, device=DEV)
        m.enable_fused(ops, gemm="sjd", max_rows=64)
        m.setup_cache(batch=2 * N_SLOTS, s_max=((1 + 64 + 64 + 31) // 32) * 32)
        _toy["model"] = m
    return _toy["model"]


def _spec(model, j):
    from sjd_amd.engine import WindowSpec
    cond = torch.tensor([(207 + 101 * j) % 1000, model.num_classes], device=DEV)
    return WindowSpec(first_tokens=None, first_positions=None, key_start=torch.zeros(2, dtype=torch.int32), pos_offset=torch.zeros(2, dtype=torch.long),
                      kv_base=1, cond_embeds=model.embed_condition(cond), cond_sampling=dict(cfg_scale=4.0, temperature=1.0, top_k=1000, top_p=1.0))


def _grammar(n_image_tokens=None):
    """LlamaGen's top-k rows; n_image_tokens: every row from that position on is forced to EOS -- the prompt then ends after that many tokens,
    so the prompts of one queue can have latents of different heights"""
    from sjd_amd.grammar import TopKTopPGrammar

    class _EndsAt(TopKTopPGrammar):
        def reset(self):
            self.count = 0

        def _advance(self, t):
            self.count += 1

        def _snapshot(self):
            return self.count

        def _restore(self, s):
            self.count = s

        def window_rules(self, n):
            open_ = ops.make_rule((), -1, self.top_k, self.top_p, temperature=self.temperature)
            forced = ops.make_rule((), EOS, self.top_k, self.top_p, temperature=self.temperature)
            return [open_ if n_image_tokens is None or self.count + j < n_image_tokens else forced for j in range(n)]

        def fast_residual_rules(self, win, rules):          # the rules depend on the NUMBER of tokens only
            return list(rules[:len(win) - 1])

    return _EndsAt(1000, 1.0)


def _config(max_length):
    from sjd_amd.engine import SJDConfig
    # (the windows shrink towards max_length: no prompt emits more; fresh drafts from ids 0..8191: they are never EOS)
    return SJDConfig(jacobi_loop_interval_l=1, jacobi_loop_interval_r=max_length - 2, max_num_new_tokens=WINDOW, guidance_scale=4.0, seed=7,
                     max_length=max_length, img_vocab_lo=0, img_vocab_n=8192, eos_token_ids=(EOS,))


def _engine():
    from sjd_amd.engine_batch import SJDBatchEngine
    eng = SJDBatchEngine(_model(), VOCAB, DEV, N_SLOTS, max_window=WINDOW, use_graph=True)
    assert eng.head_partials
    return eng


def _decode(ids, rows=4):
    """ids of one prompt (1-d, on the device) -> uint8 [4 * rows, 16, 3]: the first rows x 4 codes through the decoder"""
    from sjd_amd.detokenizers import to_uint8
    return to_uint8(_vq().decode_code(ids[:rows * 4], (1, 8, rows, 4)))[0]


def _run(eng, detokenize=None, lengths=None):
    n = N_PROMPTS
    lengths = lengths or [None] * n
    return eng.decode_many([[] for _ in range(n)], [_spec(_model(), j) for j in range(n)], [_grammar(k) for k in lengths],
                           _config(16 if lengths[0] is None else 64), detokenize=detokenize)


def _plain():
    """the queue without a callable: computed once, the reference of the tests below"""
    if "plain" not in _toy:
        res = _run(_engine())
        # (a window sized before the last accept may run past max_length by a few tokens: the image is the first 16)
        assert isinstance(res, list) and all(16 <= len(seq) < 32 and EOS not in seq for seq, _ in res)
        assert len({tuple(seq[:16]) for seq, _ in res}) == N_PROMPTS
        _toy["plain"] = [list(seq) for seq, _ in res]
    return _toy["plain"]


def test_overlapped_detokenize_changes_no_result():
    plain = _plain()
    eng = _engine()
    streams = []

    def detok(ids):
        streams.append(torch.cuda.current_stream().cuda_stream)
        assert ids.is_cuda and ids.dtype == torch.long and ids.dim() == 1
        return _decode(ids)

    main = torch.cuda.current_stream().cuda_stream
    res, images = _run(eng, detok)
    assert [list(seq) for seq, _ in res] == plain, "the ids with detokenize= are those without it"
    assert len(streams) == N_PROMPTS and len(set(streams)) == 1 and streams[0] != main == torch.cuda.current_stream().cuda_stream, \
        "every call ran under ONE side stream"
    assert streams[0] == eng.detok_stream.cuda_stream and all(e is not None and e.query() for e in eng.detok_events)
    for j, img in enumerate(images):
        want = _decode(torch.tensor(plain[j], device=DEV))                 # afterwards, on the default stream
        assert img.shape == (16, 16, 3) and img.dtype == torch.uint8 and img.is_cuda
        diff = int((img.int() - want.int()).abs().max())
        print("prompt", j, "max |pixel difference| side stream vs default stream:", diff)
        assert torch.equal(img, want), f"prompt {j}"
    assert len({img.cpu().numpy().tobytes() for img in images}) == N_PROMPTS
    side = eng.detok_stream
    _run(eng, detok)
    assert eng.detok_stream is side, "the engine keeps its one side stream"


def test_images_come_back_in_prompt_order():
    """prompts 0 and 2 hold 48 image tokens (a 12 x 4 latent), the others 16 (4 x 4): prompt 1 ends before prompt 0"""
    lengths = [48, 16, 48, 16, 16]
    eng = _engine()
    order = []

    def detok(ids):
        n = int(ids.numel())                                # host-side shape: 48 (+ EOS) or 16 (+ EOS) ids
        order.append(n)
        return _decode(ids, rows=12 if n > 48 else 4)

    res, images = _run(eng, detok, lengths)
    seqs = [list(seq) for seq, _ in res]
    for j, (seq, k) in enumerate(zip(seqs, lengths)):
        assert len(seq) >= k + 1 and EOS not in seq[:k] and seq[k] == EOS, f"prompt {j}"
    assert [n > 48 for n in order] != [k > 16 for k in lengths], "the prompts ended in prompt order: the test shows nothing"
    for j, (img, k) in enumerate(zip(images, lengths)):
        assert img.shape == (k, 16, 3), f"prompt {j}: the image of another prompt"
        assert torch.equal(img, _decode(torch.tensor(seqs[j], device=DEV), rows=k // 4)), f"prompt {j}"


def test_refill_cannot_reach_pending_reads():
    """the callable idles on the side stream before it reads its ids: the slot has long been refilled (and has decoded on) by then"""
    plain = _plain()
    eng = _engine()

    def slow(ids):
        torch.cuda._sleep(2_000_000)                        # a plain delay on the side stream
        return _decode(ids)

    res, images = _run(eng, slow)
    assert [list(seq) for seq, _ in res] == plain
    for j, img in enumerate(images):
        assert torch.equal(img, _decode(torch.tensor(plain[j], device=DEV))), f"prompt {j}"


def test_solver_generate_many_labels_with_images():
    from llamagen.llamagen_solver import LlamaGenSolver, renew_llamagen
    from scheduler.jacobi_iteration_lumina_mgpt import renew_sampler
    from sjd_amd.detokenizers import to_uint8
    model = make_llamagen(TOY_C2I, 17, 0.25, ops.HipWindowAttention(n_split=2), dtype=torch.bfloat16, device=DEV)
    model.enable_fused(ops, gemm="sjd", max_rows=64)
    jac = dict(jacobi_loop_interval_l=1, jacobi_loop_interval_r=64 - 16 - 2, max_num_new_tokens=16, guidance_scale=4.0, seed=7,
               multi_token_init_scheme='random', do_cfg=True, image_top_k=1000, text_top_k=10, prefix_token_sampler_scheme='speculative_jacobi')
    model.__class__ = renew_llamagen(model.__class__)
    model._init_new_params(**jac)
    model.__class__ = renew_sampler(model.__class__)
    model._init_new_params(**jac)
    solver = LlamaGenSolver(model=model, image_top_k=1000, image_top_p=1.0, prompts_per_forward=2)
    labels = torch.tensor([207, 1, 980], device=DEV)
    kw = dict(cfg_scale=4.0, temperature=1.0, top_k=1000, top_p=1.0, sample_logits=True)
    plain = solver.generate(labels, 64, None, **kw)                                   # an 8 x 8 latent
    ids, images = solver.generate(labels, 64, None, vq_model=_vq(), **kw)
    assert isinstance(plain, torch.Tensor) and plain.shape == (3, 64) and torch.equal(ids, plain)
    assert images.shape == (3, 32, 32, 3) and images.dtype == torch.uint8 and images.is_cuda
    for j in range(3):
        assert torch.equal(images[j], to_uint8(_vq().decode_code(ids[j], (1, 8, 8, 8)))[0]), f"prompt {j}"


def test_lumina_generate_ids_decode():
    dev = torch.device(DEV)
    import sjd_amd.synthetic as synthetic
    from lumina_mgpt.inference_solver import FlexARInferenceSolver
    from scheduler.jacobi_iteration_lumina_mgpt import renew_pipeline_sampler
    from sjd_amd.detokenizers import ChameleonVQ
    d = np.load(os.path.join(GOLDEN, "decode_images.npz"), allow_pickle=False)
    meta = json.loads(str(d["meta"]))
    vq = synthetic.fill_state_dict_conv(ChameleonVQ(**meta["kwargs"]).eval(), seed=meta["seed"])
    conf = dict(vocab_size=9216, hidden_size=512, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4,
                num_key_value_heads=4, max_position_embeddings=512, rms_norm_eps=1e-5, rope_theta=10000.0)
    hg, wg = 2, 3                                                   # a 4 x 6 latent
    prompt = [9000 + i for i in range(9)] + [8197, 8804 + hg, 8804 + wg]
    n_img = 2 * hg * (2 * wg + 1)
    kw = dict(jacobi_loop_interval_l=0, jacobi_loop_interval_r=n_img - 10, max_num_new_tokens=16, guidance_scale=3.0, seed=11,
              multi_token_init_scheme='random', do_cfg=True, image_top_k=2000, text_top_k=10, prefix_token_sampler_scheme='speculative_jacobi')
    m1 = make_chameleon(conf, 23, 0.25, None, dtype=torch.bfloat16, device=dev)
    solver = FlexARInferenceSolver(model=m1, precision="bf16", device=dev, gemm="torch", vq_model=vq, bpe_to_vq=torch.from_numpy(d["bpe_to_vq"]))
    assert solver.item_processor is None and next(solver.vq_model.parameters()).is_cuda
    solver.eos_token_ids = [8196]
    solver = renew_pipeline_sampler(solver, **kw)
    lp = solver.create_logits_processor(cfg=3.0, image_top_k=2000)
    ids = solver.generate_ids(prompt, max_gen_len=n_img + 1, logits_processor=lp)
    assert len(ids) == n_img + 1 and ids[-1] == 8196
    text, images = solver.generate_ids(prompt, max_gen_len=n_img + 1, logits_processor=lp, decode=True)
    assert text == [] and len(images) == 1
    # the full-size decoder gives 32 pixels per grid (16 per code); the toy decoder's three levels give 4 per code: 8 per grid
    assert images[0].size == (8 * wg, 8 * hg) and images[0].mode == "RGB"
    want = solver.decode_image(prompt[-3:] + ids)
    assert np.array_equal(np.asarray(images[0]), np.asarray(want))
    assert np.asarray(want).std() > 5
