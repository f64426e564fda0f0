"""Independent check of the hand-written forward at the PRODUCTION shapes and launch configuration (missing #1).

Every other real-shape test is teacher-forced: the oracle consumes the engine's own logits, so a wrong G1 / K1 / F1r / F2 result at the
Lumina-7B or Emu3-8B launch configuration would pass.  Here the logits themselves are compared, three ways, on the same weights and the
same token windows:

  hip16   what the engine runs: prefill (hipBLASLt + F1/F2/F3 + K1), then window forwards exactly as SJDEngine launches them --
          enable_fused(gemm="sjd"), folded norm, production G1_CFG / G1_CFG_EMU3, K1 auto-split over the device-side kv_len, G1s,
          output head as split-K partials on the grammar's column window read by K2 -- the first windows eager, the later ones as
          hipGraph replays (ONE graph per iteration: K5, forward, K2 with in-kernel noise, K4).  The logits are the ones K2 derived (its `dbg` output).
  aten16  an INDEPENDENT PyTorch-ROCm 16-bit forward written in this file from the reference's call sites (MC:59-73 RMSNorm, MC:198-219
          per-head LayerNorm, MC:144-178 RoPE, MC:499-581 attention with torch.cat KV + additive mask (JL:1256-1336) + SDPA,
          MC:593-668 layer, MC:1560-1561 head) -- hipBLASLt GEMMs, ATen norms / RoPE, nothing from libsjd_hip.so, nothing from
          sjd_amd.backbones' forward code.
  fp32    the same independent forward in fp32 on the 16-bit-rounded weights (cast layer by layer), explicit softmax attention.

Asserted: |hip16 - fp32| <= 1.5 x |aten16 - fp32| (max and mean) on the rows and vocabulary columns K2 reads, and the per-row argmax of
hip16 agrees with aten16's unless the two candidates are closer in fp32 than the 16-bit error itself.  The numbers go to
gpurun_out/r4_real_shape_forward_<family>[_P<prompt length>].json (committed under profiles/).
"""
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rotate_half(x):
    h = x.shape[-1] // 2
    return torch.cat((-x[..., h:], x[..., :h]), dim=-1)


class _IndependentForward:
    """ATen restatement of the reference's Chameleon / Llama decoder over a torch.cat KV cache, in `dt` (16-bit: as the reference runs it;
    fp32: weights cast per layer)."""

    def __init__(self, model, dt):
        self.m, self.dt, self.a = model, dt, model.args
        self.k, self.v = {}, {}

    def _w(self, t):
        return t if t.dtype == self.dt else t.to(self.dt)

    def rollback(self, rows):
        for li in self.k:
            self.k[li], self.v[li] = self.k[li][:, :, :rows], self.v[li][:, :, :rows]

    def _rms(self, x, w, eps):                                   # MC:68-73
        xf = x.to(torch.float32)
        xf = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
        return self._w(w) * xf.to(x.dtype)

    def _attn(self, q, K, V, mask):                              # q [B,H,n,D], K/V [B,H,S,D], mask additive [B,1,n,S]
        if self.dt == torch.float32:
            outs = []
            for r0 in range(0, q.shape[2], 1024):          # (row blocks: a prefill of 8200 rows would hold 2 x 17 GB of scores at once)
                s = q[:, :, r0:r0 + 1024] @ K.transpose(-1, -2) / math.sqrt(q.shape[-1]) + mask[:, :, r0:r0 + 1024]
                outs.append(torch.softmax(s, dim=-1) @ V)
            return torch.cat(outs, dim=2)
        return F.scaled_dot_product_attention(q, K, V, attn_mask=mask)

    @torch.no_grad()
    def forward(self, tokens, kv_len, key_start, pos_offset, cols):
        """tokens [B,n] occupy cache rows [kv_len, kv_len+n); key j visible to row i of batch b iff key_start[b] <= j <= kv_len+i;
        RoPE position = cache row + pos_offset[b] (hidden rows: 1, JL:705-706).  -> fp32 logits [B,n,cols[1]-cols[0]]"""
        m, a, dt = self.m, self.a, self.dt
        B, n = tokens.shape
        dev = tokens.device
        H, Hkv = a.num_attention_heads, a.num_key_value_heads
        D = a.hidden_size // H
        rows = kv_len + torch.arange(n, device=dev)
        pos = rows[None, :] + pos_offset.to(dev)[:, None]
        pos = torch.where(rows[None, :] < key_start.to(dev)[:, None], torch.ones_like(pos), pos)
        inv = 1.0 / (a.rope_theta ** (torch.arange(0, D, 2, dtype=torch.int64, device=dev).float() / D))        # MC:144-178
        fr = pos[:, :, None].float() * inv[None, None, :]
        emb = torch.cat((fr, fr), dim=-1)
        cos, sin = emb.cos().to(dt)[:, None], emb.sin().to(dt)[:, None]                                          # [B,1,n,D]
        j = torch.arange(kv_len + n, device=dev)[None, None, :]
        vis = (j >= key_start.to(dev)[:, None, None]) & (j <= rows[None, :, None])                               # [B,n,S]
        mask = torch.zeros(B, 1, n, kv_len + n, dtype=dt, device=dev).masked_fill(~vis[:, None], torch.finfo(dt).min)
        h = self._w(m.model.embed_tokens.weight)[tokens] if dt != torch.float32 else m.model.embed_tokens.weight[tokens].to(dt)
        for li, layer in enumerate(m.model.layers):
            at, mlp = layer.self_attn, layer.mlp
            x = self._rms(h, layer.input_layernorm.weight, a.rms_norm_eps)
            q = F.linear(x, self._w(at.q_proj.weight)).view(B, n, H, D)
            k = F.linear(x, self._w(at.k_proj.weight)).view(B, n, Hkv, D)
            v = F.linear(x, self._w(at.v_proj.weight)).view(B, n, Hkv, D)
            if a.qk_norm:                                                                                        # MC:198-219
                q = F.layer_norm(q, (D,), None, None, eps=1e-5) * self._w(at.q_norm.weight) + self._w(at.q_norm.bias)
                k = F.layer_norm(k, (D,), None, None, eps=1e-5) * self._w(at.k_norm.weight) + self._w(at.k_norm.bias)
            q, k, v = q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)
            q = q * cos + _rotate_half(q) * sin
            k = k * cos + _rotate_half(k) * sin
            if li in self.k:                                                                                     # DynamicCache.update
                self.k[li], self.v[li] = torch.cat([self.k[li], k], dim=2), torch.cat([self.v[li], v], dim=2)
            else:
                self.k[li], self.v[li] = k, v
            assert self.k[li].shape[2] == kv_len + n
            G = H // Hkv
            K = self.k[li][:, :, None].expand(B, Hkv, G, kv_len + n, D).reshape(B, H, kv_len + n, D)             # repeat_kv (MC:222-232)
            V = self.v[li][:, :, None].expand(B, Hkv, G, kv_len + n, D).reshape(B, H, kv_len + n, D)
            o = self._attn(q.contiguous(), K.contiguous(), V.contiguous(), mask).transpose(1, 2).reshape(B, n, H * D)
            h = h + F.linear(o, self._w(at.o_proj.weight))
            x = self._rms(h, layer.post_attention_layernorm.weight, a.rms_norm_eps)
            h = h + F.linear(F.silu(F.linear(x, self._w(mlp.gate_proj.weight))) * F.linear(x, self._w(mlp.up_proj.weight)),
                             self._w(mlp.down_proj.weight))
        x = self._rms(h, m.model.norm.weight, a.rms_norm_eps)
        return F.linear(x, self._w(m.lm_head.weight[cols[0]:cols[1]])).float()                                    # MC:1560-1561


def _allowed_columns(rules, V):
    """(lo, hi) hull of the ids the non-forced rules allow (the columns K2 reads); rows with a forced token read no logits"""
    lo, hi = V, 0
    for r in rules:
        if r.forced >= 0:
            continue
        if r.n_ranges == 0:
            return 0, V
        lo = min([lo] + [r.lo[i] for i in range(r.n_ranges)])
        hi = max([hi] + [r.hi[i] for i in range(r.n_ranges)])
    return (lo, hi) if hi > lo else (0, V)


# (family, prompt length, cache rows): P = 700 is round 3's case; P = 2300 (Lumina: the end of a 768x768 image) and P = 4100 (Emu3: the middle
# of a 720x720 one, K1 with 16 splits x 8 tiles) put K1 and the late-image G1 / head launch shapes under the same INDEPENDENT check -- until
# round 4 that region was only teacher-forced (VERDICT r3 missing #5, MC:499-581).  P = 8200 (round 5): the END of Emu3's 720x720 image (8190 visual
# tokens, emu3/mllm/modeling_emu3.py:668-744) -- the ring kernel with 16 splits x 16 tiles.  emu3_8b_bf16: the dtype the reference's test_emu3.py:27
# loads Emu3 in; there the window projections run on the 12-bit stream (G1z / 64-row G1sz).
@pytest.mark.parametrize("family,P,s_max", [("lumina7b", 700, 1024), ("emu3_8b", 700, 1024), ("emu3_8b_bf16", 700, 1024),
                                            ("lumina7b", 2300, 2432), ("emu3_8b", 4100, 4224), ("emu3_8b", 8200, 8320)])
@torch.no_grad()
def test_window_forward_at_production_shapes_against_independent_forwards(family, P, s_max):
    import sjd_amd.ops as ops
    import sjd_amd.backbones as BB
    import sjd_amd.synthetic as synthetic
    from sjd_amd.engine import SJDEngine, SJDConfig
    from sjd_amd.frontends import lumina_window_spec, lumina_prompt, emu3_window_spec
    from sjd_amd.grammar import LuminaGrammar, Emu3Grammar
    dev = torch.device("cuda:0")
    seed = 17
    tag_name = family if P == 700 else f"{family}_P{P}"
    if family == "lumina7b":
        margs, dt, window = BB.LUMINA_7B, torch.bfloat16, 16
    else:
        margs, dt, window = BB.EMU3_8B, (torch.bfloat16 if family.endswith("bf16") else torch.float16), 32
        family = "emu3_8b"
    with torch.device(dev):
        model = BB.ChameleonBackbone(margs, attn=ops.HipWindowAttention()).to(dt).eval()
    if family == "emu3_8b":
        model.G1_CFG = dict(model.G1_CFG_EMU3)
    synthetic.fill_state_dict_device(model, seed=0, embed_token_scale=0.7)
    model.enable_fused(ops, gemm="sjd")
    V = margs.vocab_size
    if family == "lumina7b":
        if P == 700:
            prompt = lumina_prompt(P, 48, 48, seed=seed)
            spec = lumina_window_spec(prompt, dev)
        else:
            # late in an image: a 64-token prompt followed by P - 64 image tokens, all handed over as the context, so that BOTH batch rows
            # read a long cache (the uncond row hides only the 63 text tokens, as it does at the end of a real decode)
            from sjd_amd.frontends import WindowSpec
            prompt = lumina_prompt(64, 48, 48, seed=seed) + synthetic.synthetic_prompt(P - 64, seed + 5, lo=4, hi=8196)[0].tolist()
            rows_ = torch.arange(P)
            spec = WindowSpec(first_tokens=torch.tensor([prompt, prompt], dtype=torch.long, device=dev),
                              first_positions=torch.stack([rows_, torch.where(rows_ < 63, torch.ones_like(rows_), rows_ - 63)]).to(dev),
                              key_start=torch.tensor([0, 63], dtype=torch.int32), pos_offset=torch.tensor([0, -63], dtype=torch.long), kv_base=0)
        grammar = LuminaGrammar(2000, 10)
        cfg = SJDConfig(jacobi_loop_interval_l=0, jacobi_loop_interval_r=48 * 48 + 48 - 13, max_num_new_tokens=window, guidance_scale=3.0,
                        seed=seed, max_length=P + 400, eos_token_ids=(8196,))
    else:
        tok = dict(img_token=151851, eoi_token=151853, eos_token=151850, eol_token=151846, eof_token=151847, pad_token=151643)
        pos = synthetic.synthetic_prompt(P - 1, seed, lo=1000, hi=150000)[0].tolist() + [tok["img_token"]]
        neg = synthetic.synthetic_prompt(11, seed + 1, lo=1000, hi=150000)[0].tolist() + [tok["img_token"]]
        spec = emu3_window_spec(pos, neg, tok["pad_token"], dev)
        prompt = spec.first_tokens[0].tolist()
        grammar = Emu3Grammar(90, 90, 151854, 32768, top_k=2048, **tok)
        cfg = SJDConfig(jacobi_loop_interval_l=1, jacobi_loop_interval_r=90 * 90 - 1, max_num_new_tokens=window, guidance_scale=3.0,
                        seed=seed, max_length=P + 400, eos_token_ids=(tok["eos_token"],))
    if dt == torch.bfloat16 and os.environ.get("SJD_G1Z", "1") != "0":          # (SJD_G1Z=0: the uncompressed stream, an A/B aid)
        # every layer matrix streams in the 12-bit form (the synthetic 184640-row output head may be declined: its units of 32 x 2048 weights
        # carry more than 127 out-of-window values -- it is logged and streams uncompressed, bit-identical either way)
        assert model.compress_stats["compressed"] >= model.compress_stats["matrices"] - 1, model.compress_stats
    model.setup_cache(batch=2, s_max=s_max)
    eng = SJDEngine(model, V, dev, max_window=window, use_graph=True)
    assert eng.head_partials, "the production path reads the output head's split-K partials"
    recs = []

    def hook(d):
        n = d["n_rows"]
        lo, hi = _allowed_columns(d["rules"], V)
        live = [i for i, r in enumerate(d["rules"][:n]) if r.forced < 0]
        lc, lu = d["logits_c"], d["logits_u"]
        recs.append(dict(first=d["first"], n=n, kv_len=int(eng.params.view.kv_len), cols=(lo, hi), live=live, use_cfg=d["use_cfg"],
                         graph=(not d["first"]) and eng.logit_columns(d["rules"]) in eng.captured_column_windows(),
                         ids=None if d["first"] else eng.input_ids[:, :n].clone(),
                         pos=None if d["first"] else eng.positions[:, :n].clone(),
                         hip=torch.stack([lc[:, lo:hi], lu[:, lo:hi]]).clone()))

    eng.hook = hook
    eng.decode(prompt, spec, grammar, cfg, warmup_iters=0, timed_iters=8)
    eng.hook = None
    wins = [r for r in recs if not r["first"] and r["n"] > 1]
    assert recs[0]["first"] and len(wins) >= 3 and any(r["graph"] for r in wins) and all(r["use_cfg"] for r in wins)
    # which K1 form these windows ran on: a multi-head window over <= 736 keys takes the column split (k1_dsplit, round 4) -- Lumina at P = 700 --
    # everything else key splits + combine (k1_partial / the ring kernel) in the multi-split regime
    if family == "lumina7b" and P == 700:
        assert model.attn.regime == "colsplit"
    else:
        assert model.attn.regime == "keysplit" and model.attn.n_split >= 4, "a long prompt must put K1 into the multi-split regime"
    assert min(r["kv_len"] for r in wins) >= P
    ks, po = spec.key_start.to(dev), spec.pos_offset.to(dev)
    outs = {}
    for tag, fdt in (("aten16", dt), ("fp32", torch.float32)):
        f = _IndependentForward(model, fdt)
        res = []
        for r in recs:
            if r["first"]:
                lg = f.forward(spec.first_tokens.to(dev), 0, ks, po, r["cols"])[:, -1:]
                # the independent position rule must reproduce what the front end hands the engine
                rows = torch.arange(spec.first_tokens.shape[1], device=dev)
                pos = torch.where(rows[None] < ks[:, None], torch.ones(1, dtype=torch.long, device=dev), rows[None] + po[:, None])
                assert torch.equal(pos, spec.first_positions.to(dev))
            else:
                f.rollback(r["kv_len"])
                assert torch.equal(r["pos"], r["kv_len"] + torch.arange(r["n"], device=dev)[None] + po[:, None])      # K5's position ids
                lg = f.forward(r["ids"], r["kv_len"], ks, po, r["cols"])
            res.append(lg)
        outs[tag] = res
        del f
        torch.cuda.empty_cache()
    rep = dict(family=tag_name, dtype=str(dt), prompt_len=P, window=window, k1_regime=model.attn.regime, n_split=int(model.attn.n_split or 0), iterations=[])
    worst = dict(hip_max=0.0, aten_max=0.0, hip_mean=[], aten_mean=[])
    for i, r in enumerate(recs):
        rows = [0] if r["first"] else r["live"]
        if not rows:
            continue
        hip, a16, f32 = r["hip"][:, rows], outs["aten16"][i][:, rows], outs["fp32"][i][:, rows]
        assert torch.isfinite(hip).all() and hip.shape == a16.shape == f32.shape
        e_hip, e_aten = (hip - f32).abs(), (a16 - f32).abs()
        # argmax per (batch row, window row): agreement, or a tie inside the 16-bit noise (the two candidates' fp32 logits closer than
        # the library path's own worst error)
        ia, ib = hip.argmax(-1), a16.argmax(-1)
        gap = (f32.gather(-1, ib[..., None]) - f32.gather(-1, ia[..., None])).abs()[..., 0]
        agree = (ia == ib)
        ok = agree | (gap <= 2.0 * e_aten.max())
        it = dict(first=r["first"], graph=bool(r["graph"]), rows=len(rows), kv_len=r["kv_len"], cols=list(r["cols"]),
                  logit_std=round(float(f32.std()), 3), hip16_max=round(float(e_hip.max()), 5), hip16_mean=round(float(e_hip.mean()), 6),
                  aten16_max=round(float(e_aten.max()), 5), aten16_mean=round(float(e_aten.mean()), 6),
                  hip_vs_aten_max=round(float((hip - a16).abs().max()), 5), argmax_agree=round(float(agree.float().mean()), 4),
                  argmax_agree_or_tie=round(float(ok.float().mean()), 4))
        rep["iterations"].append(it)
        if not r["first"]:
            worst["hip_max"], worst["aten_max"] = max(worst["hip_max"], it["hip16_max"]), max(worst["aten_max"], it["aten16_max"])
            worst["hip_mean"].append(it["hip16_mean"])
            worst["aten_mean"].append(it["aten16_mean"])
        assert ok.all(), it
        assert e_hip.max() <= 1.5 * e_aten.max() + 1e-3 and e_hip.mean() <= 1.5 * e_aten.mean() + 1e-4, it
    rep["windows"] = dict(hip16_max=worst["hip_max"], aten16_max=worst["aten_max"], hip16_mean=round(sum(worst["hip_mean"]) / len(worst["hip_mean"]), 6),
                          aten16_mean=round(sum(worst["aten_mean"]) / len(worst["aten_mean"]), 6),
                          argmax_agree=round(sum(x["argmax_agree"] * x["rows"] for x in rep["iterations"] if not x["first"]) /
                                             sum(x["rows"] for x in rep["iterations"] if not x["first"]), 4))
    print("real-shape forward:", json.dumps(rep))
    out_dir = os.path.join(ROOT, "gpurun_out")
    if os.path.isdir(out_dir):
        with open(os.path.join(out_dir, f"r5_real_shape_forward_{tag_name}.json"), "w") as fh:
            json.dump(rep, fh, indent=1)
    assert rep["windows"]["argmax_agree"] >= 0.8, rep["windows"]


# ------------------------------------------------------------------------------------------------ several prompts per forward (blob array)
def _logits_from_head_partials(ho):
    """the logits K2 derives from an ops.HeadOut: planes summed in chunk order, the folded final norm as a row scale, the 16-bit rounding
    of the lm_head output (as tests/test_gpu_llamagen_batch.py::_head_logits_from_partials)"""
    p = ho.part
    acc = p.data[0].clone()
    for c in range(1, p.n_chunks):
        acc = acc + p.data[c]
    ss, hid, eps = ho.row_norm
    s = ss[0].clone()
    for i in range(1, ss.shape[0]):
        s = s + ss[i]
    return (acc * torch.rsqrt(s / hid + eps)[:, None]).to(ho.dtype).float()


BLOB_FORWARD_LAYERS = 3          # real widths, three layers: every kernel of the layer runs at its production launch shape; time and memory stay small

# family, compress (the 12-bit weight stream), slots: kv_len / n_rows per slot.  kv_len lies on both sides of HipWindowAttention.COLSPLIT_MAX_KEYS (736);
# a one-row slot is a finished prompt's dummy window, nine rows a ragged one
BLOB_FORWARD_CASES = [
    ("lumina7b", True, [300, 1216, 700, 2300], [16, 1, 9, 16]),
    ("lumina7b", False, [2300, 700, 1216, 300], [16, 9, 1, 16]),
    ("emu3_8b", False, [2000, 300], [32, 9]),
]


@pytest.mark.parametrize("family,compress,kvs,n_rows", BLOB_FORWARD_CASES, ids=["lumina7b_12bit", "lumina7b_raw", "emu3_8b"])
@torch.no_grad()
def test_blob_array_window_forward_against_independent_forwards(family, compress, kvs, n_rows):
    """The Chameleon-family window forward with several prompts per launch -- every slot's kv_len / n_rows from its own sjd_iter_params blob
    (batch_rows = 2), production G1_CFG_128ROW, K1 in the regime and split count the engine would choose -- against this file's
    _IndependentForward (aten16 and fp32) run per slot on its own torch.cat cache.  The SJDBatchEngine tests are teacher-forced: a slot
    that attended over its neighbour's kv_len, or appended its K/V rows at the neighbour's offset, gives self-consistent logits there.
    Here the logits K2 would read (head partials summed) are held, PER SLOT and on the slot's valid rows only, to the bound of the
    single-prompt test: |hip - fp32| <= 1.5 x |aten16 - fp32| (max and mean) and its argmax rule.  A pooled maximum would let one wrong
    slot hide behind another slot's large but honest error.  Lumina-7B width (MHA 32 x 128, QK-norm, bf16, window 16, four slots, 12-bit
    stream and uncompressed) and Emu3-8B width (GQA 32 / 8, fp16, window 32, two slots: the ring kernel)."""
    import dataclasses
    import sjd_amd.ops as ops
    import sjd_amd._lib as L
    import sjd_amd.backbones as BB
    import sjd_amd.synthetic as synthetic
    from sjd_amd.engine_batch import _CacheView
    dev = torch.device("cuda:0")
    if family == "lumina7b":
        margs, dt, W = dataclasses.replace(BB.LUMINA_7B, num_hidden_layers=BLOB_FORWARD_LAYERS), torch.bfloat16, 16
    else:
        margs, dt, W = dataclasses.replace(BB.EMU3_8B, num_hidden_layers=BLOB_FORWARD_LAYERS), torch.float16, 32
    nb, P = 2, len(kvs)
    B, V = nb * P, margs.vocab_size
    with torch.device(dev):
        model = BB.ChameleonBackbone(margs, attn=ops.HipWindowAttention()).to(dt).eval()
    synthetic.fill_state_dict_device(model, seed=0, embed_token_scale=0.7)
    model.G1_CFG = dict(model.G1_CFG_128ROW)
    model.enable_fused(ops, gemm="sjd", compress=compress)
    if compress:
        assert model.compress_stats["compressed"] >= model.compress_stats["matrices"] - 1, model.compress_stats
    else:
        assert model.compress_stats["compressed"] == 0
    s_max = ((max(kvs) + W + 127) // 128) * 128
    model.setup_cache(batch=B, s_max=s_max)
    g = torch.Generator().manual_seed(23)
    u0 = [20 + 7 * j for j in range(P)]                       # the uncond row of slot j hides the first u0[j] context tokens
    ks = torch.tensor([x for j in range(P) for x in (0, u0[j])], dtype=torch.int32, device=dev)
    po = -ks.long()
    ctx = [torch.randint(4, 8196, (1, kv), generator=g).repeat(nb, 1).to(dev) for kv in kvs]
    win = torch.randint(4, 8196, (P, 1, W), generator=g).repeat(1, nb, 1).view(B, W).to(dev)
    # every slot's context through the backbone's prefill path (library GEMMs + F2 + K1 with host kv_len), two batch rows at a time
    model.attn.params = None
    full = model.cache
    for j, kv in enumerate(kvs):
        lo, hi = j * nb, (j + 1) * nb
        rows = torch.arange(kv, device=dev)
        pos = torch.where(rows[None] < ks[lo:hi, None], torch.ones(1, dtype=torch.long, device=dev), rows[None] + po[lo:hi, None])
        model.cache = _CacheView(full, lo, hi)
        model.attn.choose_regime(kv, dt, shape=(nb, kv, model.n_heads, model.n_kv_heads, model.head_dim))
        model.forward_window(ctx[j], pos, 0, ks[lo:hi].contiguous())
    model.cache = full
    # the window forward: every slot's kv_len / n_rows from its blob
    params = ops.BlobArray(L.IterParams, P, dev)
    for j, (kv, n) in enumerate(zip(kvs, n_rows)):
        view = params.blobs[j].view
        view.kv_len, view.n_rows, view.batch_rows = kv, n, nb
    params.upload()
    kv_rows = torch.tensor(kvs, device=dev).repeat_interleave(nb)
    pos = kv_rows[:, None] + torch.arange(W, device=dev)[None] + po[:, None]
    shape = (B, W, model.n_heads, model.n_kv_heads, model.head_dim)
    regime = model.attn.choose_regime(max(kvs) + W, dt, shape=shape)          # as SJDBatchEngine does per iteration
    assert regime == "keysplit", "several prompts per forward are not a shape the column split serves"
    seen, real = [], ops.skinny_gemm
    ops.skinny_gemm = lambda x, *a_, **k_: (seen.append(int(x.shape[0])), real(x, *a_, **k_))[1]
    try:
        model.attn.params = params
        ho = model.forward_window(win, pos, -1, ks, head_partials=True)
    finally:
        ops.skinny_gemm = real
        model.attn.params = None
    torch.cuda.synchronize()
    assert isinstance(ho, ops.HeadOut) and ho.col0 == 0 and ho.urow_off == W
    assert seen and set(seen) == {B * W}, "the projections ran on G1 at the full row count"
    hip = _logits_from_head_partials(ho)[:B * W].view(B, W, -1)[..., :V]
    assert torch.isfinite(hip).all()
    rep = dict(family=family, dtype=str(dt), compress=bool(compress), layers=BLOB_FORWARD_LAYERS, window=W, k1_regime=regime,
               n_split=int(model.attn.n_split or 0), slots=[])
    failures = []
    for j, (kv, n) in enumerate(zip(kvs, n_rows)):
        lo, hi = j * nb, (j + 1) * nb
        ref = {}
        for tag, fdt in (("aten16", dt), ("fp32", torch.float32)):
            f = _IndependentForward(model, fdt)
            f.forward(ctx[j], 0, ks[lo:hi], po[lo:hi], (0, 32))
            ref[tag] = f.forward(win[lo:hi, :n], kv, ks[lo:hi], po[lo:hi], (0, V))
            del f
        h, a16, f32 = hip[lo:hi, :n], ref["aten16"], ref["fp32"]
        e_hip, e_aten = (h - f32).abs(), (a16 - f32).abs()
        ia, ib = h.argmax(-1), a16.argmax(-1)
        gap = (f32.gather(-1, ib[..., None]) - f32.gather(-1, ia[..., None])).abs()[..., 0]
        agree = ia == ib
        ok = agree | (gap <= 2.0 * e_aten.max())
        rec = dict(slot=j, kv_len=kv, n_rows=n, key_start=[0, u0[j]], logit_std=round(float(f32.std()), 3),
                   hip16_max=round(float(e_hip.max()), 5), hip16_mean=round(float(e_hip.mean()), 6),
                   aten16_max=round(float(e_aten.max()), 5), aten16_mean=round(float(e_aten.mean()), 6),
                   hip_over_aten_max=round(float(e_hip.max() / e_aten.max()), 3), hip_over_aten_mean=round(float(e_hip.mean() / e_aten.mean()), 3),
                   argmax_agree=round(float(agree.float().mean()), 4), argmax_agree_or_tie=round(float(ok.float().mean()), 4))
        rep["slots"].append(rec)
        if not (ok.all() and e_hip.max() <= 1.5 * e_aten.max() + 1e-3 and e_hip.mean() <= 1.5 * e_aten.mean() + 1e-4):
            failures.append(rec)
        torch.cuda.empty_cache()
    print("blob-array forward:", json.dumps(rep))
    out_dir = os.environ.get("SJD_TEST_RECORD_DIR", "")          # where a run keeps its records (committed under profiles/)
    if out_dir and os.path.isdir(out_dir):
        with open(os.path.join(out_dir, f"blob_array_forward_{family}{'' if compress or family != 'lumina7b' else '_raw'}.json"), "w") as fh:
            json.dump(rep, fh, indent=1)
    assert not failures, failures
