"""GPU: swin-norm Chameleon backbones (the 30B-class form) on the HIP path.

  * the reference's whole SJD loops (tests/golden/loop_lumina_swin.npz) replay bit-exactly through SJDEngine (fp32 backbone, exact-fp32 K1);
  * F1 in its post-norm form and F2 with sharded QK-norm gains against torch restatements, in bf16 and fp16, at 32 / 64 / 256 rows;
    the mode bits leave the plain kernels' bits alone;
  * K1 at a GQA group of 8 (64 / 8 heads) against the fp64 oracle, windows of 16 and 32 rows;
  * G1 / G1z / G1w at the 30B-class projection shapes;
  * two layers at the full 30B-class width: window forwards exactly as SJDEngine launches them (hipGraph replays included) against an
    independent ATen 16-bit forward and an fp32 forward written here, and a teacher-forced loop against the CPU oracle.
"""
import dataclasses
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _make_swin(config, weight_seed, embed_token_scale, attn, dtype, device):
    import sjd_amd.backbones as BB
    import sjd_amd.synthetic as synthetic
    keys = {k: v for k, v in config.items() if k in BB.ChameleonArgs.__dataclass_fields__}
    model = BB.ChameleonBackbone(BB.ChameleonArgs(qk_norm=True, **keys), attn=attn).eval()
    synthetic.fill_state_dict(model, seed=weight_seed, embed_token_scale=embed_token_scale)
    return model.to(device=device, dtype=dtype)


# ------------------------------------------------------------------------------------------------ golden replay
def test_swin_golden_loops_replay_bit_exactly(dev, golden_dir):
    import sjd_amd.ops as ops
    from sjd_amd.engine import SJDEngine, SJDConfig
    from sjd_amd.frontends import lumina_window_spec
    from sjd_amd.grammar import LuminaGrammar
    d = np.load(os.path.join(golden_dir, "loop_lumina_swin.npz"))
    meta = json.loads(str(d["meta"]))
    assert len(meta) == 3
    for m in meta:
        name, jac = m["name"], m["jacobi"]
        model = _make_swin(m["config"], m["weight_seed"], m["embed_token_scale"], ops.HipWindowAttention(n_split=1), torch.float32, dev)
        assert model.args.swin_norm and model.args.model_parallel_size == 2
        prompt = d[f"{name}.prompt"][0].tolist()
        model.setup_cache(batch=2, s_max=((m["max_len"] + 64 + 31) // 32) * 32)
        cfg = SJDConfig(jacobi_loop_interval_l=jac["jacobi_loop_interval_l"], jacobi_loop_interval_r=jac["jacobi_loop_interval_r"],
                        max_num_new_tokens=jac["max_num_new_tokens"], guidance_scale=jac["guidance_scale"], seed=jac["seed"],
                        prefix_token_sampler_scheme=jac["prefix_token_sampler_scheme"], max_length=m["max_len"],
                        eos_token_ids=(8196,), noise_device="cpu", do_sample=m["do_sample"])
        eng = SJDEngine(model, m["config"]["vocab_size"], dev, max_window=jac["max_num_new_tokens"], use_graph=False)
        seq, stats = eng.decode(prompt, lumina_window_spec(prompt, dev), LuminaGrammar(2000, 10), cfg)
        assert seq == d[f"{name}.sequence"][0].tolist(), name
        assert stats.matched == d[f"{name}.matched"].tolist(), name


# ------------------------------------------------------------------------------------------------ F1 post-norm
def _seq_sum(planes, n):
    acc = planes[0].clone()
    for c in range(1, n):
        acc = acc + planes[c]
    return acc


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("rows", [32, 64, 256])
@pytest.mark.parametrize("hidden,n_chunks", [(8192, 13), (8192, 4), (4096, 16)])
def test_f1_post_norm_against_torch(dev, dtype, rows, hidden, n_chunks):
    """h += dtype(w * dtype(rmsnorm(dtype(sum of planes)))) -- the swin order of ChameleonSwinDecoderLayer, from G1 planes and from a dense
    delta; h rounds exactly where the reference's ops round"""
    import sjd_amd.ops as ops
    from sjd_amd.backbones import _CRMSNorm
    g = torch.Generator(device=dev).manual_seed(rows * 7 + hidden + n_chunks)
    h = torch.randn(rows, hidden, generator=g, device=dev).to(dtype)
    planes = torch.zeros(n_chunks, ops._prows(rows), hidden, device=dev)
    planes[:, :rows] = torch.randn(n_chunks, rows, hidden, generator=g, device=dev) * 0.5
    norm = _CRMSNorm(hidden, 1e-5).to(dev).to(dtype)
    norm.weight.data = (1 + 0.1 * torch.randn(hidden, generator=g, device=dev)).to(dtype)
    delta = _seq_sum(planes[:, :rows], n_chunks).to(dtype)                       # the projection output, rounded
    href = h + norm(delta)                                                        # modeling_chameleon.py:717-718
    for src in (ops.Partials(planes, n_chunks, hidden), delta):
        h1 = h.clone()
        out = ops.add_rmsnorm_post(h1, src, norm.weight, 1e-5)
        assert out.data_ptr() == h1.data_ptr()
        torch.testing.assert_close(h1.float(), href.float(), atol=2e-2, rtol=2e-2)
        assert (h1.float() - href.float()).abs().mean() < 2e-3
        if dtype == torch.bfloat16:            # (element mismatches: only where the fp32 sum of squares rounds differently)
            assert (h1 != href).float().mean() < 0.01


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_f1_post_norm_at_16384_columns_and_mode_bits(dev, dtype):
    import ctypes
    import sjd_amd._lib as L
    import sjd_amd.ops as ops
    from sjd_amd.backbones import _CRMSNorm
    g = torch.Generator(device=dev).manual_seed(11)
    rows, hidden, nc = 32, 16384, 3
    h = torch.randn(rows, hidden, generator=g, device=dev).to(dtype)
    planes = torch.randn(nc, 32, hidden, generator=g, device=dev)
    norm = _CRMSNorm(hidden, 1e-5).to(dev).to(dtype)
    h1 = h.clone()
    ops.add_rmsnorm_post(h1, ops.Partials(planes, nc, hidden), norm.weight, 1e-5)
    href = h + norm(_seq_sum(planes, nc).to(dtype))
    torch.testing.assert_close(h1.float(), href.float(), atol=2e-2, rtol=2e-2)
    # mode 0 is the plain kernel: the same bits through the raw entry point with dtype exactly the dtype code
    d = torch.randn(rows, 4096, generator=g, device=dev).to(dtype)
    ha, hb = h[:, :4096].contiguous(), h[:, :4096].contiguous()
    w = norm.weight[:4096].contiguous()
    ya = ops.add_rmsnorm(ha, d, w, 1e-5)
    yb = torch.empty_like(hb)
    lib = L.load()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.sjd_add_rmsnorm(vp(hb), vp(d), vp(w), vp(yb), rows, 4096, ctypes.c_float(1e-5), ops._dtype_code(dtype), None, 0, ops._stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(ha, hb) and torch.equal(ya, yb)
    # an unknown mode bit is refused, post-norm without a sublayer output too
    assert lib.sjd_add_rmsnorm(vp(hb), vp(d), vp(w), vp(yb), rows, 4096, ctypes.c_float(1e-5), ops._dtype_code(dtype) | 0x200, None, 0,
                               ops._stream()) == -2
    assert lib.sjd_add_rmsnorm(vp(hb), None, vp(w), None, rows, 4096, ctypes.c_float(1e-5), ops._dtype_code(dtype) | L.F1_POST_NORM, None, 0,
                               ops._stream()) == -1


# ------------------------------------------------------------------------------------------------ F2 sharded QK-norm
def _f2_inputs(dev, dtype, B, n, H, Hkv, mp, D, n_chunks, seed):
    import sjd_amd.ops as ops
    g = torch.Generator(device=dev).manual_seed(seed)
    T, ncol = B * n, (H + 2 * Hkv) * D
    planes = torch.zeros(n_chunks, ops._prows(T), ncol, device=dev)
    planes[:, :T] = torch.randn(n_chunks, T, ncol, generator=g, device=dev)
    gains = [(1 + 0.3 * torch.randn(mp, D, generator=g, device=dev)).to(dtype) for _ in range(2)]
    biases = [(0.1 * torch.randn(mp, D, generator=g, device=dev)).to(dtype) for _ in range(2)]
    inv = (1.0 / (10000.0 ** (torch.arange(0, D, 2, device=dev).float() / D)))
    pos = (torch.randint(0, 3000, (B, 1), generator=g, device=dev) + torch.arange(n, device=dev)[None]).reshape(-1).contiguous()
    return ops.Partials(planes, n_chunks, ncol), gains, biases, inv, pos


def _f2_run(dev, dtype, part, qn_w, qn_b, kn_w, kn_b, inv, pos, B, n, H, Hkv, D, shards, S=64, kv_len=9):
    import sjd_amd.ops as ops
    kc, vc = torch.zeros(B, Hkv, S, D, dtype=dtype, device=dev), torch.zeros(B, Hkv, S, D, dtype=dtype, device=dev)
    q = ops.qknorm_rope_append(part, kc, vc, qn_w, qn_b, kn_w, kn_b, inv, pos, B, n, H, Hkv, D, None, kv_len, dtype=dtype, qk_shards=shards)
    torch.cuda.synchronize()
    return q, kc, vc


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,n", [(2, 16), (2, 32), (8, 32)])           # 32 / 64 / 256 rows (256 bf16: the four-heads-per-wave kernel)
@pytest.mark.parametrize("H,Hkv,mp", [(64, 8, 4), (8, 4, 2)])
def test_f2_sharded_qk_norm(dev, dtype, B, n, H, Hkv, mp):
    """q / k head h takes gain and bias row h // (heads / mp): bit for bit what the shared-row kernel writes for the heads of shard r when it is
    handed row r, and within the 16-bit tolerance of the ATen restatement (ChameleonLayerNorm with model_parallel_size mp)"""
    from sjd_amd.backbones import _HeadLayerNorm, _rotate_half
    D, kv_len, T = 128, 9, B * n
    part, (qw, kw), (qb, kb), inv, pos = _f2_inputs(dev, dtype, B, n, H, Hkv, mp, D, 3, B * n + H + mp)
    q, kc, vc = _f2_run(dev, dtype, part, qw, qb, kw, kb, inv, pos, B, n, H, Hkv, D, mp)
    hq, hk = H // mp, Hkv // mp
    for r in range(mp):
        q0, kc0, vc0 = _f2_run(dev, dtype, part, qw[r:r + 1].contiguous(), qb[r:r + 1].contiguous(), kw[r:r + 1].contiguous(),
                               kb[r:r + 1].contiguous(), inv, pos, B, n, H, Hkv, D, 1)
        assert torch.equal(q[:, :, r * hq:(r + 1) * hq], q0[:, :, r * hq:(r + 1) * hq]), r
        assert torch.equal(kc[:, r * hk:(r + 1) * hk], kc0[:, r * hk:(r + 1) * hk]), r
        assert torch.equal(vc, vc0)
    # every shard holding the same row: the sharded kernel writes what the plain (mode 0) kernel writes with that row, bit for bit
    same = lambda t: t[:1].expand(mp, -1).contiguous()
    qs, kcs, vcs = _f2_run(dev, dtype, part, same(qw), same(qb), same(kw), same(kb), inv, pos, B, n, H, Hkv, D, mp)
    q1, kc1, vc1 = _f2_run(dev, dtype, part, qw[:1].contiguous(), qb[:1].contiguous(), kw[:1].contiguous(), kb[:1].contiguous(), inv, pos,
                           B, n, H, Hkv, D, 1)
    assert torch.equal(qs, q1) and torch.equal(kcs, kc1) and torch.equal(vcs, vc1)
    # the ATen restatement
    qn, kn = _HeadLayerNorm(D, H, mp).to(dev).to(dtype), _HeadLayerNorm(D, Hkv, mp).to(dev).to(dtype)
    qn.weight.data, qn.bias.data, kn.weight.data, kn.bias.data = qw, qb, kw, kb
    x = _seq_sum(part.data[:, :T], 3).to(dtype).view(B, n, H + 2 * Hkv, D)
    qr, kr = qn(x[:, :, :H]), kn(x[:, :, H:H + Hkv])
    fr = pos.view(B, n)[:, :, None].float() * inv[None, None, :]
    emb = torch.cat((fr, fr), dim=-1)
    cos, sin = emb.cos().to(dtype)[:, :, None, :], emb.sin().to(dtype)[:, :, None, :]
    qr = qr * cos + _rotate_half(qr) * sin
    kr = kr * cos + _rotate_half(kr) * sin
    torch.testing.assert_close(q.float(), qr.float(), atol=4e-2, rtol=4e-2)
    torch.testing.assert_close(kc[:, :, kv_len:kv_len + n].float(), kr.transpose(1, 2).float(), atol=4e-2, rtol=4e-2)
    assert (q.float() - qr.float()).abs().mean() < 4e-3


def test_f2_shards_must_divide_heads(dev):
    import sjd_amd._lib as L
    import sjd_amd.ops as ops
    part, (qw, kw), (qb, kb), inv, pos = _f2_inputs(dev, torch.bfloat16, 2, 16, 12, 4, 3, 128, 2, 1)
    with pytest.raises(L.SjdLibraryError):
        _f2_run(dev, torch.bfloat16, part, qw, qb, kw, kb, inv, pos, 2, 16, 12, 4, 128, 3)      # 3 does not divide H_kv = 4
    assert ops is not None


# ------------------------------------------------------------------------------------------------ K1 at group 8
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n,kv_len", [(16, 200), (32, 200), (16, 1500), (32, 1500)])
def test_k1_gqa_group_8(dev, dtype, n, kv_len):
    """64 q heads over 8 kv heads: a 16-row window runs on the LDS-DMA ring kernel (eight (head, chunk) pairs), a 32-row one on the eight-wave
    k1_partial -- against the fp64 oracle, CFG batch of two with the uncond row's hidden prefix"""
    import sjd_amd.ops as ops
    from oracle.attention_ref import OracleWindowAttention
    B, H, Hkv, D = 2, 64, 8, 128
    S = ((kv_len + n + 63) // 64) * 64
    g = torch.Generator(device=dev).manual_seed(n + kv_len)
    kc = torch.zeros(1, B, Hkv, S, D, dtype=dtype, device=dev)
    vc = torch.zeros_like(kc)
    kc[0, :, :, :kv_len] = torch.randn(B, Hkv, kv_len, D, generator=g, device=dev).to(dtype)
    vc[0, :, :, :kv_len] = torch.randn(B, Hkv, kv_len, D, generator=g, device=dev).to(dtype)
    q = torch.randn(B, n, H, D, generator=g, device=dev).to(dtype)
    k = torch.randn(B, n, Hkv, D, generator=g, device=dev).to(dtype)
    v = torch.randn(B, n, Hkv, D, generator=g, device=dev).to(dtype)
    ks = torch.tensor([0, 37], dtype=torch.int32, device=dev)

    class _C:
        pass
    c1, c2 = _C(), _C()
    c1.k, c1.v, c2.k, c2.v = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    out = ops.HipWindowAttention()(0, q, k, v, c1, kv_len, ks)
    ref = OracleWindowAttention()(0, q, k, v, c2, kv_len, ks.cpu())
    torch.cuda.synchronize()
    assert torch.equal(c1.k, c2.k) and torch.equal(c1.v, c2.v)
    err = (out.float() - ref.float()).abs()
    assert err.max() < 2e-2 and err.mean() < 2e-3, (err.max(), err.mean())


# ------------------------------------------------------------------------------------------------ G1 family at the 30B-class shapes
def _g1_shapes():
    import sjd_amd.backbones as BB
    a = BB.CHAMELEON_30B
    D = a.hidden_size // a.num_attention_heads
    hid, inter = a.hidden_size, a.intermediate_size
    cz, cu = BB.ChameleonBackbone.G1_CFG_30B_Z, BB.ChameleonBackbone.G1_CFG_30B
    return [("qkv", (a.num_attention_heads + 2 * a.num_key_value_heads) * D, hid, cu["qkv"], cz["qkv"]),
            ("o", hid, a.num_attention_heads * D, cu["o"], cz["o"]),
            ("gate_up", 2 * inter, hid, cu["gate_up"], cz["gate_up"]),
            ("down", hid, inter, cu["down"], cz["down"]),
            ("down_tail", hid, inter, (1792, 4, True), (1792, 8, False))]


@pytest.mark.parametrize("case", range(5))
def test_g1_family_at_30b_shapes(dev, case):
    """the production launch shapes of the 30B class: G1 (uncompressed) against an fp32 matmul, G1z (12-bit) bit-identical to G1 at 32 and
    64 rows, G1w at 256 rows against the fp32 matmul; K = 22016 in 1792-chunks ends in a 512-long tail chunk"""
    import sjd_amd.ops as ops
    name, N, K, cu, cz = _g1_shapes()[case]
    g = torch.Generator(device=dev).manual_seed(N + K + case)
    w = (torch.randn(N, K, generator=g, device=dev) / K ** 0.5).to(torch.bfloat16)
    for M, cfg in ((32, cu), (64, cu), (32, cz), (64, cz)):
        assert cfg[0] <= 2560 or M > 32, "a 32-row window stages its K chunk in LDS"
        x = torch.randn(M, K, generator=g, device=dev).to(torch.bfloat16)
        wp = ops.pack_weight(w, cfg[0], cfg[2])
        ref = ops.skinny_gemm(x, wp, N, K, cfg[0], cfg[1], cfg[2]).data
        got = ref.sum(0)[:M]
        torch.testing.assert_close(got, x.float() @ w.float().t(), atol=3e-3, rtol=3e-3)
        wz = ops.pack_weight_z(w, cfg[0], cfg[2])
        assert wz is not None
        zz = ops.skinny_gemm(x, wz, N, K, cfg[0], cfg[1], cfg[2]).data
        torch.cuda.synchronize()
        assert torch.equal(zz.view(torch.int32), ref.view(torch.int32)), (name, M, cfg)
        del wp, wz
    x = torch.randn(256, K, generator=g, device=dev).to(torch.bfloat16)
    kc = 2048 if K <= 8192 else 1408
    wp = ops.pack_weight(w, kc, True)
    got = ops.skinny_gemm(x, wp, N, K, kc, 4, True).data.sum(0)[:256]
    torch.testing.assert_close(got, x.float() @ w.float().t(), atol=3e-3, rtol=3e-3)


def test_g1_output_head_at_30b_shape(dev):
    """the 8192 x 65536 output head as G1 column windows (the image body's 8192 columns, and all of them), G1z bit-identical"""
    import sjd_amd.backbones as BB
    import sjd_amd.ops as ops
    a = BB.CHAMELEON_30B
    N, K = a.vocab_size, a.hidden_size
    KC, waves, sm = BB.ChameleonBackbone.HEAD_CFG
    g = torch.Generator(device=dev).manual_seed(5)
    w = (torch.randn(N, K, generator=g, device=dev) * (3.0 / K ** 0.5)).to(torch.bfloat16)
    x = torch.randn(32, K, generator=g, device=dev).to(torch.bfloat16)
    wp, wz = ops.pack_weight(w, KC, sm), ops.pack_weight_z(w, KC, sm)
    for c0, nc in ((0, 8192), (0, N)):
        ref = ops.skinny_gemm_cols(x, wp, N, K, KC, c0, nc, waves, sm).data
        got = ops.skinny_gemm_cols(x, wz, N, K, KC, c0, nc, waves, sm).data
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
        torch.testing.assert_close(ref.sum(0)[:32], x.float() @ w[c0:c0 + nc].float().t(), atol=5e-3, rtol=5e-3)


# ------------------------------------------------------------------------------------------------ the full 30B-class width
class _IndependentSwinForward:
    """ATen restatement of the reference's ChameleonSwinDecoderLayer stack (MC:670-735) over a torch.cat KV cache, in `dt`; QK-norm gains
    repeat-interleaved from their [mp, D] shards (MC:196-219).  Nothing from libsjd_hip.so or from sjd_amd.backbones' forward code."""

    def __init__(self, model, dt):
        self.m, self.dt, self.a = model, dt, model.args
        self.k, self.v = {}, {}

    def _w(self, t):
        return t if t.dtype == self.dt else t.to(self.dt)

    def rollback(self, rows):
        for li in self.k:
            self.k[li], self.v[li] = self.k[li][:, :, :rows], self.v[li][:, :, :rows]

    def _rms(self, x, w, eps):
        xf = x.to(torch.float32)
        xf = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
        return self._w(w) * xf.to(x.dtype)

    def _qkn(self, x, norm, heads):
        rep = heads // norm.weight.shape[0]
        x = F.layer_norm(x, (x.shape[-1],), None, None, eps=1e-5)
        return x * self._w(norm.weight).repeat_interleave(rep, dim=0) + self._w(norm.bias).repeat_interleave(rep, dim=0)

    @torch.no_grad()
    def forward(self, tokens, kv_len, key_start, pos_offset, cols):
        m, a, dt = self.m, self.a, self.dt
        B, n = tokens.shape
        dev = tokens.device
        H, Hkv = a.num_attention_heads, a.num_key_value_heads
        D = a.hidden_size // H
        rows = kv_len + torch.arange(n, device=dev)
        pos = rows[None, :] + pos_offset.to(dev)[:, None]
        pos = torch.where(rows[None, :] < key_start.to(dev)[:, None], torch.ones_like(pos), pos)
        inv = 1.0 / (a.rope_theta ** (torch.arange(0, D, 2, dtype=torch.int64, device=dev).float() / D))
        fr = pos[:, :, None].float() * inv[None, None, :]
        emb = torch.cat((fr, fr), dim=-1)
        cos, sin = emb.cos().to(dt)[:, None], emb.sin().to(dt)[:, None]
        j = torch.arange(kv_len + n, device=dev)[None, None, :]
        vis = (j >= key_start.to(dev)[:, None, None]) & (j <= rows[None, :, None])
        mask = torch.zeros(B, 1, n, kv_len + n, dtype=dt, device=dev).masked_fill(~vis[:, None], torch.finfo(dt).min)
        h = self._w(m.model.embed_tokens.weight)[tokens]
        for li, layer in enumerate(m.model.layers):
            at, mlp = layer.self_attn, layer.mlp
            q = F.linear(h, self._w(at.q_proj.weight)).view(B, n, H, D)
            k = F.linear(h, self._w(at.k_proj.weight)).view(B, n, Hkv, D)
            v = F.linear(h, self._w(at.v_proj.weight)).view(B, n, Hkv, D)
            q, k = self._qkn(q, at.q_norm, H), self._qkn(k, at.k_norm, Hkv)
            q, k, v = q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)
            q = q * cos + torch.cat((-q[..., D // 2:], q[..., :D // 2]), dim=-1) * sin
            k = k * cos + torch.cat((-k[..., D // 2:], k[..., :D // 2]), dim=-1) * sin
            if li in self.k:
                self.k[li], self.v[li] = torch.cat([self.k[li], k], dim=2), torch.cat([self.v[li], v], dim=2)
            else:
                self.k[li], self.v[li] = k, v
            G = H // Hkv
            K = self.k[li][:, :, None].expand(B, Hkv, G, kv_len + n, D).reshape(B, H, kv_len + n, D)
            V = self.v[li][:, :, None].expand(B, Hkv, G, kv_len + n, D).reshape(B, H, kv_len + n, D)
            if dt == torch.float32:
                s = q @ K.transpose(-1, -2) / math.sqrt(D) + mask
                o = torch.softmax(s, dim=-1) @ V
            else:
                o = F.scaled_dot_product_attention(q.contiguous(), K.contiguous(), V.contiguous(), attn_mask=mask)
            o = o.transpose(1, 2).reshape(B, n, H * D)
            h = h + self._rms(F.linear(o, self._w(at.o_proj.weight)), layer.input_layernorm.weight, a.rms_norm_eps)      # MC:717-718
            act = F.silu(F.linear(h, self._w(mlp.gate_proj.weight))) * F.linear(h, self._w(mlp.up_proj.weight))
            h = h + self._rms(F.linear(act, self._w(mlp.down_proj.weight)), layer.post_attention_layernorm.weight, a.rms_norm_eps)   # MC:721-724
        x = self._rms(h, m.model.norm.weight, a.rms_norm_eps)
        return F.linear(x, self._w(m.lm_head.weight[cols[0]:cols[1]])).float()


def _model_30b(dev, layers, compress=True):
    import sjd_amd.backbones as BB
    import sjd_amd.ops as ops
    import sjd_amd.synthetic as synthetic
    margs = dataclasses.replace(BB.CHAMELEON_30B, num_hidden_layers=layers)
    with torch.device(dev):
        model = BB.ChameleonBackbone(margs, attn=ops.HipWindowAttention()).to(torch.bfloat16).eval()
    synthetic.fill_state_dict_device(model, seed=0, embed_token_scale=0.7)
    model.enable_fused(ops, gemm="sjd", compress=compress)
    assert not model._fold_norm and model.G1_CFG == (model.G1_CFG_30B_Z if compress else model.G1_CFG_30B)
    return model


def _allowed_columns(rules, V):
    lo, hi = V, 0
    for r in rules:
        if r.forced >= 0:
            continue
        if r.n_ranges == 0:
            return 0, V
        lo = min([lo] + [r.lo[i] for i in range(r.n_ranges)])
        hi = max([hi] + [r.hi[i] for i in range(r.n_ranges)])
    return (lo, hi) if hi > lo else (0, V)


@torch.no_grad()
def test_window_forward_at_30b_width_against_independent_forwards(dev):
    """two swin-norm layers at the full 30B-class width (hidden 8192, 64 / 8 heads, four QK-norm shards, intermediate 22016, V 65536) on the
    12-bit stream: prefill, then window forwards as SJDEngine launches them (eager first, hipGraph replays after) -- against an ATen 16-bit and an
    fp32 forward of the same weights: |hip16 - fp32| <= 1.5 x |aten16 - fp32| (max and mean) and the argmax rule"""
    from sjd_amd.engine import SJDEngine, SJDConfig
    from sjd_amd.frontends import lumina_window_spec, lumina_prompt
    from sjd_amd.grammar import LuminaGrammar
    model = _model_30b(dev, 2)
    assert model.compress_stats["compressed"] == model.compress_stats["matrices"], model.compress_stats
    V, window, P, seed = model.vocab_size, 16, 300, 17
    prompt = lumina_prompt(P, 48, 48, seed=seed)
    spec = lumina_window_spec(prompt, dev)
    cfg = SJDConfig(jacobi_loop_interval_l=0, jacobi_loop_interval_r=48 * 48 + 48 - 13, max_num_new_tokens=window, guidance_scale=3.0,
                    seed=seed, max_length=P + 400, eos_token_ids=(8196,))
    model.setup_cache(batch=2, s_max=512)
    eng = SJDEngine(model, V, dev, max_window=window, use_graph=True)
    recs = []

    def hook(d):
        n = d["n_rows"]
        lo, hi = _allowed_columns(d["rules"], V)
        live = [i for i, r in enumerate(d["rules"][:n]) if r.forced < 0]
        recs.append(dict(first=d["first"], n=n, kv_len=int(eng.params.view.kv_len), cols=(lo, hi), live=live,
                         graph=(not d["first"]) and eng.logit_columns(d["rules"]) in eng.captured_column_windows(),
                         ids=None if d["first"] else eng.input_ids[:, :n].clone(),
                         hip=torch.stack([d["logits_c"][:, lo:hi], d["logits_u"][:, lo:hi]]).clone()))

    eng.hook = hook
    eng.decode(prompt, spec, LuminaGrammar(2000, 10), cfg, warmup_iters=0, timed_iters=8)
    eng.hook = None
    wins = [r for r in recs if not r["first"] and r["n"] > 1]
    assert recs[0]["first"] and len(wins) >= 3 and any(r["graph"] for r in wins)
    ks, po = spec.key_start.to(dev), spec.pos_offset.to(dev)
    outs = {}
    for tag, fdt in (("aten16", torch.bfloat16), ("fp32", torch.float32)):
        f = _IndependentSwinForward(model, fdt)
        res = []
        for r in recs:
            if r["first"]:
                res.append(f.forward(spec.first_tokens.to(dev), 0, ks, po, r["cols"])[:, -1:])
            else:
                f.rollback(r["kv_len"])
                res.append(f.forward(r["ids"], r["kv_len"], ks, po, r["cols"]))
        outs[tag] = res
        del f
        torch.cuda.empty_cache()
    rep = dict(family="chameleon30b_2layers", iterations=[])
    for i, r in enumerate(recs):
        rows = [0] if r["first"] else r["live"]
        if not rows:
            continue
        hip, a16, f32 = r["hip"][:, rows], outs["aten16"][i][:, rows], outs["fp32"][i][:, rows]
        assert torch.isfinite(hip).all() and hip.shape == a16.shape == f32.shape
        e_hip, e_aten = (hip - f32).abs(), (a16 - f32).abs()
        ia, ib = hip.argmax(-1), a16.argmax(-1)
        gap = (f32.gather(-1, ib[..., None]) - f32.gather(-1, ia[..., None])).abs()[..., 0]
        ok = (ia == ib) | (gap <= 2.0 * e_aten.max())
        it = dict(first=r["first"], graph=bool(r["graph"]), rows=len(rows), kv_len=r["kv_len"], hip16_max=round(float(e_hip.max()), 5),
                  hip16_mean=round(float(e_hip.mean()), 6), aten16_max=round(float(e_aten.max()), 5), aten16_mean=round(float(e_aten.mean()), 6),
                  argmax_agree=round(float((ia == ib).float().mean()), 4))
        rep["iterations"].append(it)
        assert ok.all(), it
        assert e_hip.max() <= 1.5 * e_aten.max() + 1e-3 and e_hip.mean() <= 1.5 * e_aten.mean() + 1e-4, it
    print("30b-width forward:", json.dumps(rep))
    out_dir = os.environ.get("SJD_TEST_RECORD_DIR")         # (optional: where the record goes, profiles/swin30b_real_width_forward.json)
    if out_dir and os.path.isdir(out_dir):
        with open(os.path.join(out_dir, "swin30b_real_width_forward.json"), "w") as fh:
            json.dump(rep, fh, indent=1)


@torch.no_grad()
def test_teacher_forced_loop_at_30b_width(dev):
    """the engine's decisions at the full 30B-class width (two swin-norm layers, uncompressed stream this time) replayed into the CPU oracle
    loop with the helpers of tests/gpu_loop_check.py: identical tokens, accept lengths and random streams"""
    from oracle import sjd_oracle as O
    from sjd_amd.engine import SJDEngine, SJDConfig
    from sjd_amd.frontends import lumina_window_spec, lumina_prompt
    from sjd_amd.grammar import LuminaGrammar
    from tests.gpu_loop_check import _Recorder, _replay, _loop_cfg
    model = _model_30b(dev, 2, compress=False)
    V, window, seed, grid = model.vocab_size, 16, 11, 48
    prompt = lumina_prompt(120, grid, grid, seed=seed)
    spec = lumina_window_spec(prompt, dev)
    cfg = SJDConfig(jacobi_loop_interval_l=0, jacobi_loop_interval_r=grid * grid + grid - 13, max_num_new_tokens=window, guidance_scale=3.0,
                    seed=seed, max_length=len(prompt) + 60, eos_token_ids=(8196,))
    model.setup_cache(batch=2, s_max=((len(prompt) + 60 + 2 * window + 64 + 31) // 32) * 32)
    eng = SJDEngine(model, V, dev, max_window=window, use_graph=True)
    O.set_threads(8)
    rec = _Recorder()
    eng.hook = rec
    seq, stats = eng.decode(prompt, spec, LuminaGrammar(2000, 10), cfg)
    seq_ref, tr, checks = _replay(rec, prompt, lambda c, n: O.lumina_rules(c, n, 2000, 10), _loop_cfg(cfg), V, no_cfg_fn=O.lumina_force_no_cfg,
                                  device=dev)
    assert seq == seq_ref, "token sequences differ"
    assert stats.matched == tr.matched and stats.nfe == len(tr.matched)
    assert stats.nfe >= 12 and len(seq) - len(prompt) >= 40, (stats.nfe, len(seq) - len(prompt))
    assert checks["noise"] >= 12
