"""Case tables and the fp64 reference of the several-prompt ("blob array") kernel tests.

One launch of the window forward serves P slots x nb batch rows; every slot has its own kv_len / n_rows in its sjd_iter_params blob
(batch_rows = nb), batch row b belongs to blob b // nb.  tests/test_gpu_kernels.py runs K1 / K3 over these tables on the GPU;
tests/test_blob_array_cases.py checks on the CPU that the tables hold the conditions that make them bite and that the reference and the
bound below are consistent before any kernel is involved.  Nothing here touches the GPU or libsjd_hip.so.
"""
import math

import torch

FP8 = torch.float8_e4m3fn


def _case(name, H, Hkv, D, dtypes, nb, kv, rows, window, key_start, forms, fp8_forms=(), fp8_scales=(1.0, 1.0), reverse=False):
    assert len(kv) == len(rows) and len(key_start) == len(kv) * nb
    return dict(name=name, H=H, Hkv=Hkv, D=D, dtypes=tuple(dtypes), nb=nb, kv=list(kv), rows=list(rows), window=window,
                key_start=list(key_start), forms=tuple(forms), fp8_forms=tuple(fp8_forms), fp8_scales=fp8_scales, reverse=reverse)


# forms: an int = key splits (1: k1_partial writes the output itself; the grouped-query shapes: ring kernel + combine), "colsplit" = k1_dsplit,
# ("merged", s) = the one-launch form with s splits.  key_start: one per batch row, slot-major; the second (uncond) row of a CFG pair is
# non-zero, and some hide the first rows of their slot (kv + i < key_start).
BLOB_CASES = [
    # Lumina-like multi-head window: an empty cache in blob 0, a tile edge (31), mid-image, a finished slot's one-row dummy window
    _case("mha_d128_bf16", 4, 4, 128, [torch.bfloat16], 2, [0, 31, 1216, 700], [16, 16, 16, 1], 16,
          [0, 5, 0, 40, 0, 59, 0, 63], [1, 4, 8, "colsplit", ("merged", 4)], fp8_forms=[1, 8, "colsplit"], fp8_scales=(0.5, 2.0), reverse=True),
    # ragged windows; a fifth slot (the issue's four leave 31 of 64 rows valid) keeps more than half of the rows in the comparison
    _case("mha_d128_fp16", 4, 4, 128, [torch.float16], 2, [33, 2368, 95, 640, 1100], [5, 16, 1, 9, 16], 16,
          [0, 36, 0, 63, 0, 17, 0, 59, 0, 7], [1, 8, "colsplit", ("merged", 8)], reverse=True),
    # Emu3-like grouped-query window of 32 rows: 4 q heads x 2 chunks = 8 pairs per workgroup (ring kernel)
    _case("gqa4_window32", 8, 2, 128, [torch.float16, torch.bfloat16], 2, [2000, 7, 333], [32, 20, 1], 32,
          [0, 5, 0, 10, 0, 40], [1, 8, 16], fp8_forms=[1, 8]),
    # 2 q heads x 2 chunks = 4 pairs; one batch row per slot
    _case("gqa2_window32", 4, 2, 128, [torch.bfloat16], 1, [300, 0, 4101], [32, 17, 32], 32, [11, 5, 4089], [1, 8]),
    # LlamaGen head size, eight slots
    _case("mha_d64_8slots", 12, 12, 64, [torch.bfloat16], 2, [1000, 300, 777, 121, 512, 936, 248, 640], [16, 16, 16, 16, 16, 1, 16, 16], 16,
          [0, 5, 0, 17, 0, 9, 0, 123, 0, 1, 0, 30, 0, 3, 0, 12], [1, 2]),
]


def ordered(case, reverse):
    """the case with its slots in table order or reversed (blob 0 takes another code path than the later blobs)"""
    if not reverse:
        return case
    nb, P = case["nb"], len(case["kv"])
    ks = [case["key_start"][j * nb:(j + 1) * nb] for j in range(P)][::-1]
    return dict(case, name=case["name"] + "_reversed", kv=case["kv"][::-1], rows=case["rows"][::-1], key_start=[x for pair in ks for x in pair])


def s_max_of(case):
    return ((max(case["kv"]) + case["window"] + 127) // 128) * 128


def hidden_rows(case):
    """bool [B, window]: rows that see no key (kv + i < key_start)"""
    nb, W = case["nb"], case["window"]
    kv = torch.tensor(case["kv"]).repeat_interleave(nb)
    return kv[:, None] + torch.arange(W)[None] < torch.tensor(case["key_start"])[:, None]


def padding_rows(case):
    """bool [B, window]: rows >= the slot's n_rows"""
    nb, W = case["nb"], case["window"]
    return torch.arange(W)[None] >= torch.tensor(case["rows"]).repeat_interleave(nb)[:, None]


def make_inputs(case, dtype, seed=0):
    """-> q [B, W, H, D], k / v [B, W, Hkv, D] (rows past a slot's n_rows NaN: a shape-static window may append anything there), caches
    [1, B, Hkv, S, D] with a different content in every batch row.  All on the CPU, in `dtype`."""
    nb, W, H, Hkv, D = case["nb"], case["window"], case["H"], case["Hkv"], case["D"]
    B, S = nb * len(case["kv"]), s_max_of(case)
    g = torch.Generator().manual_seed(1000 + seed + len(case["name"]))
    kc = torch.randn(1, B, Hkv, S, D, generator=g).to(dtype)
    vc = torch.randn(1, B, Hkv, S, D, generator=g).to(dtype)
    q = (torch.randn(B, W, H, D, generator=g) * 1.5).to(dtype)
    k = torch.randn(B, W, Hkv, D, generator=g).to(dtype)
    v = torch.randn(B, W, Hkv, D, generator=g).to(dtype)
    pad = padding_rows(case)
    k[pad], v[pad] = float("nan"), float("nan")
    return q, k, v, kc, vc


def unit_roundoff(dtype):
    return 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11


def attention_fp64(q, kc, vc, kv_len, n_rows, key_start, dtype=None):
    """fp64 draft-window attention of ONE slot over 16-bit operands, vectorised, and the element-wise rounding bound of K1.

    q [nb, n, H, D]; kc / vc [nb, Hkv, S, D] holding the window's rows at [kv_len, kv_len + n_rows); key_start [nb] ints.
    Key j is visible to row i of batch row b iff key_start[b] <= j <= kv_len + i.
    -> exact [nb, n_rows, H, D] fp64 (zero where no key is visible), bound (same shape), visible [nb, n_rows] bool.

    The bound restates the kernel's rounding points: scores and the softmax sum are fp32, each probability is rounded ONCE to the 16-bit
    MFMA operand type before P.V (relative error <= u = 2^-8 bf16 / 2^-11 fp16), the output is rounded once more, so element by element
        |out - exact| <= u * 1.05 * (sum_j p_j |v_jd| + |exact_d|) + 2e-6     (+ fp16: N * 2^-25 max|v| for subnormal probabilities)
    -- about two output ulps.  Measured on Gaussian operands (tests/test_attention_probe_cases.py): a dropped 32-key tile puts about two thirds
    of the output elements beyond it, ONE wrong key at the causal edge 2-4 % of them; tests/test_gpu_attention_probes.py holds K1 to exact answers."""
    dtype = dtype or q.dtype
    nb, _, H, D = q.shape
    Hkv = kc.shape[1]
    G, n, total = H // Hkv, int(n_rows), int(kv_len) + int(n_rows)
    K = kc[:, :, :total].double().repeat_interleave(G, dim=1)           # [nb, H, total, D]
    V = vc[:, :, :total].double().repeat_interleave(G, dim=1)
    Q = q[:, :n].double().transpose(1, 2)                                # [nb, H, n, D]
    S = Q @ K.transpose(-1, -2) / math.sqrt(D)
    j = torch.arange(total)[None, None, None, :]
    i = torch.arange(n)[None, None, :, None]
    ks = torch.as_tensor(key_start).view(nb, 1, 1, 1)
    vis = (j >= ks) & (j <= int(kv_len) + i)                            # [nb, 1, n, total]
    any_vis = vis.any(-1)[:, 0]                                          # [nb, n]
    S = S.masked_fill(~vis, float("-inf"))
    m = S.max(dim=-1, keepdim=True).values
    E = torch.exp(S - torch.where(torch.isinf(m), torch.zeros_like(m), m))
    den = E.sum(-1, keepdim=True)
    P = torch.where(den > 0, E / den.clamp_min(1e-300), torch.zeros_like(E))
    exact = (P @ V).transpose(1, 2)                                      # [nb, n, H, D]
    bound = unit_roundoff(dtype) * 1.05 * ((P @ V.abs()).transpose(1, 2) + exact.abs()) + 2e-6
    if dtype == torch.float16:
        # per (batch row, row, head): visible keys x the largest |v| among them
        vmax = V.abs().amax(-1).masked_fill(torch.arange(total)[None, None, :] < ks[:, :, 0], 0.0)      # [nb, H, total]
        run = torch.cummax(vmax, dim=-1).values
        last = (int(kv_len) + torch.arange(n)).clamp(max=total - 1)
        count = vis.sum(-1)[:, 0].double()                               # [nb, n]
        bound = bound + (count[:, :, None] * 2.0 ** -25 * run[:, :, last].transpose(1, 2))[..., None]
    return exact, bound, any_vis


def _hilo(x):
    """K1-fp8's on-chip operand pair: hi = fp8(x), lo = fp8(16 (x - hi)); value hi + lo / 16"""
    x = x.float()
    hi = x.to(FP8).float()
    return (hi + ((x - hi) * 16.0).to(FP8).float() / 16.0).double()


def attention_fp8_refs(q, kd, vd, kv_len, n_rows, key_start):
    """The two references of test_k1_k3_fp8_kv_cache for ONE slot, vectorised.  q [nb, n, H, D] 16-bit; kd / vd [nb, Hkv, S, D] the
    DEQUANTISED cache (fp8 value x scale).  -> emu (the kernel's arithmetic restated: hi / lo q, P = hi / lo of 256 e, l from the
    unrounded e), want (exact attention over the same cache), conc = sqrt(sum p^2) [nb, n, H], visible [nb, n]."""
    nb, _, H, D = q.shape
    G, n, total = H // kd.shape[1], int(n_rows), int(kv_len) + int(n_rows)
    K = kd[:, :, :total].double().repeat_interleave(G, dim=1)
    V = vd[:, :, :total].double().repeat_interleave(G, dim=1)
    j = torch.arange(total)[None, None, None, :]
    i = torch.arange(n)[None, None, :, None]
    vis = (j >= torch.as_tensor(key_start).view(nb, 1, 1, 1)) & (j <= int(kv_len) + i)
    any_vis = vis.any(-1)[:, 0]

    def probs(Q):
        S = (Q @ K.transpose(-1, -2) / math.sqrt(D)).masked_fill(~vis, float("-inf"))
        m = S.max(dim=-1, keepdim=True).values
        return torch.exp(S - torch.where(torch.isinf(m), torch.zeros_like(m), m))
    e8 = probs(_hilo(q[:, :n]).transpose(1, 2))
    emu = ((_hilo(e8 * 256) / 256) @ V / e8.sum(-1, keepdim=True).clamp_min(1e-300)).transpose(1, 2).float()
    e = probs(q[:, :n].double().transpose(1, 2))
    p = e / e.sum(-1, keepdim=True).clamp_min(1e-300)
    want = (p @ V).transpose(1, 2).float()
    p8 = e8 / e8.sum(-1, keepdim=True).clamp_min(1e-300)
    return emu, want, p8.pow(2).sum(-1).sqrt().transpose(1, 2), any_vis         # conc [nb, n, H]


# ---- F2 (QK-norm + RoPE + KV append) under a blob array: tests/test_gpu_glue.py
F2_SLOT_KV = [21, 0, 300, 63, 64, 1000, 5, 511]

# name, nb, n, slots, H, Hkv, n_chunks (0: a dense qkv source), qk_norm, folded row_norm, QK-norm shards, fp8 cache, dtypes, rows ("0": ops one_head=True, "1": the four-heads-per-wave kernel)
F2_BLOB_CASES = [
    ("qknorm_partials_64rows", 2, 16, 2, 8, 8, 3, True, False, 1, False, ("bf16", "fp16"), (None,)),
    ("plain_folded_64rows", 2, 16, 2, 8, 2, 4, False, True, 1, False, ("bf16", "fp16"), (None,)),
    ("qknorm_folded_fp8_64rows", 2, 16, 2, 8, 8, 2, True, True, 1, True, ("bf16", "fp16"), (None,)),
    ("shards4_32rows", 1, 16, 2, 8, 4, 5, True, False, 4, False, ("bf16",), (None,)),
    ("dense_64rows", 2, 16, 2, 8, 2, 0, True, False, 1, False, ("bf16", "fp16"), (None,)),
    ("dense_fp8_48rows", 1, 16, 3, 4, 4, 0, False, False, 1, True, ("fp16",), (None,)),
    ("planes_128rows", 2, 16, 4, 32, 32, 2, True, True, 1, False, ("bf16", "fp16"), ("0", "1")),
    ("planes_256rows", 2, 16, 8, 32, 8, 4, True, True, 1, False, ("bf16",), ("0", "1")),
    ("planes_256rows_fp8_shards2", 2, 16, 8, 8, 4, 4, True, False, 2, True, ("bf16",), ("0", "1")),
    ("planes_128rows_plain_fp8", 2, 16, 4, 8, 8, 9, False, True, 1, True, ("bf16",), ("0", "1")),
]
