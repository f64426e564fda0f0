"""torch-tensor wrappers over the C-ABI (include/sjd_hip.h).  Plumbing only: device pointers, strides, stream."""
import ctypes
import os

import torch

from . import _lib as L
from . import launch_shapes as LS

gateup_silu_ok = LS.gateup_silu_ok          # the shapes kernels G1s / G1sz / G1sq serve
gateup_silu_chunked_ok = LS.gateup_silu_chunked_ok          # ... and the K = 8192 form of G1sq4 over a copy packed in four chunks


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _dtype_code(dt):
    if dt == torch.bfloat16:
        return L.DTYPE_BF16
    if dt == torch.float16:
        return L.DTYPE_F16
    if dt == torch.float32:
        return L.DTYPE_F32        # K1/K3 only (exact-fp32 parity variant)
    raise L.SjdLibraryError(f"SJD HIP kernels support bf16/fp16 KV and activations, got {dt}")


_PHILOX_BLOCKS = {}


def philox_max_blocks(device):
    """grid cap of ATen's distribution kernels on this device (sjd_iter_params.philox_blocks): multiProcessorCount *
    (maxThreadsPerMultiProcessor / 256) -- calc_execution_policy in ATen/native/cuda/DistributionTemplates.h"""
    device = torch.device(device)
    mb = _PHILOX_BLOCKS.get(device)
    if mb is None:
        p = torch.cuda.get_device_properties(device)
        mb = _PHILOX_BLOCKS[device] = int(p.multi_processor_count) * (int(p.max_threads_per_multi_processor) // 256)
    return mb


def philox_step(numel, max_blocks):
    """what a device generator's offset advances by when ATen fills `numel` elements (== sjd_philox_offset_increment)"""
    if numel <= 0:
        return 0
    T = min((numel + 255) // 256, max_blocks) * 256
    return ((numel - 1) // (T * 4) + 1) * 4


def philox_fill(numel, seed, offset, device, kind=1):
    """-> fp32 [numel]: what K2 / K4 generate in place, written out -- the tensor torch would fill from a device generator at (seed, offset);
    kind 1: exponential_(1), 0: uniform_(0, 1).  sjd_philox_fill (tests/test_gpu_philox.py holds it to torch bit for bit); observers and tests only."""
    out = torch.empty(int(numel), dtype=torch.float32, device=device)
    L.check(L.load().sjd_philox_fill(out.data_ptr(), int(numel), int(seed), int(offset), philox_max_blocks(device), int(kind), _stream()), "sjd_philox_fill")
    return out


_RULE_CACHE = {}


def make_rule(ranges=(), forced=-1, top_k=0, top_p=None, temperature=1.0):
    """-> sjd_row_rule.  A decode asks for the same handful of rules thirty times per iteration, so the structs are interned
    (treat them as read-only; assigning one into a params blob copies it)."""
    key = (tuple((int(lo), int(hi)) for lo, hi in ranges), int(forced), int(top_k or 0), None if top_p is None else float(top_p),
           float(temperature or 1.0))
    r = _RULE_CACHE.get(key)
    if r is not None:
        return r
    rg = key[0]
    if len(rg) > L.MAX_RANGES:
        raise ValueError(f"grammar needs {len(rg)} allowed ranges, kernel supports {L.MAX_RANGES}")
    r = L.RowRule()
    r.n_ranges = len(rg)
    for i, (lo, hi) in enumerate(rg):
        r.lo[i], r.hi[i] = lo, hi
    r.forced, r.top_k = key[1], key[2]
    import numpy as np
    r.top_p_thr = -1.0 if (top_p is None or top_p >= 1.0) else float(np.float32(1.0 - float(top_p)))
    r.temperature = key[4]
    if len(_RULE_CACHE) < 4096:
        _RULE_CACHE[key] = r
    return r


class DeviceBlob:
    """A ctypes struct mirrored in pinned host memory and in a device buffer (one async H2D per upload)."""

    def __init__(self, ctype, device, host=None, dev=None):
        """host / dev: optional pre-allocated uint8 slices (one element of a contiguous array of blobs, see BlobArray)."""
        self.ctype = ctype
        self.nbytes = ctypes.sizeof(ctype)
        self.host = host if host is not None else torch.zeros(self.nbytes, dtype=torch.uint8, pin_memory=True)
        self.dev = dev if dev is not None else torch.zeros(self.nbytes, dtype=torch.uint8, device=device)
        assert self.host.numel() == self.nbytes and self.dev.numel() == self.nbytes
        self.view = ctype.from_address(self.host.data_ptr())
        self._mirror = None

    def upload(self, nbytes=None):
        """pinned host -> device on the current stream (hipMemcpyAsync through the C-ABI: a torch copy_ costs the host 6-8 us per call);
        nbytes: only the leading bytes of the blob (the rest is uploaded by someone else, see SJDEngine._upload_resid)"""
        L.check(L.load().sjd_upload_async(self.dev.data_ptr(), self.host.data_ptr(), self.nbytes if nbytes is None else int(nbytes), _stream()),
                "sjd_upload_async")

    def download(self):
        self.host.copy_(self.dev)
        return self.view

    # ---- read-back without a copy: the kernel that ends the iteration (sjd_verify_accept_ex) writes this blob into a pinned HOST mirror
    # itself and publishes params->iter_seq in the 8 bytes behind it
    @property
    def mirror_ptr(self):
        if self._mirror is None:
            self._mirror = torch.zeros(self.nbytes + 8, dtype=torch.uint8, pin_memory=True)
        return ctypes.c_void_p(self._mirror.data_ptr())

    def collect_mirror(self):
        ctypes.memmove(self.host.data_ptr(), self._mirror.data_ptr(), self.nbytes)
        return self.view

    def wait_mirror(self, seq=None, timeout_s=300.0):
        """seq: the iter_seq the iteration's params carried -> the host spins on the mirror's sequence word (sjd_host_wait_u64: no HIP
        call, the GIL is released) and has the result a microsecond after K4 wrote it; None -> a stream synchronize."""
        assert self._mirror is not None, "no kernel was given this blob's mirror (verify_accept(..., mirror=True))"
        if seq is None:
            L.check(L.load().sjd_stream_synchronize(_stream()), "sjd_stream_synchronize")
        else:
            L.check(L.load().sjd_host_wait_u64(self._mirror.data_ptr() + self.nbytes, int(seq) & 0xFFFFFFFF, int(timeout_s * 1e6)),
                    "sjd_host_wait_u64 (the iteration's last kernel did not report within the timeout)")
        return self.collect_mirror()

    def field_ptr(self, name):
        return ctypes.c_void_p(self.dev.data_ptr() + getattr(self.ctype, name).offset)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.dev.data_ptr())


class BlobArray:
    """n blobs of one ctypes struct, contiguous on the host (pinned) and on the device: the kernels that take per-prompt control
    data index the device array (sjd_iter_params.batch_rows), the host uploads / downloads all of it with one copy."""

    def __init__(self, ctype, n, device):
        nb = ctypes.sizeof(ctype)
        self.host = torch.zeros(n * nb, dtype=torch.uint8, pin_memory=True)
        self.dev = torch.zeros(n * nb, dtype=torch.uint8, device=device)
        self.blobs = [DeviceBlob(ctype, device, self.host[i * nb:(i + 1) * nb], self.dev[i * nb:(i + 1) * nb]) for i in range(n)]

        self.nbytes, self._mirrors = nb, None

    def mirror_array(self):
        """the blobs' pinned host mirrors as ONE allocation at a fixed stride (nbytes + 8: blob, then its sequence word) -> (pointer of blob 0's
        mirror, stride in bytes): what sjd_verify_accept_slots writes for every slot of a continuous batch"""
        if self._mirrors is None:
            st = self.nbytes + 8
            self._mirrors = torch.zeros(len(self.blobs) * st, dtype=torch.uint8, pin_memory=True)
            for i, b in enumerate(self.blobs):
                b._mirror = self._mirrors[i * st:(i + 1) * st]
        return ctypes.c_void_p(self._mirrors.data_ptr()), self.nbytes + 8

    def upload(self):
        L.check(L.load().sjd_upload_async(self.dev.data_ptr(), self.host.data_ptr(), self.host.numel(), _stream()), "sjd_upload_async")

    def download(self):
        self.host.copy_(self.dev)

    def wait_mirror(self):
        """every blob's last writer (sjd_verify_accept_ex with host_mirror) wrote the blob's pinned host mirror itself: one stream wait"""
        L.check(L.load().sjd_stream_synchronize(_stream()), "sjd_stream_synchronize")
        for b in self.blobs:
            if b._mirror is not None:
                b.collect_mirror()

    @property
    def ptr(self):
        return ctypes.c_void_p(self.dev.data_ptr())


def reguess(params: DeviceBlob, state: DeviceBlob, input_ids_out: torch.Tensor, pos_offset=None, positions_out=None):
    """K5: window ids; with positions_out ([n_batch, max_rows] int64) also the window's position ids kv_len + i + pos_offset[b]"""
    n_batch, max_rows = input_ids_out.shape
    assert input_ids_out.dtype == torch.int64 and input_ids_out.is_contiguous()
    if positions_out is None:
        L.check(L.load().sjd_reguess(params.ptr, state.ptr, _ptr(input_ids_out), n_batch, max_rows, _stream()), "sjd_reguess")
        return
    assert positions_out.dtype == torch.int64 and positions_out.is_contiguous() and tuple(positions_out.shape) == (n_batch, max_rows)
    assert pos_offset is None or (pos_offset.dtype == torch.int64 and pos_offset.is_contiguous() and pos_offset.numel() == n_batch)
    L.check(L.load().sjd_reguess_ex(params.ptr, state.ptr, _ptr(input_ids_out), n_batch, max_rows, _ptr(pos_offset) if pos_offset is not None else None,
                                   _ptr(positions_out), _stream()), "sjd_reguess_ex")


def logits_to_probs_sample(logits_c, logits_u, guidance, params: DeviceBlob, noise, probs_out, tokens_out_ptr, col0=0, amax_out_ptr=None):
    """logits_c/u: [rows, V] fp32 views with a common row stride (last dim contiguous) -- or, with col0 > 0, compact views holding
    only the vocabulary columns [col0, col0 + width): every rule in `params` must then keep its allowed ranges inside that window
    (K2 reads no other column; the pointers handed over are those of the virtual column 0)."""
    max_rows, V = probs_out.shape
    assert logits_c.dtype == torch.float32 and logits_c.stride(-1) == 1 and probs_out.is_contiguous()
    assert noise is None or (noise.dtype == torch.float32 and noise.is_contiguous() and noise.shape[-1] == V)      # None: params->philox_blocks > 0
    if logits_u is not None:
        assert logits_u.stride(-2) == logits_c.stride(-2) and logits_u.stride(-1) == 1
    shift = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr() - 4 * int(col0))
    L.check(L.load().sjd_logits_to_probs_sample_ex(shift(logits_c), shift(logits_u), logits_c.stride(-2), float(guidance),
                                                  max_rows, V, params.ptr, _ptr(noise), _ptr(probs_out), tokens_out_ptr, amax_out_ptr,
                                                  _stream()), "sjd_logits_to_probs_sample")


def verify_accept(params: DeviceBlob, state: DeviceBlob, probs, prev_probs, rs, noise2, scratch, mirror=False):
    """mirror: K4 also writes the state into the blob's pinned host copy (read it with state.wait_mirror(), not download())"""
    max_rows, V = probs.shape
    for t in (probs, prev_probs, rs, noise2, scratch):          # rs / noise2 None: the kernel generates them (params->philox_blocks > 0)
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous())
    L.check(L.load().sjd_verify_accept_ex(params.ptr, state.ptr, _ptr(probs), _ptr(prev_probs), _ptr(rs), _ptr(noise2),
                                         _ptr(scratch), max_rows, V, state.mirror_ptr if mirror else None, _stream()), "sjd_verify_accept")


def kv_append(k_new, v_new, k_cache, v_cache, params, kv_len):
    """k_new/v_new [B,n,Hkv,D]; k_cache/v_cache [B,Hkv,S,D] (one layer)."""
    B, n, Hkv, D = k_new.shape
    assert k_new.is_contiguous() and v_new.is_contiguous() and k_cache.is_contiguous() and v_cache.is_contiguous()
    L.check(L.load().sjd_kv_append(_ptr(k_new), _ptr(v_new), _ptr(k_cache), _ptr(v_cache), B, n, Hkv, D,
                                  k_cache.shape[2], _dtype_code(k_new.dtype), params.ptr if params is not None else None,
                                  int(kv_len), _stream()), "sjd_kv_append")


FP8 = torch.float8_e4m3fn      # OCP e4m3: the fp8 KV-cache element type (BASELINE config 5)


def kv_append_fp8(k_new, v_new, k_cache, v_cache, k_scale, v_scale, params, kv_len, head_major=False):
    """k_new/v_new bf16/fp16 [B,n,Hkv,D] (or [B,Hkv,n,D] with head_major) -> fp8(x / scale) rows [kv_len, kv_len+n) of the
    fp8 caches [B,Hkv,S,D]."""
    if head_major:
        B, Hkv, n, D = k_new.shape
    else:
        B, n, Hkv, D = k_new.shape
    assert k_cache.dtype == FP8 and v_cache.dtype == FP8 and k_new.is_contiguous() and v_new.is_contiguous()
    assert k_cache.is_contiguous() and v_cache.is_contiguous()
    L.check(L.load().sjd_kv_append_fp8(_ptr(k_new), _ptr(v_new), _ptr(k_cache), _ptr(v_cache), B, n, Hkv, D, k_cache.shape[2],
                                      _dtype_code(k_new.dtype), float(k_scale), float(v_scale), int(head_major),
                                      params.ptr if params is not None else None, int(kv_len), _stream()), "sjd_kv_append_fp8")


# round 3 experiment (VERDICT r2 next #2a), correct, tested, OFF by default: K1 in ONE launch -- the key splits merged by the last of their
# workgroups to finish instead of by k1_combine.  Same output bits.  Measured per layer (partial + merge, hipGraph): 5.7 / 10.5 / 14.1 /
# 20.4 us at kv 64 / 448 / 1216 / 2368 against 8.6 / 10.7 / 14.4 / 21.0 for the two kernels, but end to end 3.431 against 3.416 ms/step
# at the mean KV length (3.24 against 3.31 at kv 64, where one split is in effect and the output is written directly): the chain store
# acknowledgement -> ticket -> partial loads is three device-scope round trips, a graph-node boundary plus one.  SJD_K1_MERGED=1 selects it.
K1_MERGED_DEFAULT = __import__("os").environ.get("SJD_K1_MERGED", "0") == "1"
_K1_TICKETS = {}


def k1_tickets(B, Hkv, n_rows, device):
    """merge tickets of the one-launch K1 (sjd_draft_window_attention_merged): one zeroed uint32 per (batch, kv head, 16-row chunk); they
    re-arm themselves, so one buffer per device serves every launch of a stream (launches of one stream never overlap)"""
    need = B * Hkv * ((n_rows + 15) // 16)
    device = torch.device(device)
    t = _K1_TICKETS.get(device)
    if t is None or t.numel() < need:
        t = _K1_TICKETS[device] = torch.zeros(max(need, 4096), dtype=torch.int32, device=device)
    return t


def draft_window_attention_fp8(q, k_cache, v_cache, out, k_scale, v_scale, key_start, params, kv_len, n_split, workspace, merged=None):
    """K1 over fp8 caches [B,Hkv,S,D] (value = fp8 * scale); q/out bf16/fp16 [B,n,H,D].  merged: one launch (the key splits are merged by
    their last workgroup); False: k1_partial_fp8 + k1_combine."""
    B, n, H, D = q.shape
    assert q.is_contiguous() and out.is_contiguous() and k_cache.is_contiguous() and v_cache.is_contiguous()
    assert k_cache.dtype == FP8 and v_cache.dtype == FP8
    assert key_start is None or (key_start.dtype == torch.int32 and key_start.is_cuda)
    need = L.load().sjd_attention_workspace_bytes(B, H, n, D, n_split)
    assert workspace.numel() * 4 >= need, "attention workspace too small"
    if K1_MERGED_DEFAULT if merged is None else merged:
        L.check(L.load_exp().sjd_draft_window_attention_fp8_merged(_ptr(q), _ptr(k_cache), _ptr(v_cache), _ptr(out), B, n, H, k_cache.shape[1], D,
                                                              k_cache.shape[2], _dtype_code(q.dtype), float(k_scale), float(v_scale),
                                                              _ptr(key_start), params.ptr if params is not None else None, int(kv_len),
                                                              int(n_split), _ptr(workspace), _ptr(k1_tickets(B, k_cache.shape[1], n, q.device)),
                                                              _stream()), "sjd_draft_window_attention_fp8_merged")
        return
    L.check(L.load().sjd_draft_window_attention_fp8(_ptr(q), _ptr(k_cache), _ptr(v_cache), _ptr(out), B, n, H, k_cache.shape[1], D,
                                                   k_cache.shape[2], _dtype_code(q.dtype), float(k_scale), float(v_scale),
                                                   _ptr(key_start), params.ptr if params is not None else None, int(kv_len),
                                                   int(n_split), _ptr(workspace), _stream()), "sjd_draft_window_attention_fp8")


def colsplit_ok(B, n, H, H_kv, D, cache_dtype):
    """shapes sjd_draft_window_attention(_fp8)_colsplit serves: one prompt's multi-head 16-row window, head size 128"""
    return H == H_kv and D == 128 and n <= 16 and B * H <= 64 and cache_dtype in (torch.bfloat16, torch.float16, FP8)


def _k1_mode(head_dim, D):
    """the K1 mode bit of a logical head dim: None or D = none; 100 at D = 128 = SJD_K1_HEAD_DIM_100 (16-bit caches)"""
    if head_dim is None or head_dim == D:
        return 0
    if (head_dim, D) != (100, 128):
        raise L.SjdLibraryError(f"K1 serves a logical head_dim of 100 stored 128 wide only, got {head_dim} at D = {D}")
    return L.K1_HEAD_DIM_100


def draft_window_attention_colsplit(q, k_cache, v_cache, out, key_start, params, kv_len, kv_scale=(1.0, 1.0), head_dim=None):
    """K1 without key splits: four workgroups per (batch, head) split the output columns, one launch, no workspace (see include/sjd_hip.h).
    head_dim: the logical head dim where it differs from the stored D (100 at D = 128: zero pad columns, softmax scale 1/sqrt(100))."""
    B, n, H, D = q.shape
    assert q.is_contiguous() and out.is_contiguous() and k_cache.is_contiguous() and v_cache.is_contiguous()
    assert key_start is None or (key_start.dtype == torch.int32 and key_start.is_cuda)
    if k_cache.dtype == FP8:
        L.check(L.load().sjd_draft_window_attention_fp8_colsplit(_ptr(q), _ptr(k_cache), _ptr(v_cache), _ptr(out), B, n, H, k_cache.shape[1], D,
                                                                k_cache.shape[2], _dtype_code(q.dtype) | _k1_mode(head_dim, D), float(kv_scale[0]),
                                                                float(kv_scale[1]), _ptr(key_start), params.ptr if params is not None else None,
                                                                int(kv_len), _stream()), "sjd_draft_window_attention_fp8_colsplit")
    else:
        L.check(L.load().sjd_draft_window_attention_colsplit(_ptr(q), _ptr(k_cache), _ptr(v_cache), _ptr(out), B, n, H, k_cache.shape[1], D,
                                                            k_cache.shape[2], _dtype_code(q.dtype) | _k1_mode(head_dim, D), _ptr(key_start),
                                                            params.ptr if params is not None else None, int(kv_len), _stream()),
                "sjd_draft_window_attention_colsplit")


def attention_workspace(B, H, n_rows, D, n_split, device):
    nbytes = L.load().sjd_attention_workspace_bytes(B, H, n_rows, D, n_split)
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device)


def draft_window_attention(q, k_cache, v_cache, out, key_start, params, kv_len, n_split, workspace, ev0=None, ev1=None, merged=None, head_dim=None):
    """q/out [B,n,H,D]; caches [B,Hkv,S,D] already holding the window rows; key_start int32 [B] (device).
    ev0/ev1: optional raw hipEvent_t handles recorded around the k1_partial launch.  merged: one launch -- the key splits are merged by
    the last of their workgroups to finish (same output bits); False: k1_partial + k1_combine, two launches.
    head_dim: the logical head dim where it differs from the stored D (see draft_window_attention_colsplit)."""
    B, n, H, D = q.shape
    dcode = _dtype_code(q.dtype) | _k1_mode(head_dim, D)
    assert q.is_contiguous() and out.is_contiguous() and k_cache.is_contiguous() and v_cache.is_contiguous()
    assert key_start is None or (key_start.dtype == torch.int32 and key_start.is_cuda)
    need = L.load().sjd_attention_workspace_bytes(B, H, n, D, n_split)
    assert workspace.numel() * 4 >= need, "attention workspace too small"
    if (K1_MERGED_DEFAULT if merged is None else merged) and q.dtype != torch.float32:
        L.check(L.load_exp().sjd_draft_window_attention_merged(_ptr(q), _ptr(k_cache), _ptr(v_cache), _ptr(out), B, n, H,
                                                          k_cache.shape[1], D, k_cache.shape[2], dcode,
                                                          _ptr(key_start), params.ptr if params is not None else None,
                                                          int(kv_len), int(n_split), _ptr(workspace), _ptr(k1_tickets(B, k_cache.shape[1], n, q.device)),
                                                          _stream(), ev0, ev1), "sjd_draft_window_attention_merged")
        return
    L.check(L.load().sjd_draft_window_attention_ex(_ptr(q), _ptr(k_cache), _ptr(v_cache), _ptr(out), B, n, H,
                                                  k_cache.shape[1], D, k_cache.shape[2], dcode,
                                                  _ptr(key_start), params.ptr if params is not None else None,
                                                  int(kv_len), int(n_split), _ptr(workspace), _stream(), ev0, ev1),
            "sjd_draft_window_attention")


class Partials:
    """fp32 split-K partial products [n_chunks, 32, N] of a G1 projection; consumers (F1/F2/F3) sum the chunks."""

    def __init__(self, data, n_chunks, N):
        self.data, self.n_chunks, self.N = data, n_chunks, N


def pack_weight(weight, KC, step_major=False):
    """[N, K] linear weight -> MFMA 32x32x16 B-fragment-major stream for sjd_skinny_gemm: for every k-chunk c and
    32-column tile t a contiguous run of (chunk_k/16) 1-KiB records; record s, lane l, element j =
    W[32t + (l&31)][k0 + 16s + 8(l>>5) + j]."""
    N, K = weight.shape
    assert N % 32 == 0 and K % 16 == 0 and KC % 16 == 0
    out = []
    for k0 in range(0, K, KC):
        kc = min(KC, K - k0)
        w = weight[:, k0:k0 + kc].reshape(N // 32, 32, kc // 16, 2, 8)      # [t, r, s, h, j]
        if step_major:
            out.append(w.permute(2, 0, 3, 1, 4).reshape(-1))                # [s, t, h, r, j] : records of all tiles per k-step
        else:
            out.append(w.permute(0, 2, 3, 1, 4).reshape(-1))                # [t, s, h, r, j] ; lane = 32h + r
    return torch.cat(out).contiguous()


class Packed:
    """a packed weight that is more than pack_weight's tensor: PackedZ, or a copy of a row of LS.STREAMS (which names it in `weight_stream`: see streamed)"""

    def numel(self):
        return self.N * self.K


class PackedZ(Packed):
    """A packed weight in the 12-bit lossless stream format of kernels G1z / G1sz (see pack_weight_z): `data` uint8 [N * K * 3 / 2] (1536-byte
    record pairs in pack_weight's record order), `exc` int32 [n_chunks, N / 32, cap, 2] (per-unit base / count and exceptions).  RAW units (round 6:
    more out-of-window weights than a header holds) are zero-filled in `data`; their weights travel verbatim in `raw_data` (pack_weight's 1-KiB
    records, KC / 16 per unit) and the launches behind the stream kernels recompute the tiles they feed: `raw_index` int32 [n_raw, 2] = (chunk,
    tile) of unit i of `raw_data`; a weight packed with gateup=True additionally lists the gate tiles of the raw (gate, up) PAIRS in `raw_tiles`
    int32 [n_pairs] -- its raw units are ordered [pair][K half][gate | up], so the same `raw_data` serves both fix-up kernels."""

    def __init__(self, data, exc, N, K, KC, step_major, n_exceptions, raw_index=None, raw_tiles=None, raw_data=None, stats=None):
        self.data, self.exc, self.N, self.K, self.KC, self.step_major, self.n_exceptions = data, exc, N, K, KC, bool(step_major), int(n_exceptions)
        self.cap = int(exc.shape[2])
        self.raw_index, self.raw_tiles, self.raw_data = raw_index, raw_tiles, raw_data
        self.n_raw = 0 if raw_data is None else int(raw_index.shape[0])
        self.n_raw_pairs = 0 if raw_tiles is None else int(raw_tiles.shape[0])
        self.stats = stats or {}

    def nbytes(self):
        return self.data.numel() + self.exc.numel() * 4 + (0 if self.raw_data is None else self.raw_data.numel() * 2)


Z_MAX_EXC = 127         # exceptions a (k-chunk, 32-column tile) unit can carry: headers of 32 / 64 / 128 entries, chosen per matrix


def pack_weight_z(weight, KC, step_major=False, gateup=False):
    """[N, K] bf16 weight -> PackedZ, the LOSSLESS 12-bit form of pack_weight(weight, KC, step_major) that sjd_skinny_gemm_z / sjd_gateup_silu_z
    stream (include/sjd_hip.h), or None when the format does not apply (not bf16, KC > 4096).
    The header of a unit has 32 entries (31 exceptions: Gaussian weights need 3-13) or, for the whole matrix, 64 / 128 when some unit needs
    them (heavy-tailed weights, norm gains folded into the columns: 10-30 per 16 k-weight unit).
    Per unit (k-chunk c, tile t) the window of eight consecutive values of the weights' 7 high exponent bits that covers most of the unit is
    chosen from the unit's histogram (robust against outliers on either side); a weight inside it is stored as low byte + code
    (sign << 3 | offset), one outside it additionally verbatim as an exception.
    A unit with more than 127 exceptions (zero rows, pruned blocks, weights spanning more than sixteen binades) is RAW (round 6; the packer
    used to decline the whole matrix): see PackedZ.  gateup=True: `weight` is [Wg; Wu] packed with KC = K / 2 for sjd_gateup_silu_z -- a raw
    unit makes the packer list its whole (gate tile, up tile) pair, both K halves."""
    if weight.dtype != torch.bfloat16 or KC > LS.Z_MAX_KC:
        return None
    N, K = weight.shape
    assert N % 32 == 0 and K % 16 == 0 and KC % 16 == 0
    T, dev = N // 32, weight.device
    n_chunks = (K + KC - 1) // KC
    assert not gateup or (2 * KC == K and T % 2 == 0)
    bits = weight.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    # ---- pass 1: per unit the window and its exception count -> which units are raw
    bases, cnts = [], []
    for k0 in range(0, K, KC):
        kc = min(KC, K - k0)
        S = kc // 16
        eh = (bits[:, k0:k0 + kc].reshape(T, 32 * kc) >> 8) & 0x7F
        hist = torch.zeros(T, 128, dtype=torch.int64, device=dev)
        hist.scatter_add_(1, eh.to(torch.int64), torch.ones(1, dtype=torch.int64, device=dev).expand(T, 32 * kc))
        cs = torch.cat([torch.zeros(T, 1, dtype=torch.int64, device=dev), hist.cumsum(1)], dim=1)
        inside = cs[:, 8:129] - cs[:, 0:121]
        base = inside.argmax(dim=1)
        bases.append(base.to(torch.int32))                                   # [T] in 0..120: window [base, base + 7]
        cnts.append(32 * kc - inside.gather(1, base[:, None])[:, 0])
    cnt_all = torch.stack(cnts)                                              # [n_chunks, T]
    raw_mask = cnt_all > Z_MAX_EXC
    if gateup and bool(raw_mask.any()):                                      # a raw unit anywhere in a (gate, up) pair: the pair, both K halves
        pair = raw_mask.reshape(n_chunks, 2, T // 2).any(dim=0).any(dim=0)   # [T / 2]
        raw_mask = pair[None, None, :].expand(n_chunks, 2, T // 2).reshape(n_chunks, T).clone()
    stats = dict(units=int(n_chunks * T), raw_units=int(raw_mask.sum()), max_exceptions=int(cnt_all[~raw_mask].max()) if bool((~raw_mask).any()) else 0,
                 mean_exceptions=float(cnt_all[~raw_mask].float().mean()) if bool((~raw_mask).any()) else 0.0)
    # ---- pass 2: encode
    datas, hdrs, total, max_cnt = [], [], 0, 0
    for ci, k0 in enumerate(range(0, K, KC)):
        kc = min(KC, K - k0)
        S = kc // 16
        b = bits[:, k0:k0 + kc].reshape(T, 32, S, 2, 8)                     # [t, r, s, h, j]
        rm = raw_mask[ci]
        if bool(rm.any()):
            b = torch.where(rm.view(T, 1, 1, 1, 1), torch.zeros_like(b), b)  # a raw unit's slot in the stream: zeros (code 0, low byte 0, base 0)
        base = torch.where(rm, torch.zeros_like(bases[ci]), bases[ci])
        eh = (b >> 8) & 0x7F
        e3 = eh - base.view(T, 1, 1, 1, 1)
        bad = ((e3 < 0) | (e3 > 7)) & ~rm.view(T, 1, 1, 1, 1)
        cnt = bad.reshape(T, -1).sum(dim=1)
        max_cnt = max(max_cnt, int(cnt.max()))
        code = ((b >> 15) << 3) | e3.clamp(0, 7)                             # [t, r, s, h, j]
        lo = b & 0xFF
        lo0 = lo[..., 0] | (lo[..., 1] << 8) | (lo[..., 2] << 16) | (lo[..., 3] << 24)        # int32 wrap-around is the bit pattern wanted
        lo1 = lo[..., 4] | (lo[..., 5] << 8) | (lo[..., 6] << 16) | (lo[..., 7] << 24)
        cb = code[..., 0:4] | (code[..., 4:8] << 4)
        cw = cb[..., 0] | (cb[..., 1] << 8) | (cb[..., 2] << 16) | (cb[..., 3] << 24)
        # record PAIR p = k-steps 2p, 2p + 1 (an odd last k-step is padded with zeros): 64 lanes (= 32 h + r) x {lo0, lo1 of 2p; lo0, lo1 of
        # 2p + 1}, then 64 lanes x {cw of 2p, cw of 2p + 1}  -> 256 + 128 int32: one 16-byte and one 8-byte load per lane, both aligned
        P = (S + 1) // 2
        st = torch.stack([lo0, lo1, cw], dim=-1).permute(0, 2, 3, 1, 4)                         # [t, s, h, r, 3]
        if S % 2:
            st = torch.cat([st, torch.zeros_like(st[:, :1])], dim=1)
        st = st.reshape(T, P, 2, 64, 3)                                                         # [t, p, k-step of the pair, lane, 3]
        lo_part = st[..., :2].permute(0, 1, 3, 2, 4).reshape(T, P, 256)                         # lane-major: (lane, k-step, 2)
        c_part = st[..., 2].permute(0, 1, 3, 2).reshape(T, P, 128)                              # (lane, k-step)
        rec = torch.cat([lo_part, c_part], dim=-1)                                              # [t, p, 384]
        if step_major:
            rec = rec.permute(1, 0, 2)
        datas.append(rec.reshape(-1))
        hdr = torch.full((T, Z_MAX_EXC + 1, 2), -1, dtype=torch.int32, device=dev)       # (cut to the matrix's capacity below)
        hdr[:, 0, 0] = base
        hdr[:, 0, 1] = torch.where(rm, torch.full_like(cnt, -1), cnt).to(torch.int32)     # (-1: a raw unit; entry 1 then holds where its records are)
        idx = bad.nonzero()                                                  # rows sorted by t first
        if idx.numel():
            t_i, r_i, s_i, h_i, j_i = idx.unbind(1)
            first = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), cnt.cumsum(0)[:-1]])
            rank = torch.arange(idx.shape[0], device=dev) - first[t_i]
            hdr[t_i, 1 + rank, 0] = ((s_i << 9) | ((32 * h_i + r_i) << 3) | j_i).to(torch.int32)
            hdr[t_i, 1 + rank, 1] = b[t_i, r_i, s_i, h_i, j_i]
            total += idx.shape[0]
        hdrs.append(hdr)
    data = torch.cat(datas).contiguous().view(torch.uint8)
    cap = 32 if max_cnt <= 31 else 64 if max_cnt <= 63 else 128
    # ---- the raw units' weights, verbatim, in pack_weight's record order ([s, h, r, j]: lane = 32 h + r), KC / 16 records per unit
    raw_index = raw_tiles = raw_data = None
    if stats["raw_units"]:
        SF = KC // 16

        def unit_records(ci, t):
            k0 = ci * KC
            kc = min(KC, K - k0)
            u = weight[32 * t:32 * t + 32, k0:k0 + kc].reshape(32, kc // 16, 2, 8).permute(1, 2, 0, 3).reshape(kc // 16, 512)
            if kc // 16 < SF:
                u = torch.cat([u, torch.zeros(SF - kc // 16, 512, dtype=u.dtype, device=dev)])
            return u
        if gateup:                      # units ordered [pair][K half][gate | up]
            tiles = raw_mask[0, :T // 2].nonzero()[:, 0]
            raw_tiles = tiles.to(torch.int32).contiguous()
            units = [(kh, int(t) + gu * (T // 2)) for t in tiles.tolist() for kh in (0, 1) for gu in (0, 1)]
        else:
            units = [(int(c), int(t)) for c, t in raw_mask.nonzero().tolist()]
        raw_index = torch.tensor(units, dtype=torch.int32, device=dev).contiguous()
        raw_data = torch.stack([unit_records(c, t) for c, t in units]).contiguous()
    # ONE allocation: the headers, then the raw units' records -- a kernel reaches a raw unit's records from `exc` through the byte offset in
    # entry 1 of the unit's header (csrc/sjd_gemm.hip: g1z_raw_records), so no kernel takes another pointer argument
    hdr_all = torch.stack(hdrs)[:, :, :cap].contiguous()
    if raw_data is None:
        return PackedZ(data, hdr_all, N, K, KC, step_major, total, None, None, None, stats)
    hdr_ints = hdr_all.numel()
    assert hdr_ints * 4 + raw_data.numel() * 2 < 2 ** 31
    for u, (c, t) in enumerate(units):
        hdr_all[c, t, 1, 0] = hdr_ints * 4 + u * (KC // 16) * 1024
        hdr_all[c, t, 1, 1] = 0
    blob = torch.cat([hdr_all.reshape(-1), raw_data.reshape(-1).view(torch.int32)]).contiguous()
    exc = blob[:hdr_ints].view(hdr_all.shape)
    raw_view = blob[hdr_ints:].view(torch.bfloat16).view(raw_data.shape)
    return PackedZ(data, exc, N, K, KC, step_major, total, raw_index, raw_tiles, raw_view, stats)


class _PackedQuant(Packed):
    """what the quantised stream formats share: `data` uint8 = the records, then the scales; LOSSY -- the kernels multiply by dequant(), exactly"""

    dtype = torch.bfloat16          # the activation type the kernels take (and the type of dequant()); a subclass adds `weight_stream`, its row of LS.STREAMS

    def __init__(self, data, N, K, KC, step_major, stats=None):
        self.data, self.N, self.K, self.KC, self.step_major = data, int(N), int(K), int(KC), bool(step_major)
        self.stats = stats or {}

    def nbytes(self):
        return self.data.numel()


def _rel_rms_error(weight, dequantised):
    """RMS(w - dequant) / RMS(w) (0 for an all-zero matrix): what compress_stats judges a quantised matrix by"""
    wf = weight.float()
    rms = float(wf.pow(2).mean().sqrt())
    return float((wf - dequantised.float()).pow(2).mean().sqrt()) / rms if rms > 0 else 0.0


class PackedQ8(_PackedQuant):
    """A packed weight in the 8-bit (OCP e4m3fn) stream format of kernels G1q / G1sq (see pack_weight_q8): `data` uint8 [N * K + 4 * N] = the
    records, one byte per weight, then the fp32 column scales [N] at byte offset N * K.  LOSSY: the kernels multiply by dequant(), exactly."""

    weight_stream = LS.STREAMS[0]

    def reads_as(self, KC):
        """can a launch with split-K chunk KC stream this buffer?  The chunk it was packed with -- or, step-major with K and both chunks multiples of
        32, any other: every chunk is then whole record pairs and the buffer is [pair][tile] throughout, whatever the chunking"""
        return KC == self.KC or (self.step_major and self.K % 32 == 0 and self.KC % 32 == 0 and KC % 32 == 0)

    def scales(self):
        """fp32 [N] view of the column scales inside `data`"""
        return self.data[self.N * self.K:].view(torch.float32)

    def codes(self):
        """uint8 [N, K]: the e4m3 codes read back from the packed records (the inverse of pack_weight_q8's permutation)"""
        N, K, KC, T = self.N, self.K, self.KC, self.N // 32
        cols, off = [], 0
        for k0 in range(0, K, KC):
            kc = min(KC, K - k0)
            S = kc // 16
            P = S // 2
            blk = self.data[off:off + N * kc]
            off += N * kc
            if self.step_major:
                pr, hf = blk[:P * T * 1024].reshape(P, T, 1024).permute(1, 0, 2), blk[P * T * 1024:].reshape(T, (S - 2 * P) * 512)
            else:
                u = blk.reshape(T, S * 512)
                pr, hf = u[:, :P * 1024].reshape(T, P, 1024), u[:, P * 1024:]
            st = pr.reshape(T, P, 64, 2, 8).permute(0, 1, 3, 2, 4).reshape(T, 2 * P, 64, 8)          # [t, s, lane, j]
            st = torch.cat([st, hf.reshape(T, S - 2 * P, 64, 8)], dim=1)
            cols.append(st.reshape(T, S, 2, 32, 8).permute(0, 3, 1, 2, 4).reshape(N, kc))            # [t, s, h, r, j] -> [t, r, s, h, j]
        return torch.cat(cols, dim=1).contiguous()

    def dequant(self):
        """bf16 [N, K]: the weight the kernels multiply by, read back from the packed buffer (exact: 3 mantissa bits times a power of two)"""
        return (self.codes().view(FP8).float() * self.scales()[:, None]).to(torch.bfloat16)


Q8_MIN_SCALE_EXP = -117     # 2^-9 (the smallest e4m3 magnitude) * 2^-117 = 2^-126: every dequantised value is a NORMAL bf16 number or zero


def quantize_e4m3(weight):
    """[N, K] bf16 weight -> (q uint8 [N, K] of OCP e4m3fn codes, scale fp32 [N]): one power-of-two scale per output column n (row of `weight`),
    scale[n] = 2^ceil(log2(amax_n / 448)) (1 for an all-zero column; never below 2^-117, so that q * scale has no bf16 denormals),
    q = e4m3(w / scale), round to nearest even.  |w / scale| <= 448 by construction: nothing saturates and the NaN codes 0x7f / 0xff never
    appear.  q * scale is exactly representable in bf16.  fp16 (whose exponent range does not hold the scaled values in general) raises."""
    if weight.dtype != torch.bfloat16:
        raise ValueError(f"quantize_e4m3: bf16 weights only (got {weight.dtype}): the dequantised values are bf16 numbers, fp16's exponent range does not hold them")
    if weight.dim() != 2:
        raise ValueError("quantize_e4m3: a [N, K] matrix")
    w = weight.float()
    if not bool(torch.isfinite(w).all()):
        raise ValueError("quantize_e4m3: the weight has non-finite values")
    amax = w.abs().amax(dim=1)
    m, e = torch.frexp(amax)                                      # amax = m * 2^e, m in [0.5, 1); 448 = 0.875 * 2^9
    exp = (e - 9 + (m > 0.875).to(e.dtype)).clamp(min=Q8_MIN_SCALE_EXP)
    exp = torch.where(amax > 0, exp, torch.zeros_like(exp)).to(torch.int32)
    # scale and 1 / scale built from their exponent bits: exact on every device.  torch.ldexp(1, e) is NOT on the GPU (a pow() underneath: one ulp below
    # 2^e at e = 16..20, 22, ... on the MI355X), and the kernels take the scale's EXPONENT FIELD (v_cvt_scalef32_pk_bf16_fp8): such a column was
    # multiplied by half its scale, while dequant(), a float product rounded to bf16, still gave the right weight (tests/test_gpu_gemm_exact.py)
    scale = ((127 + exp) << 23).view(torch.float32)
    inv = ((127 - exp) << 23).view(torch.float32)
    q = (w * inv[:, None]).to(FP8).view(torch.uint8)               # exact: a power of two
    return q, scale


def pack_weight_q8(weight, KC, step_major=False, gateup=False):
    """[N, K] bf16 weight -> PackedQ8: quantize_e4m3(weight) in pack_weight(weight, KC, step_major)'s (k-chunk, 32-column tile, k-step, lane,
    element) order at ONE BYTE per weight, then the fp32 column scales [N] at byte offset N * K (a multiple of 512) of the same buffer -- what
    sjd_skinny_gemm / sjd_skinny_gemm_cols / sjd_gateup_silu stream under SJD_G1_W8_E4M3 (kernels G1q / G1sq, csrc/sjd_gemm_q8.h).
    Byte layout: the k-steps of a unit (chunk c, tile t) travel in PAIRS -- pair p (1024 B) = 64 lanes x 16 B {the lane's 8 bytes of k-step 2p, its
    8 bytes of k-step 2p + 1}, lane l = 32 h + r, byte j = q[32 t + r][k0 + 16 s + 8 h + j] -- and an odd last k-step (a ragged last chunk) is a HALF
    record of 512 B = 64 lanes x 8 B behind the pairs: no padding.  Tile-major: a unit is S * 512 contiguous bytes; step_major: a chunk holds
    pair 0 of every tile, pair 1 of every tile, ..., then the half record of every tile.  A chunk starts at byte k0 * N.
    gateup=True: `weight` is [Wg; Wu] packed with KC = K / 2 for sjd_gateup_silu.
    stats: rel_rms_error (RMS of w - dequant over RMS of w), scale_exp_min / scale_exp_max (log2 of the smallest / largest column scale)."""
    q, scale = quantize_e4m3(weight)
    N, K = weight.shape
    assert N % 32 == 0 and K % 16 == 0 and KC % 16 == 0
    T = N // 32
    assert not gateup or (2 * KC == K and T % 2 == 0)
    parts = []
    for k0 in range(0, K, KC):
        kc = min(KC, K - k0)
        S = kc // 16
        P = S // 2
        b = q[:, k0:k0 + kc].reshape(T, 32, S, 2, 8).permute(0, 2, 3, 1, 4).reshape(T, S, 64, 8)     # [t, s, lane = 32 h + r, j]
        pr = b[:, :2 * P].reshape(T, P, 2, 64, 8).permute(0, 1, 3, 2, 4).reshape(T, P, 1024)          # (lane, k-step of the pair, j)
        hf = b[:, 2 * P:].reshape(T, (S - 2 * P) * 512)
        if step_major:
            parts += [pr.permute(1, 0, 2).reshape(-1), hf.reshape(-1)]
        else:
            parts.append(torch.cat([pr.reshape(T, P * 1024), hf], dim=1).reshape(-1))
    data = torch.cat(parts + [scale.contiguous().view(torch.uint8)]).contiguous()
    lg = (scale.view(torch.int32) >> 23) - 127                     # (the exponent field: a log2() need not be exact on every device either)
    stats = dict(rel_rms_error=_rel_rms_error(weight, q.view(FP8).float() * scale[:, None]), scale_exp_min=int(lg.min()), scale_exp_max=int(lg.max()))
    return PackedQ8(data, N, K, KC, step_major, stats)


Q4_GRANULE = LS.Q4_GRANULE  # K granule of the MXFP4 stream (128): K and every chunk are whole ring trips of eight k-steps = two records = one scale dword per column
Q4_MIN_SCALE_EXP = -125     # 0.5 (the smallest non-zero e2m1 magnitude) * 2^-125 = 2^-126: every dequantised value is a NORMAL bf16 number or zero
Q4_MAX_SCALE_EXP = 125      # 6 (the largest) * 2^125 is a finite bf16 number; 4 * 2^126 would not be
_E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
_E2M1_MIDPOINTS = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)       # between code i and i + 1; a tie goes to the even code


def quantize_mxfp4(weight):
    """[N, K] bf16 weight (K % 32 == 0) -> (codes uint8 [N, K / 2], scale_exp uint8 [N, K / 32]): OCP MXFP4.  One e8m0 scale per output column n (row of
    `weight`) and block of 32 consecutive k: scale = 2^ceil(log2(amax_block / 6)) (1 for an all-zero block; never below 2^-125, so that 0.5 * scale, the
    smallest non-zero dequantised value, is a normal bf16 number), stored as the byte log2(scale) + 127.  Codes are e2m1 -- sign << 3 | index into
    {0, 0.5, 1, 1.5, 2, 3, 4, 6} -- of w / scale, round to nearest even; two per byte, even k in the low nibble.  amax <= 6 * scale by construction:
    nothing saturates.  code * scale is exactly a bf16 number, and |w - code * scale| <= max(scale, |w|) / 4 for every element (the grid's step is
    0.5 up to 2, 1 up to 4, 2 up to 6: half a step is <= scale / 4 below 2 and <= |w| / 4 above).  fp16 raises; so does a block whose scale would
    exceed 2^125 (|w| above 6 * 2^125)."""
    if weight.dtype != torch.bfloat16:
        raise ValueError(f"quantize_mxfp4: bf16 weights only (got {weight.dtype}): the dequantised values are bf16 numbers, fp16's exponent range does not hold them")
    if weight.dim() != 2 or weight.shape[1] % 32:
        raise ValueError("quantize_mxfp4: a [N, K] matrix with K a multiple of 32 (one scale per block of 32)")
    w = weight.float()
    if not bool(torch.isfinite(w).all()):
        raise ValueError("quantize_mxfp4: the weight has non-finite values")
    N, K = w.shape
    blk = w.reshape(N, K // 32, 32)
    amax = blk.abs().amax(dim=2)
    m, e = torch.frexp(amax)                                      # amax = m * 2^e, m in [0.5, 1); 6 = 0.75 * 2^3
    exp = (e - 3 + (m > 0.75).to(e.dtype)).clamp(min=Q4_MIN_SCALE_EXP)
    exp = torch.where(amax > 0, exp, torch.zeros_like(exp))
    if int(exp.max()) > Q4_MAX_SCALE_EXP:
        raise ValueError(f"quantize_mxfp4: a block needs a scale above 2^{Q4_MAX_SCALE_EXP} (|w| > 6 * 2^{Q4_MAX_SCALE_EXP}): code * scale would not be a bf16 number")
    inv = ((127 - exp).to(torch.int32) << 23).view(torch.float32)          # 1 / scale, built from its exponent bits: exact on every device (a pow() need not be)
    v = blk.abs() * inv[:, :, None]                               # exact: a power of two
    idx = torch.zeros_like(v, dtype=torch.uint8)
    for i, mid in enumerate(_E2M1_MIDPOINTS):
        idx += ((v >= mid) if i % 2 else (v > mid)).to(torch.uint8)
    nib = (idx | (torch.signbit(blk).to(torch.uint8) << 3)).reshape(N, K)
    codes = (nib[:, 0::2] | (nib[:, 1::2] << 4)).contiguous()
    return codes, (exp + 127).to(torch.uint8)


def dequantize_mxfp4(codes, scale_exp):
    """(codes uint8 [N, K / 2], scale_exp uint8 [N, K / 32]) -> bf16 [N, K]: code * scale, exactly (a -0 code stays -0)"""
    N, K = codes.shape[0], 2 * codes.shape[1]
    nib = torch.stack([codes & 0xF, codes >> 4], dim=2).reshape(N, K).long()
    lut = torch.tensor(_E2M1_VALUES + tuple(-x for x in _E2M1_VALUES), dtype=torch.float32, device=codes.device)
    scale = (scale_exp.to(torch.int32) << 23).view(torch.float32)          # the e8m0 byte is the float's exponent field: what the kernels do
    return (lut[nib].reshape(N, K // 32, 32) * scale[:, :, None]).reshape(N, K).to(torch.bfloat16)


class _PackedBlockQuant(_PackedQuant):
    """what the block-scaled stream formats (MXFP4, e2m3) share: 64-k records of REC code bytes per 32-column tile, tile- or step-major per chunk, then
    one e8m0 scale byte per 32 weights in groups of 128 bytes per tile and trip of two records, laid out like the records.  A subclass supplies REC and
    its record permutation both ways: _to_records (a chunk's columns of the quantiser's codes -> [T, R, REC]) and _from_records."""

    def reads_as(self, KC):
        """can a launch with split-K chunk KC stream this buffer?  The chunk it was packed with -- or, step-major, any other multiple of the granule:
        every chunk is then whole records and whole scale groups and the buffer is [record][tile], then [trip][tile], throughout, whatever the chunking"""
        return KC == self.KC or (self.step_major and self.KC % Q4_GRANULE == 0 and KC % Q4_GRANULE == 0)

    def _chunks(self):
        return [(k0, min(self.KC, self.K - k0)) for k0 in range(0, self.K, self.KC)]

    def _groups(self, off, width, k_per):
        """the chunk walk: per chunk its groups [T, kc / k_per, width] (records: 64 k each; a trip's scales: 128 k) from byte `off` of `data` on"""
        T = self.N // 32
        for _, kc in self._chunks():
            G = kc // k_per
            blk = self.data[off:off + T * G * width]
            off += T * G * width
            yield blk.reshape(G, T, width).permute(1, 0, 2) if self.step_major else blk.reshape(T, G, width)

    def codes(self):
        """uint8, the codes as the stream's quantiser returns them (MXFP4: [N, K / 2], the e2m1 codes, two per byte; e2m3: [N, K], one per byte), read
        back from the packed records (the inverse of the packer's permutation)"""
        return torch.cat([self._from_records(rec) for rec in self._groups(0, self.REC, 64)], dim=1).contiguous()

    def scale_exp(self):
        """uint8 [N, K / 32]: the e8m0 scale bytes (e2m3: column 2 R + h, quantize_e2m3's) read back from behind the records"""
        T = self.N // 32
        cols = [grp.reshape(T, -1, 32, 4).permute(0, 2, 1, 3).reshape(self.N, -1) for grp in self._groups(T * (self.K // 64) * self.REC, 128, 128)]
        return torch.cat(cols, dim=1).contiguous()


def _pack_block_quant(cls, name, quantize, dequantize, weight, KC, step_major, gateup):
    """the packer of a block-scaled stream: `quantize`'s codes as cls's records chunk by chunk, then its scale bytes in groups of 128 (see cls)"""
    if weight.dim() != 2 or weight.shape[1] % Q4_GRANULE or KC < Q4_GRANULE or KC % Q4_GRANULE:
        raise ValueError(f"{name}: K and KC must be multiples of {Q4_GRANULE} (whole records and scale dwords); got K = {tuple(weight.shape)[-1]}, KC = {KC}")
    codes, se = quantize(weight)
    N, K = weight.shape
    assert N % 32 == 0
    T, W = N // 32, codes.shape[1]
    assert not gateup or (2 * KC == K and T % 2 == 0)
    cparts, sparts = [], []
    for k0 in range(0, K, KC):
        kc = min(KC, K - k0)
        rec = cls._to_records(codes[:, k0 * W // K:(k0 + kc) * W // K], T)
        grp = se[:, k0 // 32:(k0 + kc) // 32].reshape(T, 32, kc // 128, 4).permute(0, 2, 1, 3).reshape(T, kc // 128, 128)
        if step_major:
            rec, grp = rec.permute(1, 0, 2), grp.permute(1, 0, 2)
        cparts.append(rec.reshape(-1))
        sparts.append(grp.reshape(-1))
    data = torch.cat(cparts + sparts).contiguous()
    assert data.numel() == T * (K // 64) * cls.REC + N * K // 32
    stats = dict(rel_rms_error=_rel_rms_error(weight, dequantize(codes, se)), scale_exp_min=int(se.min()) - 127, scale_exp_max=int(se.max()) - 127)
    return cls(data, N, K, KC, step_major, stats)


class PackedQ4(_PackedBlockQuant):
    """A packed weight in the MXFP4 stream format of kernels G1q4 / G1sq4 (see pack_weight_q4): `data` uint8 [N * K / 2 + N * K / 32] = the code
    records, four bits per weight, then the e8m0 scale bytes at byte offset N * K / 2.  LOSSY: the kernels multiply by dequant(), exactly."""

    weight_stream, REC = LS.STREAMS[1], 1024

    @staticmethod
    def _to_records(c, T):
        b = c.reshape(T, 32, -1, 2, 4).permute(0, 2, 3, 1, 4).reshape(T, -1, 4, 64, 4)      # [t, r, s, h, b] -> [t, R, i, lane = 32 h + r, b]
        return b.permute(0, 1, 3, 2, 4).reshape(T, -1, 1024)

    @staticmethod
    def _from_records(rec):
        T, R = rec.shape[:2]
        st = rec.reshape(T, R, 64, 4, 4).permute(0, 1, 3, 2, 4).reshape(T, 4 * R, 2, 32, 4)         # [t, R, lane, i, b] -> [t, s, h, r, b]
        return st.permute(0, 3, 1, 2, 4).reshape(32 * T, 32 * R)

    def dequant(self):
        """bf16 [N, K]: the weight the kernels multiply by, read back from the packed buffer (exact: one mantissa bit times a power of two)"""
        return dequantize_mxfp4(self.codes(), self.scale_exp())


def pack_weight_q4(weight, KC, step_major=False, gateup=False):
    """[N, K] bf16 weight -> PackedQ4: quantize_mxfp4(weight) in pack_weight(weight, KC, step_major)'s (k-chunk, 32-column tile, k-step, lane,
    element) order at FOUR BITS per weight, then the e8m0 scale bytes at byte offset N * K / 2 of the same buffer -- what sjd_skinny_gemm /
    sjd_skinny_gemm_cols / sjd_gateup_silu stream under SJD_G1_W4_MXFP4 (kernels G1q4 / G1sq4, csrc/sjd_gemm_q4.h).  N * K / 2 + N * K / 32 bytes.
    K granule Q4_GRANULE = 128: K and KC must be multiples of 128 (ValueError otherwise) -- a unit is then whole records and whole scale dwords.
    Byte layout: the k-steps of a unit (chunk c, tile t) travel in RECORDS of four -- record R (1024 B) = 64 lanes x 16 B {the lane's 4 bytes of
    k-step 4R, .., of k-step 4R + 3}, lane l = 32 h + r, byte b = the codes of q[32 t + r][k0 + 16 s + 8 h + 2 b] (low nibble) and [.. + 2 b + 1] (high).
    Tile-major: a unit is S * 256 contiguous bytes; step_major: a chunk holds record 0 of every tile, record 1 of every tile, ...  A chunk starts at
    byte k0 * N / 2.  Scales: per unit and trip q of eight k-steps 128 bytes = 32 columns x 4 bytes (blocks 4q .. 4q + 3 of the chunk), the trips laid
    out like the records; a chunk's scales start at scale byte k0 * N / 32.
    gateup=True: `weight` is [Wg; Wu] packed with KC = K / 2 for sjd_gateup_silu.
    stats: rel_rms_error (RMS of w - dequant over RMS of w), scale_exp_min / scale_exp_max (log2 of the smallest / largest block scale)."""
    return _pack_block_quant(PackedQ4, "pack_weight_q4", quantize_mxfp4, dequantize_mxfp4, weight, KC, step_major, gateup)


Q6_MIN_SCALE_EXP = -123     # 0.125 (the smallest non-zero e2m3 magnitude) * 2^-123 = 2^-126: every dequantised value is a NORMAL bf16 number or zero
Q6_MAX_SCALE_EXP = 125      # 7.5 (the largest) * 2^125 is a finite bf16 number; 7.5 * 2^126 would not be


def _q6_block_view(t, K):
    """[N, K] -> [N, K / 64, 2, 32]: the e2m3 stream's scale blocks (n, record R, lane half h) x element e = 8 u + j, k = 64 R + 16 u + 8 h + j"""
    return t.reshape(t.shape[0], K // 64, 4, 2, 8).permute(0, 1, 3, 2, 4).reshape(t.shape[0], K // 64, 2, 32)


def quantize_e2m3(weight):
    """[N, K] bf16 weight (K % 64 == 0) -> (codes uint8 [N, K], one 6-bit code per byte in the weight's own order; scale_exp uint8 [N, K / 32]): OCP e2m3
    elements under one e8m0 scale per block of 32 weights.  THE BLOCK IS NOT 32 CONSECUTIVE k: block (n, R, h) -- scale_exp[n, 2 R + h] -- holds the
    weights at k = 64 R + 16 u + 8 h + j, u = 0..3, j = 0..7: the 32 values ONE v_cvt_scalef32_pk32_bf16_fp6 of MFMA lane 32 h + r decodes into its B
    operands of the four k-steps of record R (csrc/sjd_gemm_q6.h).  A private stream format of this library, not an interchange format (not OCP MXFP6).
    Code: sign << 5 | 2 exponent bits (bias 1) | 3 mantissa bits = sign << 5 | index into {0, 0.125, .., 0.875 (subnormals), 1 .. 1.875 in steps of 0.125,
    2 .. 3.75 in steps of 0.25, 4 .. 7.5 in steps of 0.5}; no infinity, no NaN.  scale = 2^ceil(log2(amax_block / 7.5)) (1 for an all-zero block; never
    below 2^-123, so that 0.125 * scale is a normal bf16 number), stored as the byte log2(scale) + 127.  Codes are those of w / scale, round to nearest
    even.  amax <= 7.5 * scale by construction: nothing saturates.  code * scale is exactly a bf16 number, and |w - code * scale| <= max(scale, |w|) / 16
    for every element (half a grid step is scale / 16 below 2 and at most |w| / 16 above).  fp16 raises; so does a block whose scale would exceed 2^125."""
    if weight.dtype != torch.bfloat16:
        raise ValueError(f"quantize_e2m3: bf16 weights only (got {weight.dtype}): the dequantised values are bf16 numbers, fp16's exponent range does not hold them")
    if weight.dim() != 2 or weight.shape[1] % 64:
        raise ValueError("quantize_e2m3: a [N, K] matrix with K a multiple of 64 (a scale block spans the four k-steps of a 64-k record)")
    w = weight.float()
    if not bool(torch.isfinite(w).all()):
        raise ValueError("quantize_e2m3: the weight has non-finite values")
    N, K = w.shape
    blk = _q6_block_view(w, K)                                    # [n, R, h, e]
    amax = blk.abs().amax(dim=3)
    m, e = torch.frexp(amax)                                      # amax = m * 2^e, m in [0.5, 1); 7.5 = 0.9375 * 2^3
    exp = (e - 3 + (m > 0.9375).to(e.dtype)).clamp(min=Q6_MIN_SCALE_EXP)
    exp = torch.where(amax > 0, exp, torch.zeros_like(exp))
    if int(exp.max()) > Q6_MAX_SCALE_EXP:
        raise ValueError(f"quantize_e2m3: a block needs a scale above 2^{Q6_MAX_SCALE_EXP} (|w| > 7.5 * 2^{Q6_MAX_SCALE_EXP}): code * scale would not be a bf16 number")
    inv = ((127 - exp).to(torch.int32) << 23).view(torch.float32)          # 1 / scale, built from its exponent bits: exact on every device
    v = blk.abs() * inv[..., None]                                # exact: a power of two; <= 7.5
    # the grid's step is 2^-3 below 2, 2^-2 below 4, 2^-1 above; v / step has the parity of the code index on all three, so torch.round's ties-to-even
    # are the format's (a v just under 2 or 4 rounds up onto the next binade's first code, which both steps hit)
    sh = (v >= 2).to(torch.float32) + (v >= 4).to(torch.float32)
    n = torch.round(v * torch.ldexp(torch.full_like(v, 8.0), -sh.to(torch.int32)))          # 0..16 at sh = 0, 8..16 above
    up = ((n == 16) & (sh < 2)).to(torch.float32)                 # onto the next binade: (16, sh) = (8, sh + 1)
    n, sh = torch.where(up > 0, torch.full_like(n, 8.0), n), sh + up
    idx = torch.where(sh == 0, n, n + 8 * sh).to(torch.uint8)     # sh = 1: 16 + (n - 8); sh = 2: 24 + (n - 8)
    code = idx | (torch.signbit(blk).to(torch.uint8) << 5)
    codes = code.reshape(N, K // 64, 2, 4, 8).permute(0, 1, 3, 2, 4).reshape(N, K).contiguous()
    return codes, (exp + 127).to(torch.uint8).reshape(N, K // 32)


def dequantize_e2m3(codes, scale_exp):
    """(codes uint8 [N, K], scale_exp uint8 [N, K / 32]: quantize_e2m3's) -> bf16 [N, K]: code * scale, exactly (a -0 code stays -0)"""
    N, K = codes.shape
    i = (codes & 31).long()
    mag = torch.where(i < 16, i * 0.125, torch.where(i < 24, 2.0 + (i - 16) * 0.25, 4.0 + (i - 24) * 0.5)).to(torch.float32)
    val = torch.where((codes & 32) != 0, -mag, mag)
    scale = (scale_exp.to(torch.int32) << 23).view(torch.float32).reshape(N, K // 64, 2)          # the e8m0 byte is the float's exponent field: what the kernels do
    deq = _q6_block_view(val, K) * scale[..., None]
    return deq.reshape(N, K // 64, 2, 4, 8).permute(0, 1, 3, 2, 4).reshape(N, K).to(torch.bfloat16)


def _q6_pack_bits(c):
    """uint8 [..., 32] codes of a lane (element e = 8 u + j) -> uint8 [..., 24]: code e in bits [6 e, 6 e + 6) of the 192, little-endian -- the operand
    order of v_cvt_scalef32_pk32_bf16_fp6 (tests/test_gpu_q6.py's one-hot probe holds the kernels to it)"""
    g = c.reshape(*c.shape[:-1], 8, 4).to(torch.int32)
    w24 = g[..., 0] | (g[..., 1] << 6) | (g[..., 2] << 12) | (g[..., 3] << 18)
    return torch.stack([w24 & 0xFF, (w24 >> 8) & 0xFF, w24 >> 16], dim=-1).to(torch.uint8).reshape(*c.shape[:-1], 24)


def _q6_unpack_bits(b):
    """the inverse of _q6_pack_bits: uint8 [..., 24] -> uint8 [..., 32]"""
    g = b.reshape(*b.shape[:-1], 8, 3).to(torch.int32)
    w24 = g[..., 0] | (g[..., 1] << 8) | (g[..., 2] << 16)
    return torch.stack([w24 & 63, (w24 >> 6) & 63, (w24 >> 12) & 63, w24 >> 18], dim=-1).to(torch.uint8).reshape(*b.shape[:-1], 32)


class PackedQ6(_PackedBlockQuant):
    """A packed weight in the 6-bit (e2m3) stream format of kernels G1q6 / G1sq6 (see pack_weight_q6): `data` uint8 [N * K * 3 / 4 + N * K / 32] = the code
    records, six bits per weight, then the e8m0 scale bytes at byte offset N * K * 3 / 4.  LOSSY: the kernels multiply by dequant(), exactly."""

    weight_stream, REC = LS.STREAMS[2], 1536

    @staticmethod
    def _to_records(c, T):
        c = c.reshape(T, 32, -1, 4, 2, 8).permute(0, 2, 4, 1, 3, 5).reshape(T, -1, 64, 32)          # [t, r, R, u, h, j] -> [t, R, lane = 32 h + r, e = 8 u + j]
        b = _q6_pack_bits(c)                                                                        # [t, R, lane, 24]
        return torch.cat([b[..., :16].reshape(T, -1, 1024), b[..., 16:].reshape(T, -1, 512)], dim=-1)

    @staticmethod
    def _from_records(rec):
        T, R = rec.shape[:2]
        lane = torch.cat([rec[..., :1024].reshape(T, R, 64, 16), rec[..., 1024:].reshape(T, R, 64, 8)], dim=-1)      # [t, R, lane = 32 h + r, 24]
        c = _q6_unpack_bits(lane).reshape(T, R, 2, 32, 4, 8)                                                          # [t, R, h, r, u, j]
        return c.permute(0, 3, 1, 4, 2, 5).reshape(32 * T, 64 * R)                                                    # [t, r, R, u, h, j]

    def dequant(self):
        """bf16 [N, K]: the weight the kernels multiply by, read back from the packed buffer (exact: three mantissa bits times a power of two)"""
        return dequantize_e2m3(self.codes(), self.scale_exp())


def pack_weight_q6(weight, KC, step_major=False, gateup=False):
    """[N, K] bf16 weight -> PackedQ6: quantize_e2m3(weight) in pack_weight(weight, KC, step_major)'s (k-chunk, 32-column tile, k-step, lane, element)
    order at SIX BITS per weight, then the e8m0 scale bytes at byte offset N * K * 3 / 4 of the same buffer -- what sjd_skinny_gemm /
    sjd_skinny_gemm_cols / sjd_gateup_silu stream under SJD_G1_W6_E2M3 (kernels G1q6 / G1sq6, csrc/sjd_gemm_q6.h).  N * K * 3 / 4 + N * K / 32 bytes.
    K granule Q4_GRANULE = 128 (the MXFP4 stream's): K and KC must be multiples of 128 (ValueError otherwise) -- a unit is then whole records and whole
    scale dwords.  The scale blocks are quantize_e2m3's (column, 64-k record, lane half): a private stream format, not an interchange format.
    Byte layout: the k-steps of a unit (chunk c, tile t) travel in RECORDS of four -- record R (1536 B) = 64 lanes x 16 B, then 64 lanes x 8 B: bytes
    0..15 and 16..23 of the lane's 24, which hold its 32 codes (lane l = 32 h + r, element e = 8 u + j = the code of q[32 t + r][k0 + 64 R + 16 u + 8 h + j])
    in bits [6 e, 6 e + 6), little-endian.  Tile-major: a unit is S * 384 contiguous bytes; step_major: a chunk holds record 0 of every tile, record 1 of
    every tile, ...  A chunk starts at byte k0 * N * 3 / 4.  Scales: per unit and trip q of two records 128 bytes = 32 columns x 4 bytes (byte 2 i + h: record
    2 q + i, lane half h), the trips laid out like the records; a chunk's scales start at scale byte k0 * N / 32.
    gateup=True: `weight` is [Wg; Wu] packed with KC = K / 2 for sjd_gateup_silu.
    stats: rel_rms_error (RMS of w - dequant over RMS of w), scale_exp_min / scale_exp_max (log2 of the smallest / largest block scale)."""
    return _pack_block_quant(PackedQ6, "pack_weight_q6", quantize_e2m3, dequantize_e2m3, weight, KC, step_major, gateup)


def _same_16bit_type(x, w_packed, what):
    """the kernels read the packed records as the activation's type: bf16 rows against fp16 records (or the reverse) would multiply garbage"""
    wd = getattr(w_packed, "dtype", None)
    if {x.dtype, wd} == {torch.bfloat16, torch.float16}:
        raise L.SjdLibraryError(f"{what}: activation {x.dtype} against a weight packed from {wd}: pack the weight in the activation's type")


def _prows(M):
    """row padding of the G1 partial planes: whole 32-row MFMA tiles (M <= 256: up to eight prompts per forward)"""
    return ((int(M) + 31) // 32) * 32


def streamed(w_packed):
    """(stream, records, dtype flag) of a weight: a copy of a row of LS.STREAMS, else (None, the weight itself, 0) -- pack_weight's tensor, or a PackedZ"""
    s = getattr(w_packed, "weight_stream", None)
    return (None, w_packed, 0) if s is None else (s, w_packed.data, getattr(L, s.flag))


def skinny_gemm(x, w_packed, N, K, KC, waves=4, step_major=False):
    """x [M <= LS.WINDOW_MAX_ROWS, K] bf16/fp16 -> Partials([n_chunks, 32 * ceil(M / 32), N] fp32).  waves = column tiles per workgroup: 1..16 up to 64 rows,
    <= 8 up to 128 rows; above that (bf16 or fp16, uncompressed packing) kernel G1w takes LS.WIDE_TILES.  A copy of a row of LS.STREAMS (bf16; K and KC
    multiples of its granule): up to 64 rows on G1q / G1q4 / G1q6 (min(KC, K) <= LS.CHUNK_CAP_32ROW up to 32 rows, <= LS.CHUNK_CAP_64ROW above); 65 rows and more
    on G1wq / G1wq4 with LS.WIDE_TILES (not 2 at 65..96 rows), no form there for e2m3 -- the planes of the same call on pack_weight(w_packed.dequant(), KC, step_major), bit for bit."""
    M = x.shape[0]
    assert x.is_contiguous() and x.shape[1] == K and w_packed.numel() == N * K
    _same_16bit_type(x, w_packed, "skinny_gemm")
    if isinstance(w_packed, Packed):
        return skinny_gemm_cols(x, w_packed, N, K, KC, 0, N, waves, step_major)
    nc = (K + KC - 1) // KC
    out = torch.empty(nc, _prows(M), N, dtype=torch.float32, device=x.device)
    L.check(L.load().sjd_skinny_gemm(_ptr(x), _ptr(w_packed), _ptr(out), M, N, K, KC, waves, int(step_major), _dtype_code(x.dtype), _stream()), "sjd_skinny_gemm")
    return Partials(out, nc, N)


def prefill_gemm(x, w_packed, N, K, row_scale=None, KC=None, step_major=None):
    """G1p: x [M, K] bf16 (any M >= 1) -> y [M, N] bf16 = round16(row_scale[m] * x @ W^T) over a packed copy as it is packed -- a copy of a stream that has
    "prefill" (LS.STREAMS: PackedQ8 / PackedQ4; the chunk and record order they carry) or the plain pack_weight tensor (which carries neither: pass KC and
    step_major).  row_scale: fp32 [M] or None; it multiplies the finished fp32 sum in front of the one rounding (the folded RMSNorm of F2 / F3).  A workgroup runs LS.PREFILL_ROW_BLOCK rows x the whole
    of K: no split-K planes.  A quantised copy gives the bits of prefill_gemm on pack_weight(w_packed.dequant(), KC, step_major); a row's output does not
    depend on M or on its position.  K and KC multiples of the stream's granule (plain: 32), N a multiple of 32, bf16: the library refuses the rest before
    any launch ("unsupported configuration")."""
    M = x.shape[0]
    s, data, flag = streamed(w_packed)
    if s is not None and "prefill" not in s.has:
        raise ValueError(f"prefill_gemm: the {s.names[0]} stream (Packed{s.tag.upper()}) has no prefill kernel; prefill from the 16-bit weights")
    assert x.dim() == 2 and x.is_contiguous() and x.shape[1] == K and w_packed.numel() == N * K
    if s is not None:
        assert (w_packed.N, w_packed.K) == (N, K) and KC in (None, w_packed.KC) and step_major in (None, w_packed.step_major)
        KC, step_major = w_packed.KC, w_packed.step_major
    else:
        assert isinstance(w_packed, torch.Tensor) and KC is not None and step_major is not None, "a plain packing carries neither its chunk nor its record order"
    _same_16bit_type(x, w_packed, "prefill_gemm")
    if row_scale is not None:
        assert row_scale.dtype == torch.float32 and row_scale.is_contiguous() and row_scale.shape == (M,) and row_scale.device == x.device
    y = torch.empty(M, N, dtype=x.dtype, device=x.device)
    L.check(L.load().sjd_prefill_gemm(_ptr(x), _ptr(data), _ptr(y), M, N, K, int(KC), int(step_major), _dtype_code(x.dtype) | flag, _ptr(row_scale), _stream()),
            "sjd_prefill_gemm")
    return y


_REDUCE_TICKETS = {}


def skinny_gemm_reduce_ok(M, N, K, KC, waves, device):
    """shapes sjd_skinny_gemm_reduce serves: a <= 32-row window, whole 512-column output slices, power-of-two waves that tile them, at most
    16 K chunks, enough workgroups per slice for its 32 rows, and the whole launch resident at once (its workgroups wait for each other: one
    workgroup per CU is the safe bound)"""
    n_chunks = (K + KC - 1) // KC
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    if not (M <= 32 and N % 512 == 0 and waves in (2, 4, 8) and (N // 32) % waves == 0 and n_chunks <= 16 and (N // 32 // waves) * n_chunks <= cus):
        return False
    total = (16 // waves) * n_chunks          # workgroups that share a 512-column slice; each reduces ceil(32 / total) rows, two waves per row
    return 2 * -(-32 // total) <= waves


def skinny_gemm_reduce(x, w_packed, N, K, KC, h, waves=8, step_major=False):
    """G1 with F1r as its tail: h [M, N] += dtype(x @ W^T) IN PLACE; returns the per-512-column-slice sums of h^2 [N / 512, 32] fp32 (the
    `sumsq` of a row_norm) -- bit-identical to residual_sumsq(h, skinny_gemm(x, ...)) in one launch (sjd_skinny_gemm_reduce)."""
    M = x.shape[0]
    assert x.is_contiguous() and x.shape[1] == K and w_packed.numel() == N * K and h.is_contiguous() and tuple(h.shape) == (M, N) and h.dtype == x.dtype
    nc = (K + KC - 1) // KC
    dev = x.device
    tk = _REDUCE_TICKETS.get(dev)
    if tk is None or tk.numel() < (N // 512) * 32:
        tk = _REDUCE_TICKETS[dev] = torch.zeros(max(64, N // 512) * 32, dtype=torch.int32, device=dev)     # re-arms itself; launches of one stream never overlap
    ws = torch.empty(nc, 32, N, dtype=torch.float32, device=dev)
    sumsq = torch.empty(N // 512, 32, dtype=torch.float32, device=dev)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    L.check(L.load_exp().sjd_skinny_gemm_reduce(_ptr(x), _ptr(w_packed), _ptr(ws), _ptr(h), _ptr(sumsq), _ptr(tk), M, N, K, KC, waves, int(step_major),
                                            _dtype_code(x.dtype), int(cus), _stream()), "sjd_skinny_gemm_reduce")
    return sumsq


def reduce_timeouts():
    """waits of sjd_skinny_gemm_reduce launches that were abandoned since the library was loaded (0 on a healthy, unshared device)"""
    return int(L.load_exp().sjd_reduce_timeouts())


_PREFETCH_SINK = {}


def weight_prefetch(w_packed, blocks=128, nbytes=None):
    """Read `w_packed` (a G1 packed weight) on the CURRENT stream and discard it: pulls the lines into the Infinity Cache ahead of
    the G1 launch that streams them (call it on a side stream forked from the forward, see ChameleonBackbone._prefetch)."""
    if isinstance(w_packed, Packed):
        w_packed = w_packed.data
    dev = w_packed.device
    sink = _PREFETCH_SINK.get(dev)
    if sink is None:
        sink = _PREFETCH_SINK[dev] = torch.zeros(4, dtype=torch.int32, device=dev)
    nb = int(nbytes) if nbytes is not None else w_packed.numel() * w_packed.element_size()
    L.check(L.load_exp().sjd_weight_prefetch(_ptr(w_packed), nb, int(blocks), _ptr(sink), _stream()), "sjd_weight_prefetch")


_ENGINE_TIMEOUTS_SEEN = 0


def skinny_gemm_engine(x, w_packed, n_wg=None, col0=0, n_cols=None, check=True):
    """G1z in the loader / consumer form (round 5 stage A, csrc/sjd_gemm_engine.h): x [M <= 32, K] bf16, w_packed a tile-major PackedZ ->
    Partials([n_chunks, 32, n_cols]) bit-identical to skinny_gemm_cols on the same packing.  n_wg: persistent workgroups (default: the largest
    multiple of the K-chunk count that fits the device's CUs).  check (default): synchronise and raise if a bounded LDS poll of the kernel
    gave up -- it then went on with wrong partials; check=False inside a hipGraph capture / a timed loop: call engine_timeouts()
    yourself afterwards."""
    assert w_packed.n_raw == 0, "the engine kernel does not know raw units (round 6)"
    assert isinstance(w_packed, PackedZ) and not w_packed.step_major and x.dtype == torch.bfloat16 and x.is_contiguous() and x.shape[1] == w_packed.K
    M, K, KC = x.shape[0], w_packed.K, w_packed.KC
    n = (w_packed.N - col0) if n_cols is None else n_cols
    nc = (K + KC - 1) // KC
    if n_wg is None:
        cus = torch.cuda.get_device_properties(x.device).multi_processor_count
        n_wg = max(nc, min(cus // nc, n // 32) * nc)
    out = torch.empty(nc, 32, n, dtype=torch.float32, device=x.device)
    L.check(L.load_exp().sjd_skinny_gemm_engine_z(_ptr(x), _ptr(w_packed.data), _ptr(w_packed.exc), w_packed.cap, _ptr(out), M, n, K, KC, _dtype_code(x.dtype),
                                             w_packed.N, col0 // 32, int(n_wg), _stream()), "sjd_skinny_gemm_engine_z")
    if check and not torch.cuda.is_current_stream_capturing():
        global _ENGINE_TIMEOUTS_SEEN
        torch.cuda.current_stream().synchronize()
        n_to = engine_timeouts()
        if n_to > _ENGINE_TIMEOUTS_SEEN:
            _ENGINE_TIMEOUTS_SEEN = n_to
            raise RuntimeError(f"sjd_skinny_gemm_engine_z: {n_to} bounded LDS poll(s) gave up -- the partials of this launch are wrong")
    return Partials(out, nc, n)


def engine_timeouts():
    """bounded LDS polls of sjd_skinny_gemm_engine_z that gave up since the library was loaded.  The engine kernel (round-5 experiment) never
    hangs: a poll that times out goes on with WRONG partials -- skinny_gemm_engine(check=True), the default, raises when the count moved."""
    return int(L.load_exp().sjd_engine_timeouts())


def l2_head(w_packed, M, waves=None, head_pairs=8, gateup=False, col0=0, n_cols=None):
    """-> _lib.L2Head: the first `head_pairs` record pairs of every unit of the G1z (or, gateup=True, G1sz) launch that will stream `w_packed`
    (a PackedZ) for an M-row window with `waves` waves per workgroup -- what a glue launch in front of it pulls into the L2 (round 5 experiment).
    waves: REQUIRED for the projection kind (the launch's column tiles per workgroup, G1_CFG[name][1]); the gate|up kind describes the
    512-thread G1sz launch of up to 64 rows (I / 64 workgroups) -- the 65..128-row window runs G1 + F3 instead and has no such descriptor."""
    assert isinstance(w_packed, PackedZ)
    if gateup:
        if M > 64:
            raise ValueError("l2_head(gateup=True) describes the fused G1sz launch (<= 64 rows); taller windows run G1z + F3: use the projection kind")
    elif waves is None:
        raise ValueError("l2_head: `waves` (column tiles per workgroup of the G1z launch, G1_CFG[name][1]) is required for a projection")
    h = L.L2Head()
    if gateup:
        L.check(L.load_exp().sjd_l2_head_gateup_z(ctypes.byref(h), _ptr(w_packed.data), M, w_packed.N // 2, w_packed.K, int(w_packed.step_major), int(head_pairs)),
                "sjd_l2_head_gateup_z")
    else:
        n = w_packed.N - col0 if n_cols is None else n_cols
        L.check(L.load_exp().sjd_l2_head_gemm_z(ctypes.byref(h), _ptr(w_packed.data), M, n, w_packed.K, w_packed.KC, int(waves), int(w_packed.step_major), w_packed.N,
                                           col0 // 32, int(head_pairs)), "sjd_l2_head_gemm_z")
    h._keep = w_packed           # the descriptor holds a raw address
    return h


def l2_head_bytes(head):
    return int(L.load_exp().sjd_l2_head_bytes(ctypes.byref(head)))


def weight_prefetch_head(head, blocks=256):
    """the L2 head pull as a launch of its own (bench aid; the product hosts it in F1r / F2)"""
    L.check(L.load_exp().sjd_weight_prefetch_head(ctypes.byref(head), int(blocks), _stream()), "sjd_weight_prefetch_head")


def xcc_map(gx, gy=1, device="cuda:0"):
    """XCC_ID of every workgroup of a (gx, gy) launch -> int32 [gy, gx]"""
    out = torch.full((gy, gx), -1, dtype=torch.int32, device=device)
    L.check(L.load_exp().sjd_debug_xcc_map(_ptr(out), gx, gy, _stream()), "sjd_debug_xcc_map")
    return out


def _raw_units(w_packed, gateup=False):
    """PackedZ -> ctypes pointer to the sjd_raw_units of its verbatim units (or None): the (chunk, tile) table of the plane kernels, or with
    gateup=True the gate-tile table of the raw (gate, up) pairs.  Where they are multiplied is the C entry point's business."""
    index, n = (w_packed.raw_tiles, w_packed.n_raw_pairs) if gateup else (w_packed.raw_index, w_packed.n_raw)
    if not n:
        return None
    ru = L.RawUnits()
    ru.records, ru.index, ru.n = w_packed.raw_data.data_ptr(), index.data_ptr(), n
    return ctypes.pointer(ru)


def skinny_gemm_cols(x, w_packed, N_packed, K, KC, col0, n_cols, waves=8, step_major=True):
    """G1 over the vocabulary columns [col0, col0 + n_cols) (32-aligned) of a weight packed with N_packed columns -> Partials [n_chunks, R, n_cols].
    Row counts and `waves` per packing as skinny_gemm (PackedZ: up to LS.Z_MAX_ROWS rows; a row of LS.STREAMS: where it has a wide kernel)."""
    M = x.shape[0]
    assert x.is_contiguous() and x.shape[1] == K and w_packed.numel() == N_packed * K and col0 % 32 == 0 and n_cols % 32 == 0
    nc = (K + KC - 1) // KC
    out = torch.empty(nc, _prows(M), n_cols, dtype=torch.float32, device=x.device)
    if isinstance(w_packed, PackedZ):
        assert (w_packed.KC, w_packed.step_major) == (KC, bool(step_major)) and x.dtype == torch.bfloat16
        L.check(L.load().sjd_skinny_gemm_z(_ptr(x), _ptr(w_packed.data), _ptr(w_packed.exc), w_packed.cap, _ptr(out), M, n_cols, K, KC, waves, int(step_major),
                                          _dtype_code(x.dtype), N_packed, col0 // 32, _raw_units(w_packed), _stream()), "sjd_skinny_gemm_z")
        return Partials(out, nc, n_cols)
    _same_16bit_type(x, w_packed, "skinny_gemm_cols")
    s, records, flag = streamed(w_packed)
    if s is not None:          # G1q / G1q4 / G1q6 and their wide forms: the scales ride behind the records of the same buffer
        assert (w_packed.N, w_packed.step_major) == (N_packed, bool(step_major)) and w_packed.reads_as(KC)
    L.check(L.load().sjd_skinny_gemm_cols(_ptr(x), _ptr(records), _ptr(out), M, n_cols, K, KC, waves, int(step_major), _dtype_code(x.dtype) | flag,
                                         N_packed, col0 // 32, _stream()), "sjd_skinny_gemm_cols" + (f" ({s.names[0]} weights)" if s else ""))
    return Partials(out, nc, n_cols)


def skinny_gemm_z_wide(x, w_packed, tiles, col0=0, n_cols=None):
    """EXPERIMENTAL (libsjd_hip_exp.so; late round 6): kernel G1w over the 12-bit stream -- x [33..256, K] bf16, w_packed a PackedZ, `tiles` = 2, 3, 4, 6 or 8
    column tiles per workgroup -> Partials bit-identical to skinny_gemm_cols on the same packing (raw units included).  Measured slower
    than the product's kernels: kept for its test and tools/g1wz_sweep.py."""
    assert isinstance(w_packed, PackedZ) and x.dtype == torch.bfloat16 and x.is_contiguous() and x.shape[1] == w_packed.K
    M, K, KC = x.shape[0], w_packed.K, w_packed.KC
    n = (w_packed.N - col0) if n_cols is None else n_cols
    nc = (K + KC - 1) // KC
    out = torch.empty(nc, _prows(M), n, dtype=torch.float32, device=x.device)
    L.check(L.load_exp().sjd_skinny_gemm_z_wide(_ptr(x), _ptr(w_packed.data), _ptr(w_packed.exc), w_packed.cap, _ptr(out), M, n, K, KC, int(tiles),
                                               int(w_packed.step_major), w_packed.N, col0 // 32, _raw_units(w_packed), _stream()), "sjd_skinny_gemm_z_wide")
    return Partials(out, nc, n)


class HeadOut:
    """What a backbone hands to K2 instead of logits: the lm_head split-K partials of the window (cond rows [0, n), uncond rows
    [urow_off, urow_off + n)), their vocabulary column window and the folded final-norm row statistics."""

    def __init__(self, part: Partials, col0, urow_off, dtype, row_norm=None):
        self.part, self.col0, self.urow_off, self.dtype, self.row_norm = part, int(col0), int(urow_off), dtype, row_norm


def logits_to_probs_sample_part(head: HeadOut, guidance, params: DeviceBlob, noise, probs_out, tokens_out_ptr, dbg=None, amax_out_ptr=None,
                                row0=0, urow_off=None, zero_state=None):
    """K2 reading the unmaterialised output head (see sjd_head_partials in include/sjd_hip.h).  dbg: optional fp32 [2, rows, V] that
    receives the logits K2 derived (cond, uncond) -- observers only.  row0 / urow_off: this launch's cond rows start at partial row
    `row0` and its uncond rows `urow_off` rows further (several prompts share one head launch: SJDBatchEngine).  guidance: a float, or -- for a
    head wide enough for K2a only -- ONE device float32 (a 1-element tensor) that K2a reads at run time (sjd_head_combine_g)."""
    max_rows, V = probs_out.shape
    hp = _head_partials(head, max_rows, V, probs_out.device, dbg, row0, urow_off, zero_state)
    p = head.part
    assert noise is None or (noise.dtype == torch.float32 and noise.is_contiguous() and noise.shape[-1] == V)
    assert probs_out.is_contiguous()
    if head_combine_ok(hp):
        # K2a (round 4): a WIDE head window (Emu3: 32768 columns x 2 planes x 2 rows = 524 KB per row) is combined into guided scores on the whole
        # chip first; K2 then reads ONE plane per row -- bit-identical scores (sjd_head_combine in include/sjd_hip.h)
        z = torch.empty(max_rows, p.N, dtype=torch.float32, device=probs_out.device)
        if isinstance(guidance, torch.Tensor):
            if not (guidance.dtype == torch.float32 and guidance.numel() == 1 and guidance.device == probs_out.device):
                raise ValueError(f"guidance scale in device memory: one float32 on {probs_out.device}, got {tuple(guidance.shape)} {guidance.dtype} "
                                 f"on {guidance.device}")
            L.check(L.load().sjd_head_combine_g(ctypes.byref(hp), _ptr(guidance), max_rows, V, params.ptr, _ptr(z), _stream()), "sjd_head_combine_g")
            guidance = 0.0                  # (K2 below reads ONE plane, no uncond row: it combines nothing)
        else:
            L.check(L.load().sjd_head_combine(ctypes.byref(hp), float(guidance), max_rows, V, params.ptr, _ptr(z), _stream()), "sjd_head_combine")
        h2 = L.HeadPartials()
        h2.part, h2.n_chunks, h2.row_stride, h2.chunk_stride = z.data_ptr(), 1, p.N, max_rows * p.N
        h2.col0, h2.n_cols, h2.urow_off, h2.round_dtype = hp.col0, hp.n_cols, 0, 2            # SJD_DTYPE_F32: no rounding, no scale, no uncond row
        h2.zero_state = hp.zero_state
        hp = h2
    if isinstance(guidance, torch.Tensor):
        raise ValueError("a guidance scale in device memory is served for heads wide enough for K2a (sjd_head_combine_g) and by the slot launch "
                         "(logits_to_probs_sample_part_slots); the one-slot K2 over a narrow head takes a float")
    L.check(L.load().sjd_logits_to_probs_sample_part(ctypes.byref(hp), float(guidance), max_rows, V, params.ptr, _ptr(noise), _ptr(probs_out),
                                                    tokens_out_ptr, amax_out_ptr, _stream()), "sjd_logits_to_probs_sample_part")


def _head_partials(head, max_rows, V, device, dbg=None, row0=0, urow_off=None, zero_state=None):
    """-> _lib.HeadPartials over `head` (a HeadOut) for a K2 launch whose cond rows start at partial row `row0`"""
    p = head.part
    hp = L.HeadPartials()
    hp.part, hp.n_chunks = p.data.data_ptr() + 4 * int(row0) * p.N, p.n_chunks
    hp.row_stride, hp.chunk_stride = p.N, p.data.shape[1] * p.N
    hp.col0, hp.n_cols, hp.urow_off = head.col0, p.N, head.urow_off if urow_off is None else int(urow_off)
    hp.round_dtype = _dtype_code(head.dtype)
    if head.row_norm is not None:
        sumsq, hidden, eps = head.row_norm
        hp.row_sumsq, hp.slices, hp.prows, hp.inv_hidden, hp.eps = sumsq.data_ptr() + 4 * int(row0), sumsq.shape[0], sumsq.shape[1], 1.0 / float(hidden), float(eps)
    if dbg is not None:
        assert dbg.dtype == torch.float32 and dbg.is_contiguous() and dbg.shape[0] >= 1 and dbg.shape[2] == V and dbg.shape[1] >= max_rows
        hp.dbg_c = dbg[0].data_ptr()
        if dbg.shape[0] >= 2:              # (one plane: a batch without CFG -- there is no uncond row to observe)
            hp.dbg_u = dbg[1].data_ptr()
    if zero_state is not None:         # int32 [max_rows, 2] that belongs to THIS probs_out buffer (see sjd_head_partials::zero_state)
        assert zero_state.dtype == torch.int32 and zero_state.is_contiguous() and zero_state.shape == (max_rows, 2) and zero_state.device == device
        hp.zero_state = zero_state.data_ptr()
    return hp


def slots_of(params: "BlobArray", state: "BlobArray", probs, zero_state, scratch, n_batch, dbg=None):
    """-> _lib.Slots for the *_slots launches of a continuous batch: params / state BlobArrays (one blob per slot), probs [P, 2, L, V] fp32,
    zero_state [P, 2, L, 2] int32, scratch [P, >= V] fp32, dbg None or [P * n_batch, L, V] fp32 -- all contiguous (the strides below)."""
    P, two, Lw, V = probs.shape
    assert two == 2 and probs.is_contiguous() and probs.dtype == torch.float32 and len(params.blobs) == P and len(state.blobs) == P
    assert zero_state.is_contiguous() and zero_state.dtype == torch.int32 and tuple(zero_state.shape) == (P, 2, Lw, 2)
    assert scratch.is_contiguous() and scratch.dtype == torch.float32 and scratch.shape[0] == P and scratch.shape[1] >= V
    sl = L.Slots()
    sl.n_slots, sl.head_rows = P, n_batch * Lw
    sl.params_stride, sl.state_stride = params.nbytes, state.nbytes
    sl.probs_stride, sl.zero_state_stride, sl.scratch_stride = 2 * Lw * V, 2 * Lw * 2, scratch.shape[1]
    _, sl.mirror_stride = state.mirror_array()
    if dbg is not None:
        assert dbg.is_contiguous() and dbg.dtype == torch.float32 and tuple(dbg.shape) == (P * n_batch, Lw, V)
        sl.dbg_stride = n_batch * Lw * V
    return sl


def reguess_slots(slots, params: "BlobArray", state: "BlobArray", input_ids_out, pos_offset, positions_out, n_batch):
    """K5 of every slot in one launch: input_ids_out / positions_out [P * n_batch, L] int64, pos_offset [P * n_batch] int64"""
    B, max_rows = input_ids_out.shape
    assert B == slots.n_slots * n_batch and input_ids_out.dtype == torch.int64 and input_ids_out.is_contiguous()
    assert positions_out.dtype == torch.int64 and positions_out.is_contiguous() and tuple(positions_out.shape) == (B, max_rows)
    assert pos_offset.dtype == torch.int64 and pos_offset.is_contiguous() and pos_offset.numel() == B
    L.check(L.load().sjd_reguess_slots(params.ptr, state.ptr, _ptr(input_ids_out), n_batch, max_rows, _ptr(pos_offset), _ptr(positions_out),
                                      ctypes.byref(slots), _stream()), "sjd_reguess_slots")


def head_slots_ok(head: "HeadOut"):
    """the *_slots K2 launch reads the head's planes itself: a head wide enough for K2a (Emu3) keeps the per-slot launches"""
    return not head_combine_ok(_head_partials(head, 0, 0, None))      # (the predicate logits_to_probs_sample_part itself decides with)


def logits_to_probs_sample_part_slots(slots, head: "HeadOut", guidance, params: "BlobArray", probs, cur, tokens_field, amax_field, state: "BlobArray",
                                      zero_state, n_batch, dbg=None):
    """K2 of every slot in one launch (see logits_to_probs_sample_part): slot s reads the cond rows [s * n_batch * L, ...) of the shared head launch
    and its uncond rows L further (n_batch 2), writes probs[s, cur] and the int64 rows `tokens_field` / `amax_field` (names of sjd_state fields,
    amax_field may be None) of its state.  guidance: a float for every slot (sjd_logits_to_probs_sample_part_slots, as ever), or a device float32
    tensor of n_slots values, slot s combining with guidance[s] (sjd_logits_to_probs_sample_part_slots_g: the launch reads the array, so a
    captured graph follows a later change of its contents)."""
    P, _, max_rows, V = probs.shape
    hp = _head_partials(head, max_rows, V, probs.device, None, 0, max_rows if n_batch > 1 else 0, zero_state[0, cur])
    if dbg is not None:
        hp.dbg_c = dbg[0].data_ptr()
        if n_batch > 1:
            hp.dbg_u = dbg[1].data_ptr()
    s0 = state.blobs[0]
    if isinstance(guidance, torch.Tensor):
        if not (guidance.dtype == torch.float32 and guidance.is_contiguous() and guidance.numel() == slots.n_slots and guidance.device == probs.device):
            raise ValueError(f"per-slot guidance scales: a contiguous float32 tensor of {slots.n_slots} values on {probs.device}, got "
                             f"{tuple(guidance.shape)} {guidance.dtype} on {guidance.device}")
        L.check(L.load().sjd_logits_to_probs_sample_part_slots_g(ctypes.byref(hp), _ptr(guidance), max_rows, V, params.ptr, _ptr(probs[0, cur]),
                                                                s0.field_ptr(tokens_field), s0.field_ptr(amax_field) if amax_field else None,
                                                                ctypes.byref(slots), _stream()), "sjd_logits_to_probs_sample_part_slots_g")
        return
    L.check(L.load().sjd_logits_to_probs_sample_part_slots(ctypes.byref(hp), float(guidance), max_rows, V, params.ptr, _ptr(probs[0, cur]),
                                                          s0.field_ptr(tokens_field), s0.field_ptr(amax_field) if amax_field else None,
                                                          ctypes.byref(slots), _stream()), "sjd_logits_to_probs_sample_part_slots")


def verify_accept_slots(slots, params: "BlobArray", state: "BlobArray", probs, cur, scratch):
    """K4 of every slot in one launch; every state is also written into its pinned host mirror (BlobArray.mirror_array / wait_mirror)"""
    P, _, max_rows, V = probs.shape
    mptr, _ = state.mirror_array()
    L.check(L.load().sjd_verify_accept_slots(params.ptr, state.ptr, _ptr(probs[0, cur]), _ptr(probs[0, 1 - cur]), _ptr(scratch), max_rows, V, mptr,
                                            ctypes.byref(slots), _stream()), "sjd_verify_accept_slots")


_HEAD_COMBINE_MIN_COLS = int(os.environ.get("SJD_HEAD_COMBINE_MIN_COLS", "16384"))     # (a huge value switches K2a off: A/B aid)


def head_combine_ok(hp):
    """K2a serves heads whose window is wide enough for the extra launch to pay (one CU pulls a row's planes at 16-40 GB/s: Emu3's 32768 columns
    yes, Lumina's 8192 no) and whose layout its float4 accesses need"""
    return (hp.n_cols >= _HEAD_COMBINE_MIN_COLS and hp.n_cols % 4 == 0 and hp.row_stride % 4 == 0 and hp.chunk_stride % 4 == 0 and
            (hp.part or 0) % 16 == 0)


def _part_args(delta):
    if isinstance(delta, Partials):
        return None, _ptr(delta.data), delta.n_chunks
    return delta, None, 0


def add_rmsnorm(h, delta, weight, eps):
    """h [T, hidden] is updated in place (h += delta) when delta is given (a tensor, or the Partials of a G1 projection);
    returns weight * norm(h)."""
    T, hidden = h.shape
    d, part, nc = _part_args(delta)
    assert h.is_contiguous() and (d is None or d.is_contiguous()) and weight.is_contiguous()
    y = torch.empty_like(h)
    L.check(L.load().sjd_add_rmsnorm(_ptr(h), _ptr(d), _ptr(weight), _ptr(y), T, hidden, float(eps), _dtype_code(h.dtype),
                                    part, nc, _stream()), "sjd_add_rmsnorm")
    return y


def add_rmsnorm_post(h, delta, weight, eps):
    """F1 in the swin-norm order (ChameleonSwinDecoderLayer): h [T, hidden] += dtype(weight * dtype(rmsnorm(delta))) in place, delta = a
    sublayer output (a tensor, or the Partials of a G1 projection); returns h, which is the next projection's input as it stands."""
    T, hidden = h.shape
    d, part, nc = _part_args(delta)
    assert delta is not None and h.is_contiguous() and (d is None or d.is_contiguous()) and weight.is_contiguous()
    L.check(L.load().sjd_add_rmsnorm(_ptr(h), _ptr(d), _ptr(weight), None, T, hidden, float(eps), _dtype_code(h.dtype) | L.F1_POST_NORM,
                                    part, nc, _stream()), "sjd_add_rmsnorm")
    return h


def _row_norm(row_norm):
    """(sumsq [slices, R] fp32, hidden, eps) -> ctypes pointer to an sjd_row_norm (or None)"""
    if row_norm is None:
        return None
    sumsq, hidden, eps = row_norm
    assert sumsq.dtype == torch.float32 and sumsq.is_contiguous() and sumsq.dim() == 2
    rn = L.RowNorm()
    rn.sumsq, rn.slices, rn.hidden, rn.eps = sumsq.data_ptr(), sumsq.shape[0], int(hidden), float(eps)
    return ctypes.pointer(rn)


def qknorm_rope_append(qkv, k_cache, v_cache, qn_w, qn_b, kn_w, kn_b, inv_freq, positions, B, n, H, H_kv, D, params, kv_len,
                       kv_scale=(1.0, 1.0), dtype=None, row_norm=None, qk_shards=1, rope_table=None, head_pad=None, one_head=False):
    """qkv [B*n, (H+2Hkv)*D] (tensor or G1 Partials) -> q [B,n,H,D]; k/v rows are written into k_cache/v_cache [B,Hkv,S,D].
    An fp8 cache (dtype FP8) receives fp8(x / scale) with kv_scale = (k, v); `dtype` = the activation dtype (needed with Partials
    into an fp8 cache, where no 16-bit tensor is around to tell).  row_norm = (sumsq, hidden, eps): the projection ran on the
    un-normalised residual stream with the norm gain folded into its weight; the row scale is applied here (folded-norm path).
    qk_shards = mp > 1: the QK-norm gains / biases are [mp, D] (model_parallel_size mp), head h of q uses row h // (H // mp), of k h // (Hkv // mp).
    rope_table: LlamaGen's interleaved 2-D rotary (SJD_F2_ROPE_TABLE) from an fp32 (cos, sin) table [S_rows >= S_max, D/2, 2], row p serving
    position p; inv_freq is ignored then and the QK-norm arguments must be None.
    head_pad = 128 (SJD_F2_HEAD_PAD128; with rope_table and D = 100 only): the source heads are D = 100 wide, q comes back [B,n,H,128] and the
    caches are [B,Hkv,S,128]; the pad columns of every written row are written as zeros.
    one_head (SJD_F2_ONE_HEAD): above 64 rows of Partials, one head per wave in place of four -- the same bits (parity tests and A/B timing)."""
    t, part, nc = _part_args(qkv)
    assert (t is None or t.is_contiguous()) and positions.is_contiguous() and positions.dtype == torch.int64
    mode = L.F2_ONE_HEAD if one_head else 0
    if rope_table is not None:
        assert rope_table.dtype == torch.float32 and rope_table.is_contiguous() and rope_table.shape[1:] == (D // 2, 2)
        assert rope_table.shape[0] >= k_cache.shape[2], "the rotary table needs a row per cache position"
        inv_freq, mode = rope_table, mode | L.F2_ROPE_TABLE
    DS = D
    if head_pad is not None and head_pad != D:
        assert rope_table is not None and (D, head_pad) == (100, 128), "head_pad: head_dim 100 stored 128 wide, table rotary only"
        assert k_cache.shape[3] == head_pad and v_cache.shape[3] == head_pad, "head_pad: the caches are [B, Hkv, S, 128]"
        DS, mode = head_pad, mode | L.F2_HEAD_PAD128
    assert inv_freq.dtype == torch.float32 and inv_freq.is_contiguous()
    fp8 = k_cache.dtype == FP8
    act = dtype or (t.dtype if t is not None else k_cache.dtype)
    assert act in (torch.bfloat16, torch.float16)
    q = torch.empty(B, n, H, DS, dtype=act, device=k_cache.device)
    L.check(L.load().sjd_qknorm_rope_append_ex(_ptr(t), _ptr(q), _ptr(k_cache), _ptr(v_cache), _ptr(qn_w), _ptr(qn_b), _ptr(kn_w),
                                              _ptr(kn_b), _ptr(inv_freq), _ptr(positions), B, n, H, H_kv, D, k_cache.shape[2],
                                              _dtype_code(act) | (int(qk_shards) << L.QKN_SHARDS_SHIFT if qk_shards > 1 else 0) | mode, int(fp8),
                                              float(kv_scale[0]), float(kv_scale[1]), _row_norm(row_norm),
                                              params.ptr if params is not None else None, int(kv_len), part, nc, _stream()),
            "sjd_qknorm_rope_append")
    return q


def fused_attention_ok(B, n, H, H_kv, D, cache_dtype):
    """shapes kernel K1F serves (everything else: F2 + K1 + combine)"""
    return H == H_kv and D == 128 and n <= 16 and B * n <= 32 and cache_dtype in (torch.bfloat16, torch.float16)


def qkv_attention_fused(qkv_part, k_cache, v_cache, qn_w, qn_b, kn_w, kn_b, inv_freq, positions, B, n, H, D, params, kv_len, key_start,
                        row_norm=None, dtype=None, n_split=1, workspace=None):
    """K1F: G1 Partials of the q|k|v projection -> attention output [B, n, H, D]; the window's k / v rows are appended to
    k_cache / v_cache [B, H, S, D] on the way (QK-norm + RoPE as in qknorm_rope_append).  n_split > 1 (K1Fs): the key tiles of a (batch,
    head) split over n_split workgroups + the split combine; workspace = attention_workspace(B, H, n, D, n_split)."""
    if n_split > 1:
        assert isinstance(qkv_part, Partials) and qkv_part.N == 3 * H * D and qkv_part.data.shape[1] == 32 and workspace is not None
        act = dtype or k_cache.dtype
        out = torch.empty(B, n, H, D, dtype=act, device=k_cache.device)
        L.check(L.load_exp().sjd_qkv_attention_fused_split(_ptr(qkv_part.data), qkv_part.n_chunks, _ptr(k_cache), _ptr(v_cache), _ptr(out), _ptr(qn_w),
                                                      _ptr(qn_b), _ptr(kn_w), _ptr(kn_b), _ptr(inv_freq), _ptr(positions), B, n, H, D,
                                                      k_cache.shape[2], _dtype_code(act), _row_norm(row_norm), _ptr(key_start),
                                                      params.ptr if params is not None else None, int(kv_len), int(n_split), _ptr(workspace),
                                                      _stream()), "sjd_qkv_attention_fused_split")
        return out
    assert isinstance(qkv_part, Partials) and qkv_part.N == 3 * H * D and qkv_part.data.shape[1] == 32
    assert positions.is_contiguous() and positions.dtype == torch.int64 and inv_freq.dtype == torch.float32
    assert k_cache.is_contiguous() and v_cache.is_contiguous() and k_cache.shape[1] == H
    assert key_start is None or (key_start.dtype == torch.int32 and key_start.is_cuda)
    act = dtype or k_cache.dtype
    out = torch.empty(B, n, H, D, dtype=act, device=k_cache.device)
    L.check(L.load_exp().sjd_qkv_attention_fused(_ptr(qkv_part.data), qkv_part.n_chunks, _ptr(k_cache), _ptr(v_cache), _ptr(out), _ptr(qn_w),
                                            _ptr(qn_b), _ptr(kn_w), _ptr(kn_b), _ptr(inv_freq), _ptr(positions), B, n, H, D, k_cache.shape[2],
                                            _dtype_code(act), _row_norm(row_norm), _ptr(key_start), params.ptr if params is not None else None,
                                            int(kv_len), _stream()), "sjd_qkv_attention_fused")
    return out


def silu_mul(gate_up, rows=None, dtype=None, row_norm=None):
    """gate|up [T, 2I] (tensor, or G1 Partials with `rows`/`dtype` given) -> silu(gate) * up [T, I]; row_norm as in qknorm_rope_append."""
    t, part, nc = _part_args(gate_up)
    if t is not None:
        T, two_i, dtype, dev = t.shape[0], t.shape[1], t.dtype, t.device
        assert t.is_contiguous()
    else:
        T, two_i, dev = rows, gate_up.N, gate_up.data.device
    y = torch.empty(T, two_i // 2, dtype=dtype, device=dev)
    L.check(L.load().sjd_silu_mul_ex(_ptr(t), _ptr(y), T, two_i // 2, _dtype_code(dtype), part, nc, _row_norm(row_norm), _stream()),
            "sjd_silu_mul")
    return y


def gateup_silu(x, w_packed, inter, hidden, step_major=False, row_norm=None):
    """G1s: silu(r * gate(x)) * (r * up(x)) [T, inter] in ONE launch -- the gate|up projection (w_packed = pack_weight([Wg; Wu], hidden / 2,
    step_major)) with F3 as its epilogue; bit-identical to silu_mul(skinny_gemm(x, w_packed, 2 * inter, hidden, hidden / 2), row_norm=...).
    A stream that has "gateup_k4" (LS.STREAMS: PackedQ4) packed with KC = 2048 at hidden 8192 (LS.gateup_silu_chunked_ok) runs in four chunks, skinny_gemm's."""
    T = x.shape[0]
    assert x.is_contiguous() and x.shape[1] == hidden and w_packed.numel() == 2 * inter * hidden
    y = torch.empty(T, inter, dtype=x.dtype, device=x.device)
    if isinstance(w_packed, PackedZ):
        assert (w_packed.KC, w_packed.step_major) == (hidden // 2, bool(step_major)) and x.dtype == torch.bfloat16
        assert w_packed.n_raw == 0 or w_packed.raw_tiles is not None, "a gate|up weight with raw units must be packed with gateup=True"
        L.check(L.load().sjd_gateup_silu_z(_ptr(x), _ptr(w_packed.data), _ptr(w_packed.exc), w_packed.cap, _ptr(y), T, inter, hidden, int(step_major),
                                          _dtype_code(x.dtype), _row_norm(row_norm), _raw_units(w_packed, gateup=True), _stream()), "sjd_gateup_silu_z")
        return y
    (s, records, flag), sm = streamed(w_packed), int(step_major)
    if s is not None:          # G1sq / G1sq4 / G1sq6
        _same_16bit_type(x, w_packed, "gateup_silu")
        if "gateup_k4" in s.has:
            assert (w_packed.N, w_packed.step_major) == (2 * inter, bool(step_major))
            # packed in the two K halves, or (hidden 8192: the copy skinny_gemm streams in four chunks of 2048) the chunk count goes along; the library refuses the rest
            assert hidden % w_packed.KC == 0
            chunks = hidden // w_packed.KC
            sm |= 0 if chunks == 2 else chunks << L.G1S_CHUNKS_SHIFT
        else:
            assert (w_packed.N, w_packed.KC, w_packed.step_major) == (2 * inter, hidden // 2, bool(step_major))
    L.check(L.load().sjd_gateup_silu(_ptr(x), _ptr(records), _ptr(y), T, inter, hidden, sm, _dtype_code(x.dtype) | flag, _row_norm(row_norm), _stream()),
            "sjd_gateup_silu" + (f" ({s.names[0]} weights)" if s else ""))
    return y


_PAIR_READY = {}          # (device, stream) -> arrival counters of sjd_mlp_pair_z launches that CANNOT overlap (one stream runs them in order)


def mlp_pair_ok(T, inter, hidden, gu_packed, dn_packed, KC_dn, waves_dn, device):
    """shapes sjd_mlp_pair_z serves (see include/sjd_hip.h): a <= 32-row bf16 window at hidden 4096 over two 12-bit packed weights, the down
    projection in eight-tile workgroups with a K chunk that is a multiple of 64, the whole launch resident at once"""
    if not (isinstance(gu_packed, PackedZ) and isinstance(dn_packed, PackedZ)) or gu_packed.n_raw or dn_packed.n_raw:
        return False
    if T > 32 or hidden != 4096 or inter % 64 or KC_dn % 64 or KC_dn > LS.CHUNK_CAP_32ROW or waves_dn != 8 or gu_packed.KC != hidden // 2 or dn_packed.KC != KC_dn:
        return False
    grid = max(inter // 64, ((hidden // 32 + 7) // 8) * ((inter + KC_dn - 1) // KC_dn))
    return grid <= torch.cuda.get_device_properties(device).multi_processor_count


def mlp_pair(x, gu_packed, dn_packed, inter, hidden, KC_dn, row_norm=None, ready=None):
    """the MLP as ONE launch: -> (y [T, inter], Partials of the down projection); bit-identical to gateup_silu(...) then skinny_gemm(y, ...).
    ready: int32 arrival counters (>= n_chunks + 1 words, zero on entry; the launch re-arms them) PRIVATE to launches that cannot overlap --
    a backbone hands in its own; None: one buffer per (device, current stream), whose launches are ordered (the buffer used to be
    one per device, shared by every stream and engine)."""
    T = x.shape[0]
    assert x.is_contiguous() and x.dtype == torch.bfloat16 and x.shape[1] == hidden
    dev = x.device
    nc = (inter + KC_dn - 1) // KC_dn
    rd = ready
    if rd is None:
        key = (dev, int(torch.cuda.current_stream(dev).cuda_stream))
        rd = _PAIR_READY.get(key)
        if rd is None or rd.numel() < nc + 1:
            rd = _PAIR_READY[key] = torch.zeros(max(64, nc + 1), dtype=torch.int32, device=dev)
    assert rd.dtype == torch.int32 and rd.device == dev and nc + 1 <= rd.numel(), "sjd_mlp_pair_z: one arrival counter per K chunk of the down projection + 1"
    y = torch.empty(T, inter, dtype=x.dtype, device=dev)
    out = torch.empty(nc, 32, hidden, dtype=torch.float32, device=dev)
    L.check(L.load_exp().sjd_mlp_pair_z(_ptr(x), _ptr(gu_packed.data), _ptr(gu_packed.exc), gu_packed.cap, int(gu_packed.step_major), _ptr(y),
                                   _ptr(dn_packed.data), _ptr(dn_packed.exc), dn_packed.cap, int(dn_packed.step_major), _ptr(out), T, inter, hidden,
                                   int(KC_dn), _row_norm(row_norm), _ptr(rd), torch.cuda.get_device_properties(dev).multi_processor_count, _stream()),
            "sjd_mlp_pair_z")
    return y, Partials(out, nc, hidden)


def mlp_pair_timeouts():
    return int(L.load_exp().sjd_mlp_pair_timeouts())


def residual_sumsq(h, part=None, pull=None, pull_blocks=0):
    """F1r: h [T, hidden] += dtype(sum of the G1 partials) in place (part None: h unchanged); returns the per-512-column-slice sums
    of h^2 [slices, R] fp32 -- the `sumsq` of a row_norm.  pull (an l2_head) + pull_blocks: the same launch also pulls the head of the next
    projection's weight stream into the L2 (round 5); no effect on the result."""
    T, hidden = h.shape
    assert h.is_contiguous() and (part is None or (isinstance(part, Partials) and part.N == hidden))
    R = part.data.shape[1] if part is not None else _prows(T)
    out = torch.empty((hidden + 511) // 512, R, dtype=torch.float32, device=h.device)
    if pull is not None and pull_blocks > 0:
        L.check(L.load_exp().sjd_residual_sumsq_pf(_ptr(h), _ptr(part.data) if part is not None else None, part.n_chunks if part is not None else 0,
                                              T, hidden, _dtype_code(h.dtype), _ptr(out), ctypes.byref(pull), int(pull_blocks), _stream()), "sjd_residual_sumsq_pf")
        return out
    L.check(L.load().sjd_residual_sumsq(_ptr(h), _ptr(part.data) if part is not None else None, part.n_chunks if part is not None else 0,
                                       T, hidden, _dtype_code(h.dtype), _ptr(out), _stream()), "sjd_residual_sumsq")
    return out


class HipWindowAttention:
    """Backbone attention backend = K3 append + K1 draft-window attention (the product path)."""

    def __init__(self, n_split=None):
        """n_split: static upper bound of key splits per (batch, kv head); None = enough to give the 256 CUs ~512 workgroups
        (8 for MHA 2x32 heads, 32 for Emu3's 2x8 kv heads).  The kernel opens fewer splits for short contexts on its own."""
        L.load()
        self.n_split = n_split
        self._auto_split = n_split is None
        # K1 split-partial workspaces.  The window path (<= 64 rows, captured in the engine's hipGraphs) and the prefill path
        # (a whole prompt, eager) own SEPARATE buffers, so that a long prefill never replaces the buffer whose address the
        # captured window graphs hold; `ws_version` counts replacements of the window buffer and the engines drop their graphs
        # when it changes (sjd_amd/engine.py::_graphs_valid).
        self._ws = None
        self._ws_prefill = None
        self.ws_version = 0
        self._key_start = None
        self.params = None          # DeviceBlob(IterParams) when the engine drives kv_len from the device
        self.profile_layer = None   # int: time k1_partial of that layer with HIP events (bench.py roofline leg)
        self.profile_records = []   # (ev0, ev1, algorithmic_bytes)
        self._ev_pool = []
        self.kv_scale = (1.0, 1.0)  # (k, v) scales of an fp8 cache: stored byte = fp8(x / scale)
        # round 6: per-LAYER (k, v) scales from the amax of a calibration prefill (ChameleonBackbone.calibrate_kv_scales; the engines run it on
        # the first prompt of an fp8 cache): a list of (k, v) tuples, one per layer; None = `kv_scale` for every layer
        self.layer_scales = None
        # K1 regime of the NEXT window launches (round 4): "colsplit" = no key splits, four workgroups per (batch, head) split the output
        # columns (one launch; wins while the context is short), "keysplit" = key splits + k1_combine.  The engines set it per iteration from
        # the host-side kv_len (choose_regime) and key their hipGraphs on it.  SJD_K1_REGIME=keysplit|colsplit pins it (A/B aid).
        self.regime = "keysplit"
        self._pin_regime = os.environ.get("SJD_K1_REGIME")

    def scale_of(self, layer):
        """(k_scale, v_scale) of `layer`'s fp8 cache"""
        return self.kv_scale if self.layer_scales is None else self.layer_scales[layer]

    COLSPLIT_MAX_KEYS = {"16bit": 736, "fp8": 1536}       # crossover of the two forms (profiles/r4_k1_dsplit_ab.txt, r4_k1_dsplit_fp8_ab.txt)

    def choose_regime(self, kv_rows, cache_dtype, shape=None):
        """-> the regime for a window whose longest row sees `kv_rows` keys; sets self.regime.  shape = (B, n, H, H_kv, D) of the window
        launches: a shape the column split does not serve (GQA, 32-row windows, several prompts per forward) is "keysplit" whatever the
        context length or the pin -- the kernels are the same there, and a second set of graphs would only be captured twice."""
        if shape is not None and not colsplit_ok(*shape, cache_dtype):
            self.regime = "keysplit"
        elif self._pin_regime in ("keysplit", "colsplit"):
            self.regime = self._pin_regime
        else:
            self.regime = "colsplit" if kv_rows <= self.COLSPLIT_MAX_KEYS["fp8" if cache_dtype == FP8 else "16bit"] else "keysplit"
        return self.regime

    def _resolve_split(self, B, Hkv, n_rows=16, H=None, cache_bytes_per_head=None):
        """auto mode: one workgroup per CU for MHA (256 = B * H_kv * ceil(n_rows/16) * n_split; tools/k1_bench.py --graph: 4 splits
        22.3 us vs 8 splits 24.7 us per layer at kv_len 1216), two per CU for GQA, whose workgroups share each K/V tile between
        the q-heads of a group and are VGPR-limited to two per CU."""
        if self._auto_split:
            chunks = (n_rows + 15) // 16
            target = 256 if (H is None or H == Hkv) else 512
            self.n_split = int(min(64, max(1, target // (B * Hkv * chunks))))
            # a SHORT fp8 cache (config 5: Anole 512px, <= ~1150 keys of 128 bytes) is read faster by one workgroup per (batch, head)
            # that writes the output itself than by four splits + k1_combine: 5.7 / 8.9 / 12.2 us per layer at kv 64 / 552 / 1040
            # against 8.6 / 10.4 / 12.0 (profiles/r3_k1_split_sweep_before.jsonl); 16-bit caches of that length break even at kv ~450
            if cache_bytes_per_head is not None and cache_bytes_per_head <= 160 * 1024 and (H is None or H == Hkv) and chunks == 1:
                self.n_split = 1
        return self.n_split

    def _workspace(self, B, H, n, D, device):
        need = L.load().sjd_attention_workspace_bytes(B, H, n, D, self.n_split) // 4
        if n > 64:                                   # prefill rows: never captured, free to grow
            if self._ws_prefill is None or self._ws_prefill.numel() < need or self._ws_prefill.device != device:
                self._ws_prefill = torch.empty(need, dtype=torch.float32, device=device)
            return self._ws_prefill
        if self._ws is None or self._ws.numel() < need or self._ws.device != device:
            # sized for the largest window (64 rows) of this (B, H, D, n_split) so that it is allocated once per configuration
            full = L.load().sjd_attention_workspace_bytes(B, H, 64, D, self.n_split) // 4
            self._ws = torch.empty(max(need, full), dtype=torch.float32, device=device)
            self.ws_version += 1
        return self._ws

    def __call__(self, layer, q, k, v, cache, kv_len, key_start):
        kc, vc = cache.k[layer], cache.v[layer]
        if q.shape[3] == 100 and kc.shape[3] == 128:
            # a head_dim-100 model on a cache stored 128 wide (LlamaGenBackbone.enable_fused(pad_head_dim=True)): zero pad columns in, K1 at
            # D = 128 with the softmax scale of 100, the pad columns of the output (zeros) sliced off
            if kc.dtype == FP8:
                raise L.SjdLibraryError("HipWindowAttention: a padded head_dim 100 needs a 16-bit cache")
            zp = lambda t: torch.nn.functional.pad(t, (0, 28))
            return self._call(layer, zp(q), zp(k), zp(v), kc, vc, kv_len, key_start, 100)[..., :100]
        return self._call(layer, q, k, v, kc, vc, kv_len, key_start, None)

    def _call(self, layer, q, k, v, kc, vc, kv_len, key_start, head_dim):
        B, n, H, D = q.shape
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        self._resolve_split(B, kc.shape[1], n, H, kc.shape[2] * kc.shape[3] * kc.element_size() if kc.dtype == FP8 else None)
        if isinstance(key_start, torch.Tensor) and key_start.is_cuda and key_start.dtype == torch.int32:
            ks = key_start
        else:
            ks = torch.as_tensor(key_start, dtype=torch.int32).to(q.device)
        ws = self._workspace(B, H, n, D, q.device)
        out = torch.empty_like(q)
        kv_host = 0 if self.params is not None else int(kv_len)
        colsplit = self.regime == "colsplit" and colsplit_ok(B, n, H, kc.shape[1], D, kc.dtype)
        if kc.dtype == FP8:
            sk, sv = self.scale_of(layer)
            kv_append_fp8(k, v, kc, vc, sk, sv, self.params, kv_host)
            if colsplit:
                draft_window_attention_colsplit(q, kc, vc, out, ks, self.params, kv_host, (sk, sv))
            else:
                draft_window_attention_fp8(q, kc, vc, out, sk, sv, ks, self.params, kv_host, self.n_split, ws)
            return out
        kv_append(k, v, kc, vc, self.params, kv_host)
        if colsplit:
            draft_window_attention_colsplit(q, kc, vc, out, ks, self.params, kv_host, head_dim=head_dim)
            return out
        ev0 = ev1 = None
        if self.profile_layer is not None and layer == self.profile_layer and n <= 32:
            lib = L.load()
            ev0 = self._ev_pool.pop() if self._ev_pool else ctypes.c_void_p(lib.sjd_event_create())
            ev1 = self._ev_pool.pop() if self._ev_pool else ctypes.c_void_p(lib.sjd_event_create())
            esz = q.element_size()
            Hkv = kc.shape[0 + 1]
            # algorithmic bytes of one k1_partial launch: K and V rows [0, kv_len+n) once per kv head,
            # + q in, + fp32 split partials out
            if self.params is not None:         # device-driven mode: the host mirror of the blob holds this iteration's values
                kv_rows = int(self.params.view.kv_len) + int(self.params.view.n_rows)
            else:
                kv_rows = int(kv_len) + n
            alg = 2 * B * Hkv * kv_rows * D * esz + B * n * H * D * esz
            self.profile_records.append((ev0, ev1, alg, kv_rows))
        draft_window_attention(q, kc, vc, out, ks, self.params, kv_host, self.n_split, ws, ev0, ev1, head_dim=head_dim)
        return out

    def attend(self, layer, q, cache, kv_len, key_start, head_dim=None):
        """K1 only: the window's K/V rows were already written into the cache (fused F2 path).  head_dim: the model's head dim where q and
        the cache are stored wider (100 in 128-wide rows with zero pad columns: SJD_K1_HEAD_DIM_100)."""
        B, n, H, D = q.shape
        kc, vc = cache.k[layer], cache.v[layer]
        if head_dim is not None and head_dim != D and kc.dtype == FP8:
            raise L.SjdLibraryError("HipWindowAttention: a padded head_dim 100 needs a 16-bit cache")
        kv_host = 0 if self.params is not None else int(kv_len)
        # (the split workspace is allocated whatever the regime: its first allocation bumps ws_version, which makes the engines drop every
        #  captured graph -- that must happen before the first capture, not at the crossover in the middle of an image)
        self._resolve_split(B, kc.shape[1], n, H, kc.shape[2] * kc.shape[3] * kc.element_size() if kc.dtype == FP8 else None)
        ws = self._workspace(B, H, n, D, q.device)
        if self.regime == "colsplit" and colsplit_ok(B, n, H, kc.shape[1], D, kc.dtype):
            out = torch.empty_like(q)
            draft_window_attention_colsplit(q, kc, vc, out, key_start, self.params, kv_host, self.scale_of(layer), head_dim=head_dim)
            return out
        out = torch.empty_like(q)
        if kc.dtype == FP8:
            sk, sv = self.scale_of(layer)
            draft_window_attention_fp8(q, kc, vc, out, sk, sv, key_start, self.params, kv_host, self.n_split, ws)
        else:
            draft_window_attention(q, kc, vc, out, key_start, self.params, kv_host, self.n_split, ws, head_dim=head_dim)
        return out

    def profile_summary(self):
        """-> dict(launches, avg_ms, avg_bytes, gbps) over the recorded k1_partial launches; recycles the events."""
        lib = L.load()
        tot_ms, tot_b, n, rows = 0.0, 0, 0, 0
        for ev0, ev1, alg, kv_rows in self.profile_records:
            lib.sjd_event_synchronize(ev1)
            ms = lib.sjd_event_elapsed_ms(ev0, ev1)
            if ms > 0:
                tot_ms, tot_b, n, rows = tot_ms + ms, tot_b + alg, n + 1, rows + kv_rows
            self._ev_pool += [ev0, ev1]
        self.profile_records = []
        if n == 0:
            return None
        return dict(launches=n, avg_ms=tot_ms / n, avg_bytes=tot_b / n, avg_kv_rows=rows / n,
                    gbps=(tot_b / 1e9) / (tot_ms / 1e3))
