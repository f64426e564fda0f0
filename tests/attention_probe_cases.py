"""Probe inputs for draft-window attention (K1) on which the right answer is known exactly: builders, closed-form answers, a tile / split
model of csrc/sjd_attention.hip and a float32 model of the kernels' order of operations.

tests/test_gpu_attention_probes.py runs the probes on every K1 form through the product library; tests/test_attention_probe_cases.py shows
on the CPU that every case reaches the branch it is named for, that the closed forms are what fp64 attention gives, that the float32 model
reproduces the asserted integers / bits (so a zero tolerance is legitimate before anything runs on a GPU) and that the comparators catch
deliberately wrong models.  Nothing here touches the GPU or libsjd_hip.so.

Probe 1, key census.  q = 0, K Gaussian, V[j, d] = 1 if d == j mod D_logical else 0.  Every visible score is 0, every probability exactly 1
in the MFMA operand type, every rescale and merge weight exp(0) = 1, the accumulators hold the integers c_d = #{visible j = d mod D} and
L = N (the visible count); the kernel writes round16(fl32(c_d fl32(1 / N))) (x v_scale over an fp8 cache).  round(got N) == c_d names every
key that was counted twice or not at all.

Probe 2, dominant key.  q is 16 in column 0 and zero elsewhere, k[j, 0] = 32 x an integer level, so a level is 512 / sqrt(D_logical) >= 45 nats;
one visible key (or 2 / 4 / 8 tied ones) lies >= one level above every other visible key, exp(-45) sum |v| is far below half an fp32 ulp of the
answer, and the output is V[j*] (the tie mean) bit for bit whatever the accuracy of exp.

One form needs a condition of its own.  k1_partial_ring evaluates exp2(fma(s, c1, -fl(m c1))): the winner's probability and the rescale of a
tile that leaves the maximum where it was are 2^delta, delta the rounding error of m c1, not 1.  Numerator and sum take the same factors, so a
single winner still comes out as round16(round16(2^delta) v / 2^delta) = v while |m c1| < 2^13 (delta ln 2 below a quarter of an fp16 ulp:
levels <= 120).  TIED winners T tiles apart are weighted 2^(T delta) against each other (first seen on the GPU: two keys 37 tiles apart at
level 120, one split, fp16 -- one output ulp), so the tie level of a 16-bit cache is 64: m = 2^15, m c1 exact, delta = 0.  ring_exponent_ok()
asserts both conditions; the float32 model below keeps the fma and fails a tie at level 120 as the kernel does (test_ring_tie_drift_is_modelled).

Measured (test_bound_sensitivity_of_the_gaussian_tests): how often attention_fp64's element-wise bound notices a wrong key on the Gaussian
inputs of test_k1_k3_attention -- share of output elements of visible rows beyond the bound when the fp64 reference itself is perturbed:
    case            one key dropped at the causal edge    one 32-key tile dropped (mid context / last full tile)
    mha_d128_mid    3.7 %                                 65.9 % / 64.5 %
    gqa4_d128       2.3 %                                 65.6 % / 66.2 %
A dropped tile is seen (some element of the case is beyond the bound), but a third of the elements stay inside it; a single wrong key moves
one element in thirty.  The probes here make each of them a wrong integer or a wrong bit pattern.
"""
import math

import numpy as np
import torch

FP8 = torch.float8_e4m3fn
KT, ROWS, MIN_TILES_PER_SPLIT = 32, 16, 4            # K1_KT, K1_ROWS, K1_MIN_TILES_PER_SPLIT of csrc/sjd_attention.hip
Q0, STEP = 16.0, 32.0                                # q[..., 0]; k[j, 0] = STEP * level
MARGIN_NATS = 40.0
TORCH_DTYPE = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32}
HALF_ULP_REL = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}      # half an ulp relative to the binade's lower end (8 / 11 significant bits)


# ------------------------------------------------------------------------------------------------ forms, ranges
def _form(name, H, Hkv, D, n, dtype, cache="16", head_dim=None, scales=(1.0, 1.0), colsplit=False):
    return dict(name=name, H=H, Hkv=Hkv, D=D, n=n, dtype=dtype, cache=cache, DL=head_dim or D, head_dim=head_dim, scales=scales, colsplit=colsplit)


FORMS = [
    _form("partial8_bf16", 4, 4, 128, 16, "bf16"),
    _form("partial8_fp16", 4, 4, 128, 16, "fp16"),
    _form("partial8_n5", 4, 4, 128, 5, "bf16"),
    _form("partial4", 4, 2, 128, 16, "bf16"),
    _form("partial1_two_chunks", 8, 1, 128, 20, "fp16"),
    _form("partial_d64", 2, 2, 64, 16, "bf16"),
    _form("partial_d64_four_chunks", 2, 2, 64, 60, "fp16"),
    _form("partial_head100", 2, 2, 128, 16, "bf16", head_dim=100),
    _form("partial_three_chunks", 2, 2, 128, 40, "fp16"),
    _form("prefill60", 2, 2, 128, 60, "bf16"),               # four chunks of one head: 4 pairs -> launch_attention takes the ring kernel
    _form("ring4", 8, 2, 128, 16, "bf16"),
    _form("ring8_n32", 8, 2, 128, 32, "fp16"),
    _form("ring8_n20", 8, 2, 128, 20, "bf16"),
    _form("ring8_group8", 8, 1, 128, 16, "bf16"),
    _form("dsplit_bf16", 4, 4, 128, 16, "bf16", colsplit=True),
    _form("dsplit_fp16_n5", 4, 4, 128, 5, "fp16", colsplit=True),
    _form("dsplit_head100", 2, 2, 128, 16, "bf16", head_dim=100, colsplit=True),
    _form("dsplit_fp8", 4, 4, 128, 16, "bf16", cache="fp8", scales=(1.0, 0.25), colsplit=True),
    _form("fp8_mha", 4, 4, 128, 16, "bf16", cache="fp8"),
    _form("fp8_gqa2", 4, 2, 128, 16, "fp16", cache="fp8", scales=(1.0, 0.25)),
    _form("fp8_n5_quarter_scales", 4, 4, 128, 5, "bf16", cache="fp8", scales=(0.25, 0.25)),
    _form("fp8_d64", 2, 2, 64, 16, "bf16", cache="fp8"),
    _form("f32", 4, 2, 128, 7, "f32", cache="f32"),
]
FORM = {f["name"]: f for f in FORMS}


def ranges_of(form):
    """the key ranges every form is crossed with: name, kv_len, key_start of the two batch rows, valid rows (blob: read from the device)"""
    n = form["n"]
    return [
        dict(name="kv0", kv=0, ks=(0, min(3, n - 1))),                                  # empty cache; batch row 1 hides its first rows
        dict(name="tiles4_edge0", kv=128 - n, ks=(0, 32)),                              # kv + n = 0 mod 32, key_start = 0 mod 32, exactly 4 tiles
        dict(name="tiles5", kv=160 - n, ks=(0, 37)),                                    # exactly 5 tiles: two effective splits
        dict(name="tiles8", kv=256 - n, ks=(0, 5)),                                     # exactly 8 tiles
        dict(name="edge1", kv=129 - n, ks=(31, 63)),                                    # kv + n = 1 mod 32, key_start = 31 mod 32
        dict(name="middle_row", kv=70, ks=(70 + n // 2, 5)),                            # row n / 2 sees one key, the rows before it none
        dict(name="all_hidden", kv=40, ks=(((40 + n + KT - 1) // KT) * KT + 3, 0)),     # key_start > kv + n - 1 (no tile): batch row 0 sees nothing
        dict(name="last_split_short", kv=1233 - n, ks=(0, 59)),                         # 39 / 38 tiles over 8 splits of 5: the last one short
        dict(name="last_split_empty", kv=1056 - n, ks=(0, 40)),                         # 33 tiles over 8 splits of 5: the eighth empty
        dict(name="device_blob", kv=203, ks=(0, 37), nv=max(1, n - 3), blob=True),      # kv_len = -1, fewer valid rows than launched
    ]


def geometry(form, rng):
    """per batch row kv_len / valid rows / key_start of a launch, and the cache length"""
    n = form["n"]
    if "slots" in rng:                                       # a blob array: nb batch rows per slot
        nb = rng["nb"]
        kv = [k for k in rng["slots_kv"] for _ in range(nb)]
        nv = [r for r in rng["slots_rows"] for _ in range(nb)]
        ks = list(rng["ks"])
    else:
        nb = 0
        kv, nv, ks = [rng["kv"]] * 2, [rng.get("nv", n)] * 2, list(rng["ks"])
    S = rng.get("S") or ((max(kv) + n + 2 * KT - 1) // KT) * KT
    return dict(B=len(kv), n=n, kv=kv, nv=nv, ks=ks, S=S, blob=bool(rng.get("blob")) or nb > 0, nb=nb, name=rng["name"])


BLOB_ARRAY_RANGE = dict(name="blob_array", slots=True, nb=2, slots_kv=[0, 31, 1216, 700], slots_rows=[16, 16, 16, 1], ks=(0, 5, 0, 40, 0, 59, 0, 63), S=1280)
RING_4101_RANGE = dict(name="kv4101", kv=4101, ks=(0, 4089))      # 130 tiles over 16 splits of 9: the sixteenth gets none (ring, fp16)


def splits_of(form):
    if form["colsplit"] or form["cache"] == "f32":
        return [1]
    return [1, 4, 8, 16] if route(form, 4)["kernel"] == "k1_partial_ring" else [1, 4, 8]


# ------------------------------------------------------------------------------------------------ dispatch and tile model
def route(form, n_split):
    """launch_attention / launch_attention_fp8 / k1_dispatch of csrc/sjd_attention.hip restated"""
    H, Hkv, D, n = form["H"], form["Hkv"], form["D"], form["n"]
    G, n_chunks = H // Hkv, (n + ROWS - 1) // ROWS
    if form["cache"] == "f32":
        return dict(kernel="k1_f32", detail="k1_f32", combine=False)
    if form["cache"] == "fp8":
        if form["colsplit"]:
            return dict(kernel="k1_dsplit_fp8", detail="k1_dsplit_fp8", combine=False, kparts=8)
        return dict(kernel="k1_partial_fp8", detail=f"k1_partial_fp8<{8 // G} key-parts>", combine=n_split > 1, kparts=8 // G)
    if form["colsplit"]:
        return dict(kernel="k1_dsplit", detail="k1_dsplit" + ("<head 100>" if form["DL"] != D else ""), combine=False, kparts=8)
    pairs = G * n_chunks
    if D == 128 and pairs in (4, 8) and (G > 1 or n_chunks > 1):
        return dict(kernel="k1_partial_ring", detail=f"k1_partial_ring<{pairs} pairs>", combine=True, pairs=pairs)
    detail = f"k1_partial<{8 // G} key-parts" + (", D 64" if D == 64 else "") + (", head 100" if form["DL"] != D else "") + \
        (f", {n_chunks} chunks" if n_chunks > 1 else "") + ">"
    return dict(kernel="k1_partial", detail=detail, combine=n_split > 1, kparts=8 // G)


REQUIRED_DETAILS = [
    "k1_partial<8 key-parts>", "k1_partial<4 key-parts>", "k1_partial<1 key-parts, 2 chunks>", "k1_partial<8 key-parts, D 64>",
    "k1_partial<8 key-parts, D 64, 4 chunks>", "k1_partial<8 key-parts, head 100>", "k1_partial<8 key-parts, 3 chunks>",
    "k1_partial_ring<4 pairs>", "k1_partial_ring<8 pairs>", "k1_dsplit", "k1_dsplit<head 100>", "k1_dsplit_fp8",
    "k1_partial_fp8<8 key-parts>", "k1_partial_fp8<4 key-parts>", "k1_f32", "k1_combine"]


def tile_range(kstart, total, n_split):
    """k1_tile_range: -> t_lo, t_hi, effective splits, tiles per split"""
    t_lo, t_hi = kstart // KT, (total + KT - 1) // KT
    nt = max(t_hi - t_lo, 0)
    eff = min(n_split, max(1, (nt + MIN_TILES_PER_SPLIT - 1) // MIN_TILES_PER_SPLIT))
    tps = (nt + eff - 1) // eff
    if tps > 0:
        eff = (nt + tps - 1) // tps
    return t_lo, t_hi, eff, tps


def chunk_geometry(geo, b, chunk):
    """-> row0, n_c, kv_len of the chunk, total (keys >= total are visible to no row of the chunk)"""
    row0 = chunk * ROWS
    n_c = min(ROWS, geo["nv"][b] - row0)
    kv_len = geo["kv"][b] + row0
    return row0, n_c, kv_len, kv_len + max(n_c, 0)


def plan(form, geo, b, chunk, n_split):
    """the key tiles of one (batch row, chunk): [split][key-part] -> list of tiles, as the kernel form walks them"""
    r = route(form, n_split)
    _, _, _, total = chunk_geometry(geo, b, chunk)
    t_lo, t_hi, eff, tps = tile_range(geo["ks"][b], total, n_split)
    if r["kernel"] in ("k1_dsplit", "k1_dsplit_fp8"):
        return [[list(range(t_lo + w, t_hi, 8)) for w in range(8)]]
    out = []
    for s in range(eff):
        t0 = t_lo + s * tps
        t1 = min(t_hi, t0 + tps)
        if r["kernel"] == "k1_partial_ring":
            out.append([list(range(t0, t1))])
        else:
            out.append([list(range(t0 + kp, t1, r["kparts"])) for kp in range(r["kparts"])])
    return out


def branches(form, geo, n_split):
    """what a launch exercises: the set of names among eff<k>, short_last_split, dropped_split (the effective count below the tiles would
    allow because tiles-per-split rounds up), partial_last_tile, key_start_mid_tile, no_tile, hidden_rows, padding_rows"""
    got = set()
    for b in range(geo["B"]):
        for chunk in range((geo["n"] + ROWS - 1) // ROWS):
            row0, n_c, kv_len, total = chunk_geometry(geo, b, chunk)
            if n_c <= 0:
                got.add("padding_chunk")
                continue
            t_lo, t_hi, eff, tps = tile_range(geo["ks"][b], total, n_split)
            nt = max(t_hi - t_lo, 0)
            got.add(f"eff{eff}")
            if nt == 0:
                got.add("no_tile")
            if eff > 1 and nt - (eff - 1) * tps < tps:
                got.add("short_last_split")
            if eff < min(n_split, max(1, (nt + MIN_TILES_PER_SPLIT - 1) // MIN_TILES_PER_SPLIT)):
                got.add("dropped_split")
            if total % KT:
                got.add("partial_last_tile")
            if geo["ks"][b] % KT and geo["ks"][b] < total:
                got.add("key_start_mid_tile")
            if geo["ks"][b] > kv_len:
                got.add("hidden_rows")
            got.add(f"tiles{nt}")
        if geo["nv"][b] < geo["n"]:
            got.add("padding_rows")
    return got


def visible(geo, b, mutant=None):
    """bool [n, S]: key j visible to window row i of batch row b (rows >= the valid count see nothing)"""
    n, S = geo["n"], geo["S"]
    i = np.arange(n)[:, None]
    j = np.arange(S)[None, :]
    ks, kv = geo["ks"][b], geo["kv"][b]
    lo = ks - 1 if mutant == "leak_key_start" else ks
    hi = kv + i + (1 if mutant == "leak_causal" else 0)
    vis = (j >= lo) & (j <= hi) & (i < geo["nv"][b])
    if mutant == "leak_causal":                              # (the leaked key must exist: the kernel's `key < total` still holds)
        total = np.minimum(kv + ((i // ROWS) * ROWS + ROWS), kv + geo["nv"][b])
        vis &= j < total
    return vis


# ------------------------------------------------------------------------------------------------ inputs
_GAUSS = {}


def _gauss(B, Hkv, S, D, seed):
    key = (B, Hkv, S, D, seed)
    if key not in _GAUSS:
        _GAUSS[key] = torch.randn(B, Hkv, S, D, generator=torch.Generator().manual_seed(seed))
    return _GAUSS[key]


def levels_available(form, n_split=4):
    """positive integer levels k[j, 0] / 32 can take: an e4m3 cache holds |k / k_scale| <= 448 (levels are centred there); 16-bit caches: 8
    significant bits, 120 leaves room for the hostile level above a 60-row window"""
    if form["cache"] == "fp8":
        return 2 * int(448 * form["scales"][0] // STEP)       # 28 at k_scale 1, 6 at 0.25
    return 120


TIE_LEVEL_16BIT = 64         # m = 16 * 32 * 64 = 2^15: m c1 is exact in fp32 (module docstring: the ring kernel's exponent)


def tie_level(form):
    return levels_available(form) if form["cache"] == "fp8" else TIE_LEVEL_16BIT


def ring_exponent_ok(form, inp, n_split):
    """k1_partial_ring: every winner has |m c1| < 2^13, and tied winners an m c1 that fp32 holds exactly"""
    if route(form, n_split)["kernel"] != "k1_partial_ring" or inp["k0"] is None:
        return True
    c1 = float(f32(f32(1.0 / math.sqrt(form["DL"])) * f32(1.4426950408889634)))
    for b, rows in enumerate(inp["expect"]["winners"]):
        for w in rows:
            if w:
                mc = Q0 * float(inp["k0"][b, w[0]]) * c1
                exact = float(f32(mc)) == mc
                if (len(w) > 1 and not exact) or (abs(mc) >= 2.0 ** 13 and not exact):
                    return False
    return True


def level_offset(form):
    return levels_available(form) // 2 if form["cache"] == "fp8" else 0


_DOMV = {}


def _dominant_v(B, Hkv, S, D, seed, grid):
    key = (B, Hkv, S, D, seed, grid)
    if key not in _DOMV:
        _DOMV[key] = _dominant_v_make(B, Hkv, S, D, seed, grid)
    return _DOMV[key]


def _dominant_v_make(B, Hkv, S, D, seed, grid):
    g = torch.Generator().manual_seed(seed)
    if grid:                                                  # ties: multiples of 1/8 in [1, 2): the mean of 2 / 4 / 8 rows is representable
        return 1.0 + torch.randint(0, 8, (B, Hkv, S, D), generator=g).double() / 8
    e = torch.randint(-4, 2, (B, Hkv, S, D), generator=g).double()          # 2^-4 <= |v| < 4, four significant bits (exact in e4m3)
    m = torch.randint(0, 8, (B, Hkv, S, D), generator=g).double()
    s = torch.randint(0, 2, (B, Hkv, S, D), generator=g).double() * 2 - 1
    return s * (2.0 ** e) * (1 + m / 8)


LAYOUTS = ["own_key", "first_visible", "stair_up", "stair_down", "last_split_first_tile", "huge_positive", "huge_negative", "ties2", "ties4",
           "ties8", "hostile_invisible", "hostile_nan"]


def _common_range(geo, b):
    """keys every non-hidden row of batch row b sees: [lo, hi] (empty when lo > hi)"""
    return geo["ks"][b], geo["kv"][b]


def layout_k0(form, geo, layout, n_split):
    """-> k0 [B, S] float64 (the VALUE of k[j, 0]; all kv heads alike), hostile [B, S] bool (keys whose V rows are all 4), nan [B, S] bool,
    or None where the layout does not apply to the range (a reason string)"""
    B, S, n = geo["B"], geo["S"], geo["n"]
    Lmax, off = levels_available(form), level_offset(form)
    lev = np.zeros((B, S))
    hostile = np.zeros((B, S), bool)
    nan = np.zeros((B, S), bool)
    direct = None
    if layout in ("huge_positive", "huge_negative") and form["cache"] == "fp8":
        return "an e4m3 cache holds no 2^15"
    for b in range(B):
        kv, nv, ks = geo["kv"][b], geo["nv"][b], geo["ks"][b]
        lo, hi = _common_range(geo, b)
        t_lo, t_hi, eff, tps = tile_range(ks, kv + min(nv, ROWS), n_split)
        if layout in ("own_key", "hostile_invisible", "hostile_nan"):
            if nv + 1 > Lmax:
                return f"{nv} window rows need more than the {Lmax} levels of this cache"
            lev[b, kv:kv + nv] = 1 + np.arange(nv)
            if layout != "own_key":
                top = min(Lmax, nv + 60)
                hostile[b, :ks] = True
                hostile[b, kv + nv:] = True
                lev[b, hostile[b]] = top
                if layout == "hostile_nan":
                    nan[b, kv + n:] = True
        elif layout == "first_visible":
            if ks < S:
                lev[b, ks] = 1
        elif layout in ("stair_up", "stair_down"):
            tiles = list(range(t_lo, (kv + nv + KT - 1) // KT))
            if layout == "stair_up":
                tiles = tiles[-Lmax:]
            for r, t in enumerate(tiles):
                j = t * KT + (5 * t) % KT
                if j < S:
                    lev[b, j] = (r + 1) if layout == "stair_up" else max(Lmax - r, 0)
        elif layout == "last_split_first_tile":
            j = max((t_lo + (eff - 1) * tps) * KT, ks)
            if j < S:
                lev[b, j] = Lmax
        elif layout == "huge_positive":
            direct = direct if direct is not None else -STEP * (np.arange(S)[None, :] % 5) * np.ones((B, 1))
            direct[b, (lo + hi) // 2 if lo <= hi else min(ks, S - 1)] = 2.0 ** 15
        elif layout == "huge_negative":
            direct = direct if direct is not None else np.full((B, S), -2.0 ** 15 - 256)
            direct[b, (lo + 2 * hi) // 3 if lo <= hi else min(ks, S - 1)] = -2.0 ** 15
        else:
            c = int(layout[4:])
            if hi - lo + 1 < c:
                return f"batch row {b}: fewer than {c} keys are visible to every row"
            pos = np.unique(np.linspace(lo, hi, c).round().astype(int))
            if len(pos) < c:
                return f"batch row {b}: fewer than {c} keys are visible to every row"
            lev[b, pos] = tie_level(form)
    k0 = direct if direct is not None else STEP * (lev - off)
    return k0, hostile, nan


def build(form, geo, probe, layout=None, n_split=4, seed=0):
    """-> dict(q, kc, vc: what the launch gets (CPU tensors; caches [B, Hkv, S, D] with the window rows in place), raw [B, n, S] fp32 (q . k in
    operand units), vop [B, Hkv, S, D] fp32 (V operand values: the e4m3 VALUE over an fp8 cache), expect ...) or a reason string"""
    B, S, n, H, Hkv, D, DL = geo["B"], geo["S"], geo["n"], form["H"], form["Hkv"], form["D"], form["DL"]
    sk, sv = form["scales"]
    dt = TORCH_DTYPE[form["dtype"]]
    kg = _gauss(B, Hkv, S, D, 11).clone().double()
    if DL != D:
        kg[..., DL:] = 0
    q = torch.zeros(B, n, H, D, dtype=torch.float64)
    nan = np.zeros((B, S), bool)
    if probe == "census":
        v = torch.zeros(B, Hkv, S, D, dtype=torch.float64)
        j = torch.arange(S)
        v[:, :, j, j % DL] = 1.0 * sv
        k0 = None
    else:
        made = layout_k0(form, geo, layout, n_split)
        if isinstance(made, str):
            return made
        k0, hostile, nan = made
        q[..., 0] = Q0
        v = _dominant_v(B, Hkv, S, D, 23 + seed, layout.startswith("ties"))        # the VALUE; an fp8 cache stores v / v_scale
        hv = torch.from_numpy(hostile)[:, None, :, None].expand(B, Hkv, S, D)
        v = torch.where(hv, torch.full_like(v, 4.0), v)
        if DL != D:
            v[..., DL:] = 0
        kg[..., 0] = torch.from_numpy(k0)[:, None, :]
    nan_t = torch.from_numpy(nan)[:, None, :, None].expand(B, Hkv, S, D)
    if form["cache"] == "fp8":
        kc8, vc8 = (kg / sk).float().to(FP8), (v / sv).float().to(FP8)
        kop, vop = kc8.float().double(), vc8.float().double()
        assert torch.equal(vop * sv, v), "V is exact in e4m3"
        if k0 is not None:
            assert torch.equal(kop[..., 0] * sk, kg[..., 0]), "k[j, 0] is exact in e4m3"
        kc = torch.where(nan_t, torch.full_like(kc8.float(), float("nan")), kc8.float()).to(FP8)
        vc = torch.where(nan_t, torch.full_like(vc8.float(), float("nan")), vc8.float()).to(FP8)
        kval, vval = kop * sk, vop * sv
    else:
        kc, vc = kg.to(dt), v.to(dt)
        kop, vop = kc.double(), vc.double()
        assert torch.equal(vop, v), "V is exact in the cache type"
        if k0 is not None:
            assert torch.equal(kop[..., 0], kg[..., 0]), "k[j, 0] is exact in the cache type"
        kval, vval = kop, vop
        sign = torch.where(torch.arange(D) % 2 == 0, 1.0, -1.0).expand(B, Hkv, S, D).to(dt)
        kc = torch.where(nan_t, torch.full_like(kc, float("nan")), kc)
        vc = torch.where(nan_t, sign * float("inf"), vc)
    raw = np.zeros((B, n, S), np.float32)
    if k0 is not None:
        raw[:] = (Q0 * kop[:, 0, :, 0].numpy())[:, None, :].astype(np.float32)
        raw[np.broadcast_to(nan[:, None, :], raw.shape)] = np.nan
    out = dict(q=q.to(dt), kc=kc, vc=vc, raw=raw, vop=vop.float().numpy(), kval=kval, vval=vval, k0=k0, nan=nan, probe=probe, layout=layout)
    out["expect"] = census_answer(form, geo) if probe == "census" else dominant_answer(form, geo, k0, vval.numpy())
    if probe != "census":
        want = int(layout[4:]) if layout.startswith("ties") else 1
        for b in range(B):
            for i, w in enumerate(out["expect"]["winners"][b]):
                if w and len(w) != want:
                    return f"batch row {b} row {i} sees {len(w)} keys at its highest level, the layout wants {want}"
    return out


# ------------------------------------------------------------------------------------------------ closed forms
def census_answer(form, geo):
    """-> counts [B, n, D] int64 (c_d), N [B, n] int64"""
    B, n, S, D, DL = geo["B"], geo["n"], geo["S"], form["D"], form["DL"]
    counts = np.zeros((B, n, D), np.int64)
    N = np.zeros((B, n), np.int64)
    onehot = np.zeros((S, D), np.int64)
    onehot[np.arange(S), np.arange(S) % DL] = 1
    for b in range(B):
        vis = visible(geo, b)
        counts[b] = vis.astype(np.int64) @ onehot
        N[b] = vis.sum(1)
    return dict(counts=counts, N=N)


def dominant_answer(form, geo, k0, vval):
    """-> value [B, n, Hkv, D] fp64 (V[j*] or the tie mean; 0 for rows without a visible key), winners [B][n] -> key lists, margin (levels)"""
    B, n = geo["B"], geo["n"]
    value = np.zeros((B, n, vval.shape[1], vval.shape[3]))
    winners, margin = [], np.inf
    for b in range(B):
        vis = visible(geo, b)
        rows = []
        for i in range(n):
            keys = np.nonzero(vis[i])[0]
            if not len(keys):
                rows.append([])
                continue
            top = k0[b, keys].max()
            w = keys[k0[b, keys] == top]
            rest = k0[b, keys][k0[b, keys] < top]
            if len(rest):
                margin = min(margin, (top - rest.max()) / STEP)
            value[b, i] = vval[b][:, w].mean(1)
            rows.append(w.tolist())
        winners.append(rows)
    return dict(value=value, winners=winners, margin=margin)


def nats_per_level(form):
    return Q0 * STEP / math.sqrt(form["DL"])


# ------------------------------------------------------------------------------------------------ comparators
def _round16(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(TORCH_DTYPE[dtype]).float().numpy()


def census_failures(form, geo, expect, got, limit=6):
    """got [B, n, H, D] (any float array) -> list of messages; empty = every key counted exactly once"""
    got = np.asarray(got, dtype=np.float64)
    G, sv, DL = form["H"] // form["Hkv"], form["scales"][1] if form["cache"] == "fp8" else 1.0, form["DL"]
    c, N = expect["counts"][:, :, None, :], expect["N"][:, :, None, None]
    fails = []
    if not np.isfinite(got).all():
        return [f"{int((~np.isfinite(got)).sum())} non-finite outputs"]
    dec = np.rint(got * N / sv).astype(np.int64)
    bad = np.argwhere((dec != c) & (N > 0))
    for b, i, h, d in bad[:limit]:
        fails.append(f"batch row {b} row {i} head {h}: residue {d} mod {DL} counted {dec[b, i, h, d]} times, {c[b, i, 0, d]} keys are visible (N = {N[b, i, 0, 0]})")
    with np.errstate(divide="ignore", invalid="ignore"):
        exact = np.where(N > 0, c / np.maximum(N, 1), 0.0) * sv
    if form["dtype"] == "f32":
        tol = 2.0 ** -22 * exact
    else:       # half a 16-bit ulp of the exact value's binade plus two fp32 roundings (1 / N and the product)
        tol = HALF_ULP_REL[form["dtype"]] * 2.0 ** np.floor(np.log2(np.where(exact > 0, exact, 1.0))) * (exact > 0) + 2.0 ** -22 * exact
    over = np.argwhere(np.abs(got - exact) > tol)
    for b, i, h, d in over[:limit]:
        fails.append(f"batch row {b} row {i} head {h} column {d}: {got[b, i, h, d]!r} is not {c[b, i, 0, d]} / {N[b, i, 0, 0]} rounded once")
    zero = (np.broadcast_to(c, got.shape) == 0) | (np.broadcast_to(N, got.shape) == 0)
    nz = zero & ((got != 0) | np.signbit(got))
    if nz.any():
        fails.append(f"{int(nz.sum())} outputs that must be +0 (no visible key of that residue, hidden / padding rows, pad columns) are not, first {np.argwhere(nz)[0].tolist()}")
    return fails


def census_literal_excess(form, expect, got):
    """share of non-zero outputs beyond the narrower (2^-9 + 2^-22) c / N (bf16; 2^-12 fp16) -- reported, see SUMMARY: half an ulp is up to 2^-8 c / N"""
    got = np.asarray(got, dtype=np.float64)
    sv = form["scales"][1] if form["cache"] == "fp8" else 1.0
    c, N = expect["counts"][:, :, None, :], expect["N"][:, :, None, None]
    exact = np.where(N > 0, c / np.maximum(N, 1), 0.0) * sv
    rel = HALF_ULP_REL[form["dtype"]] / 2 + 2.0 ** -22
    nzm = np.broadcast_to(exact > 0, got.shape)
    return float((np.abs(got - exact) > rel * exact)[nzm].mean()) if nzm.any() else 0.0


def dominant_failures(form, geo, expect, got_t, limit=6):
    """got_t: torch tensor [B, n, H, D] in the output type -> list of messages; empty = V[j*] (the tie mean) bit for bit, hidden rows +0"""
    G = form["H"] // form["Hkv"]
    dt = TORCH_DTYPE[form["dtype"]]
    want = torch.from_numpy(expect["value"]).repeat_interleave(G, dim=2)
    want_t = want.to(dt)
    assert torch.equal(want_t.double(), want), "the closed-form answer is representable in the output type"
    view = torch.int32 if dt == torch.float32 else torch.int16
    bad = (got_t.contiguous().view(view) != want_t.contiguous().view(view)).any(-1)
    fails = []
    for b, i, h in bad.nonzero().tolist()[:limit]:
        who = "no key is visible" if not expect["winners"][b][i] else f"the answer is the V row of key(s) {expect['winners'][b][i]}"
        fails.append(f"batch row {b} row {i} head {h} (kv head {h // G}): {who}; got {got_t[b, i, h, :4].tolist()} ..., want {want[b, i, h, :4].tolist()} ...")
    return fails


# ------------------------------------------------------------------------------------------------ float32 model of the kernels
MUTANTS = ["drop_last_key_of_split", "drop_first_tile_of_split", "leak_causal", "leak_key_start", "swap_merge_weights", "old_max_in_rescale",
           "unshifted_split_max"]
f32 = np.float32
NINF = f32(-np.inf)


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def _safe(m):
    return np.where(np.isneginf(m), f32(0), m).astype(np.float32)


def _hilo8(x):
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    hi = t.to(FP8).float()
    lo = ((t - hi) * 16.0).to(FP8).float()
    return hi.numpy(), lo.numpy()


def _part(tiles, raw, vis, vop, total, form, ring, mutant):
    """one wave's online softmax over its tiles -> m [R] (in nats), l [R], O [Hkv, R, D] (V operand units x the P scale folded back)"""
    R, Hk, D = raw.shape[0], vop.shape[0], vop.shape[2]
    fp8 = form["cache"] == "fp8"
    scale = f32(f32(1.0 / math.sqrt(form["DL"])) * f32(form["scales"][0] if fp8 else 1.0))
    c1 = f32(f32(1.0 / math.sqrt(form["DL"])) * f32(1.4426950408889634))
    m = np.full(R, NINF, np.float32)
    l = np.zeros(R, np.float32)
    acc = np.zeros((Hk, R, D), np.float32)
    acc_lo = np.zeros((Hk, R, D), np.float32)
    for t in tiles:
        sl = slice(t * KT, (t + 1) * KT)
        v = vop[:, sl].copy()
        v[:, np.arange(t * KT, (t + 1) * KT) >= total] = 0
        if ring:
            s = np.where(vis[:, sl], raw[:, sl], NINF).astype(np.float32)
        else:
            s = np.where(vis[:, sl], (raw[:, sl] * scale).astype(np.float32), NINF).astype(np.float32)
        m_new = np.maximum(m, s.max(1))
        ms = _safe(m_new)
        m_ref = _safe(m) if mutant == "old_max_in_rescale" else ms
        if ring:
            nm = (-m_ref * c1).astype(np.float32)
            alpha = np.exp2(_fma(m, c1, nm)).astype(np.float32)
            p = np.exp2(_fma(s, c1, nm[:, None])).astype(np.float32)
        else:
            alpha = np.exp((m - m_ref).astype(np.float32)).astype(np.float32)
            p = np.exp((s - m_ref[:, None]).astype(np.float32)).astype(np.float32)
        if mutant == "old_max_in_rescale":
            alpha = np.where(np.isneginf(m), f32(0), f32(1)).astype(np.float32)
        l = ((l * alpha).astype(np.float32) + p.sum(1, dtype=np.float32)).astype(np.float32)
        m = m_new
        acc = (acc * alpha[None, :, None]).astype(np.float32)
        if fp8:
            hi, lo = _hilo8((p * f32(256.0)).astype(np.float32))
            acc_lo = (acc_lo * alpha[None, :, None]).astype(np.float32)
            acc = (acc + np.einsum("rk,hkd->hrd", hi, v)).astype(np.float32)
            acc_lo = (acc_lo + np.einsum("rk,hkd->hrd", lo, v)).astype(np.float32)
        else:
            acc = (acc + np.einsum("rk,hkd->hrd", _round16(p, form["dtype"]), v)).astype(np.float32)
    if fp8:
        acc = ((acc + acc_lo * f32(1.0 / 16.0)).astype(np.float32) * f32(f32(form["scales"][1]) / f32(256.0))).astype(np.float32)
    if ring:
        m = (m * f32(1.0 / math.sqrt(form["DL"]))).astype(np.float32)
    return m, l, acc


def _merge_parts(parts, mutant):
    """k1_merge_publish / k1_dsplit: the key-parts of a workgroup -> (M, L, O)"""
    M = np.maximum.reduce([p[0] for p in parts])
    Ms = np.zeros_like(M) if mutant == "unshifted_split_max" else _safe(M)
    L = np.zeros_like(parts[0][1])
    O = np.zeros_like(parts[0][2])
    for m, l, o in parts:
        w = np.exp((m - Ms).astype(np.float32)).astype(np.float32)
        L = (L + (w * l).astype(np.float32)).astype(np.float32)
        O = (O + (w[None, :, None] * o).astype(np.float32)).astype(np.float32)
    return M, L, O


def _merge_step(M, L, acc, m, l, o, mutant):
    """k1_merge_step"""
    Mn = np.maximum(M, m)
    Ms = np.zeros_like(Mn) if mutant == "unshifted_split_max" else _safe(Mn)
    w0, w1 = np.exp((M - Ms).astype(np.float32)).astype(np.float32), np.exp((m - Ms).astype(np.float32)).astype(np.float32)
    if mutant == "swap_merge_weights":
        w0, w1 = w1, w0
    L = _fma(L, w0, (l * w1).astype(np.float32))
    acc = _fma(acc, w0[None, :, None], (o * w1[None, :, None]).astype(np.float32))
    return Mn, L, acc


def kernel_model(form, geo, inp, n_split, mutant=None):
    """float32 model of one launch, in the kernels' order of operations: per-tile maximum, rescale, P rounded to the operand type, fp32
    accumulation, key-part merge, split merge in split order, acc (1 / L), one rounding to the output type.  -> [B, n, H, D] float32.
    mutant: one of MUTANTS (a deliberately wrong kernel the comparators must catch)"""
    B, n, H, Hkv, D = geo["B"], geo["n"], form["H"], form["Hkv"], form["D"]
    r = route(form, n_split)
    out = np.zeros((B, n, Hkv, D), np.float32)
    with np.errstate(all="ignore"):
        for b in range(B):
            vis = visible(geo, b, mutant if mutant in ("leak_causal", "leak_key_start") else None)
            raw, vop = inp["raw"][b], inp["vop"][b]
            if r["kernel"] == "k1_f32":
                scale = f32(1.0 / math.sqrt(D))
                for i in range(min(n, geo["nv"][b])):
                    keys = np.nonzero(vis[i])[0]
                    if not len(keys):
                        continue
                    s = (raw[i, keys] * scale).astype(np.float32)
                    e = np.exp((s - s.max()).astype(np.float32)).astype(np.float32)
                    acc = np.zeros((Hkv, D), np.float32)
                    for e_j, j in zip(e, keys):
                        acc = _fma(e_j, vop[:, j], acc)
                    out[b, i] = (acc * f32(f32(1.0) / e.sum(dtype=np.float32))).astype(np.float32)
                continue
            for chunk in range((n + ROWS - 1) // ROWS):
                row0, n_c, kv_len, total = chunk_geometry(geo, b, chunk)
                if n_c <= 0:
                    continue
                rows = slice(row0, row0 + n_c)
                partials = []
                for s_idx, parts in enumerate(plan(form, geo, b, chunk, n_split)):
                    done = []
                    for tiles in parts:
                        v = vis[rows].copy()
                        if mutant == "drop_first_tile_of_split" and s_idx > 0:
                            first = min(p[0] for p in parts if p)
                            tiles = [t for t in tiles if t != first]
                        if mutant == "drop_last_key_of_split":
                            last = max(p[-1] for p in parts if p) if any(parts) else None
                            if last is not None:
                                v[:, min((last + 1) * KT, total) - 1] = False
                        done.append(_part(tiles, raw[rows], v, vop, total, form, r["kernel"] == "k1_partial_ring", mutant))
                    partials.append(done[0] if r["kernel"] == "k1_partial_ring" else _merge_parts(done, mutant))
                if r["combine"]:
                    M = np.full(n_c, NINF, np.float32)
                    L = np.zeros(n_c, np.float32)
                    acc = np.zeros((Hkv, n_c, D), np.float32)
                    for m, l, o in partials:
                        M, L, acc = _merge_step(M, L, acc, m, l, o, mutant)
                else:
                    _, L, acc = partials[0]
                inv = np.where(L > 0, f32(1.0) / np.where(L > 0, L, f32(1)), f32(0)).astype(np.float32)
                out[b, rows] = np.transpose((acc * inv[None, :, None]).astype(np.float32), (1, 0, 2))
    if form["dtype"] != "f32":
        out = _round16(out, form["dtype"])
    return np.repeat(out, H // Hkv, axis=2)


# ------------------------------------------------------------------------------------------------ fp64 attention with a perturbed mask
def attention_fp64_masked(q, kc, vc, kv_len, n_rows, key_start, drop=None, scale_dim=None):
    """fp64 attention of ONE slot as blob_array_cases.attention_fp64 computes it, with `drop` [nb, n, total] bool keys removed from the mask"""
    nb, _, H, D = q.shape
    G, n, total = H // kc.shape[1], int(n_rows), int(kv_len) + int(n_rows)
    K = kc[:, :, :total].double().repeat_interleave(G, dim=1)
    V = vc[:, :, :total].double().repeat_interleave(G, dim=1)
    S = q[:, :n].double().transpose(1, 2) @ K.transpose(-1, -2) / math.sqrt(scale_dim or D)
    j = torch.arange(total)[None, None, None, :]
    i = torch.arange(n)[None, None, :, None]
    vis = (j >= torch.as_tensor(key_start).view(nb, 1, 1, 1)) & (j <= int(kv_len) + i)
    if drop is not None:
        vis = vis & ~drop[:, None]
    S = S.masked_fill(~vis, float("-inf"))
    m = S.max(dim=-1, keepdim=True).values
    E = torch.exp(S - torch.where(torch.isinf(m), torch.zeros_like(m), m))
    den = E.sum(-1, keepdim=True)
    P = torch.where(den > 0, E / den.clamp_min(1e-300), torch.zeros_like(E))
    return (P @ V).transpose(1, 2)
