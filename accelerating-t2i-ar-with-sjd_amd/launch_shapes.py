"""Launch shapes (split-K chunk, column tiles per workgroup, step-major packing) of the window projections: the tuned sets, the kernels' limits, and
what serves which rows.  The packed layout depends on the chunk, so a set is chosen when the weights are packed (enable_fused).  STREAMS: the lossy streams."""
from typing import NamedTuple

import torch

# ------------------------------------------------------------------------------------------ the kernels' limits
WIDE_TILES = (2, 3, 4, 6, 8)      # column tiles per workgroup kernel G1w / G1wq takes: 2, 3, 4 (one per wave) or 6, 8 (two per wave)
CHUNK_CAP_32ROW = 2560            # columns of an activation chunk a <= 32-row window stages whole in LDS (G1, G1z, G1q)
CHUNK_CAP_64ROW = 1280            # the same at 33..64 rows: the staged chunk is twice as tall
Z_MAX_ROWS = 128                  # the 12-bit stream (G1z / G1sz) serves windows of up to 128 rows
WINDOW_MAX_ROWS = 256             # the window path (G1, F1-F3) as a whole; above 64 rows a batch row holds at most 32 of them (longer inputs are prefill)
PREFILL_ROW_BLOCK = 128           # rows of a workgroup of kernel G1p (csrc/sjd_gemm_prefill.h: G1P_ROWS), the prefill projection over the packed copies
Z_MAX_KC = 4096                   # the 12-bit packer: the k-step of an exception is 7 + 1 bits of its position

# ------------------------------------------------------------------------------------------ Chameleon / Lumina-mGPT / Emu3
# G1 launch shape per projection: (split-K chunk, column tiles per workgroup, step-major packing) -- tuned on MI355X with
# tools/g1_bench.py so that every launch gives the 256 CUs ~1000+ balanced waves
G1_CFG = dict(qkv=(896, 8, True), o=(512, 6, False), gate_up=(2048, 8, True), down=(896, 8, False))
# the same for the 12-bit weight stream (G1z): the launch-shape sweep of tools/g1z_bench.py --sweep and an end-to-end A/B on one box
# (profiles/r3_g1z_microbench.txt: 3.068 / 3.090 -> 3.044 ms per step); taken by enable_fused when the caller has not set G1_CFG itself
G1_CFG_Z = dict(qkv=(1024, 6, True), o=(512, 6, False), gate_up=(2048, 8, True), down=(768, 8, False))
# the same for 64-row windows (two prompts per forward, or a draft window of 32): the staged chunk is twice as tall, so KC <= 1280;
# set `model.G1_CFG = model.G1_CFG_64ROW` before enable_fused (the packing depends on KC).  Tuned end to end at Lumina-7B shapes.
# (round 3: gate|up packed in two K halves = the copy kernel G1s streams, which now serves 64 rows; (1024, 12) was the G1 + F3 shape)
# (late round 6: o on four column tiles per workgroup -- on the 12-bit stream that launch shape runs on kernel G1w's 12-bit form, the one place it beats
#  G1z: two prompts per forward 3.50 -> 3.44 ms per step, profiles/r6_g1wz_o_64rows_ab.txt; round 2's shape: o (512, 8, False))
G1_CFG_64ROW = dict(qkv=(896, 8, True), o=(512, 4, True), gate_up=(2048, 8, True), down=(896, 8, False))       # profiles/r2_g1_launch_shape_sweep_64rows.jsonl
# 65..128-row windows (three / four prompts per forward): the activation is sub-tiled, so KC is free again, but <= 8 waves.  Round 3:
# 4-wave workgroups run on g1_skinny_gemm_tiled8 (8-step sub-tiles, two workgroups per CU, weight ring refilled in place) -- q|k|v,
# o and down are faster there (28.1 / 15.8 / 28.4 -> 25.7 / 12.2 / 24.0 us); 8-wave workgroups run on the same kernel with one workgroup
# per CU (gate|up 49.4 -> 43.3 us, profiles/r3_g1_tiled8.txt); four prompts per forward 5.55 -> 4.89 ms per step on one box
# (late round 6: bf16 windows of 65..128 rows run on kernel G1w as well -- the second number is then its column tiles per workgroup -- with gate|up
#  on six tiles and down in chunks of 1408: four prompts 4.43 -> 4.26 ms per step, three 4.05 -> 3.95 on one box, profiles/r6_g1w_128rows_ab.txt;
#  round 5's shapes: gate_up (2048, 8), down (1376, 4).  fp16 and the 12-bit stream keep the sub-tiled kernels on the same shapes.)
G1_CFG_128ROW = dict(qkv=(2048, 4, True), o=(896, 4, True), gate_up=(2048, 6, True), down=(1408, 4, True))
# 129..256-row windows (five to eight prompts per forward): kernel G1w (csrc/sjd_gemm_wide.h, round 6) -- the second number is the column tiles
# per workgroup: 2, 3, 4 (one per wave) or 6, 8 (two per wave).  tools/g1w_bench.py at 256 rows (profiles/r6_g1w_sweep.txt), us per launch against
# round 5's g1_skinny_gemm_tiled8: q|k|v 34.3 / 46.1, o 19.6 / 23.4, gate|up 58.4 / 84.4, down 31.3 / 38.2 (hipBLASLt: 50.4 / 19.1 / 65.9 / 52.7); o with
# four planes instead of (512, 4)'s eight: 16.4 us alone, but 7.18 against 7.37 ms per step (F1r sums the planes; profiles/r6_g1w_cfg_ab.txt)
G1_CFG_256ROW = dict(qkv=(2048, 4, True), o=(1024, 2, True), gate_up=(2048, 8, True), down=(1408, 4, True))
# Emu3-Gen 8B (GQA 32/8: the q|k|v projection has 6144 columns; draft window 32 -> 64 rows), tuned end to end with bench.py --model emu3_8b
# (late round 6: 33..64-row windows on the uncompressed stream run on kernel G1w -- the second number is its column tiles per workgroup -- with its own
#  shapes: per launch q|k|v 12.8 / 13.6 us, o 9.4 / 11.2, down 22.5 / 25.2 against round 2's (512, 8) / (512, 8) / (896, 8) on the whole-chunk kernel,
#  profiles/r6_g1w_sweep_64rows_emu3.jsonl; Emu3 in fp16 4.37 -> 4.17 ms per step, profiles/r6_g1w_64rows_emu3_ab.txt)
G1_CFG_EMU3 = dict(qkv=(1024, 4, True), o=(512, 4, True), gate_up=(2048, 8, True), down=(1792, 4, True))
# the same on the 12-bit stream (Emu3 in bf16, round 4): 256-workgroup launches for q|k|v and o, step-major packing -- 11.75 / 10.25 / 19.85 us
# against 12.15 / 10.66 / 20.19 (tools/g1z_bench.py --sweep --emu3 --rows 64, profiles/r4_g1z_sweep_emu3_64rows.jsonl)
G1_CFG_EMU3_Z = dict(qkv=(512, 6, True), o=(512, 4, True), gate_up=(2048, 8, True), down=(896, 8, True))
# the 8-bit e4m3 stream (enable_fused(weights="e4m3"), kernels G1q / G1sq): UNTUNED -- the 12-bit sets with every chunk cut to what G1q stages whole
# in LDS at the architecture's row count (Emu3: 64 rows, KC <= 1280, so its gate|up runs unfused as G1q + F3 in four chunks); no launch-shape
# sweep was run for this format.  G1_CFG_Q8's gate|up keeps the two K halves of 2048 that the fused 32-row launch (G1sq) streams; a window of
# 33..64 rows (a draft window of 32 with CFG, the prefill of a 17..32-token prompt) reads that step-major copy in chunks of 1024 (chunk_for_rows)
G1_CFG_Q8 = dict(qkv=(1024, 6, True), o=(512, 6, False), gate_up=(2048, 8, True), down=(768, 8, False))
G1_CFG_EMU3_Q8 = dict(qkv=(512, 6, True), o=(512, 4, True), gate_up=(1024, 8, True), down=(896, 8, True))
# the 8-bit stream for several prompts per forward (enable_fused(weights=..., max_rows=128 / 256)): UNTUNED -- G1_CFG_256ROW / G1_CFG_EMU3 as they are,
# except o on three column tiles (kernel G1wq, like G1w, has no form of three row tiles x two column tiles: 65..96 rows).  ONE packed copy serves every row
# count: <= 32 rows on G1q / G1sq (every chunk <= 2560; gate|up in the two K halves the fused launch streams), 33..64 on G1q in halved chunks
# (chunk_for_rows: all step-major, K and the chunks multiples of 32 / 64), 65..256 on G1wq with these chunks and tile counts.  No sweep was run.
G1_CFG_Q8_WIDE = dict(qkv=(2048, 4, True), o=(1024, 3, True), gate_up=(2048, 8, True), down=(1408, 4, True))
G1_CFG_EMU3_Q8_WIDE = dict(qkv=(1024, 4, True), o=(512, 4, True), gate_up=(2048, 8, True), down=(1792, 4, True))
# the MXFP4 stream (enable_fused(weights="mxfp4"), kernels G1q4 / G1sq4): UNTUNED -- copies of the 8-bit sets (every chunk a multiple of Q4_GRANULE, <= 2560, and one
# that halves to <= 1280 for 33..64 rows); no launch-shape sweep was run for this format
G1_CFG_Q4 = dict(G1_CFG_Q8)
G1_CFG_EMU3_Q4 = dict(G1_CFG_EMU3_Q8)
# 30B-class Chameleon (hidden 8192, intermediate 22016, GQA 64 / 8: q|k|v 10240 columns, gate|up 44032, down K 22016); chunks <= 2560 so that
# the 32-row window stages its chunk in LDS.  The fastest shapes of `tools/swin30b_bench.py --sweep` at 32 rows on one MI355X
# (profiles/g1_30b_sweep.jsonl), us per launch uncompressed / 12-bit: q|k|v 30.4 / 25.2, o 23.8 / 20.3, gate|up 120.5 / 98.9, down 62.9 / 50.4
G1_CFG_30B = dict(qkv=(1536, 8, True), o=(1536, 8, False), gate_up=(2048, 8, True), down=(1536, 8, False))
G1_CFG_30B_Z = dict(qkv=(1792, 8, True), o=(1280, 8, True), gate_up=(2048, 8, True), down=(1536, 8, True))
# the same backbones on the quantised streams (enable_fused(weights=..., swin_quant=True)): UNTUNED -- G1_CFG_30B_Z's values, which pass quant_copy_errors on
# either granule at these dimensions (every chunk a multiple of Q4_GRANULE, <= CHUNK_CAP_32ROW, step-major so that 33..64 rows read it in halved chunks;
# G1_CFG_30B's tile-major chunks of 1536 cannot be halved); no launch-shape sweep was run on either stream.  gate|up keeps the four chunks of 2048: the
# copy G1q / G1q4 + F3 stream, and on "mxfp4" at <= 32 rows the one the fused K = 8192 launch streams (gateup_silu_chunked_ok)
G1_CFG_30B_Q8 = dict(G1_CFG_30B_Z)
G1_CFG_30B_Q4 = dict(G1_CFG_30B_Z)


class WeightStream(NamedTuple):
    """A LOSSY weight stream of the window projections, stated once (plain data: no import of ops or _lib); ops.PackedZ and the plain packing are not rows"""
    names: tuple                  # enable_fused(weights=...): the stream, and its verification twin (the dequantised values, packed uncompressed)
    tag: str                      # compress_stats' "<tag>_matrices" / "<tag>_bytes_packed"; the packer is ops.pack_weight_<tag>, its class ops.Packed<TAG>
    flag: str                     # the _lib constant the C entry points take beside the dtype code
    granule: int                  # K and every chunk are multiples of it
    max_rows: int                 # window rows a Chameleon-family backbone serves from it (above 64: packed with enable_fused(max_rows=128 / 256))
    kernels: str                  # the kernels a row-limit refusal names
    has: frozenset                # of "prefill" (G1p, release_16bit), "swin" (swin_quant), "llamagen" (there up to 256 rows), "gateup_k4" (gateup_silu_chunked_ok)
    sets: tuple                   # default_shapes: the plain set, Emu3's, the 30B class's, and the plain and Emu3's for max_rows > 64 (None: no wide form)


STREAMS = (
    WeightStream(("e4m3", "e4m3_as_bf16"), "q8", "G1_W8_E4M3", 32, 256, "G1q / G1sq", frozenset({"prefill", "swin", "llamagen"}),
                 (G1_CFG_Q8, G1_CFG_EMU3_Q8, G1_CFG_30B_Q8, G1_CFG_Q8_WIDE, G1_CFG_EMU3_Q8_WIDE)),
    WeightStream(("mxfp4", "mxfp4_as_bf16"), "q4", "G1_W4_MXFP4", 128, 64, "G1q4 / G1sq4", frozenset({"prefill", "swin", "llamagen", "gateup_k4"}),
                 (G1_CFG_Q4, G1_CFG_EMU3_Q4, G1_CFG_30B_Q4, None, None)),
    # (window rows of folded-norm Chameleon-family backbones only, on the MXFP4 sets -- UNTUNED for it too; no swin route, so the 30B set is never reached)
    WeightStream(("e2m3", "e2m3_as_bf16"), "q6", "G1_W6_E2M3", 128, 64, "G1q6 / G1sq6", frozenset(), (G1_CFG_Q4, G1_CFG_EMU3_Q4, G1_CFG_30B_Q4, None, None)),
)


def stream_of(weights):
    """(stream, is_twin) of a `weights=` name; (None, False) for None and for a name no stream has"""
    return next(((s, weights == s.names[1]) for s in STREAMS if weights in s.names), (None, False))


Q4_WEIGHTS, Q6_WEIGHTS = STREAMS[1].names, STREAMS[2].names
QUANT_WEIGHTS = tuple(n for s in STREAMS if "llamagen" in s.has for n in s.names)          # the streams with a LlamaGen route: without the e2m3 names
Q4_GRANULE = STREAMS[1].granule   # K granule of the MXFP4 stream (ops.pack_weight_q4), and of the e2m3 stream
Q4_MAX_ROWS, Q6_MAX_ROWS = STREAMS[1].max_rows, STREAMS[2].max_rows          # kernels G1q4 / G1sq4 and G1q6 / G1sq6 have no wide form
HEAD_CFG = (1024, 4, True)         # G1 launch shape of the output head: (split-K chunk, column tiles per workgroup, step-major)
# vocabularies whose image window is tens of thousands of columns (Emu3: 32768 of 184622): two K chunks, so that K2 sums two planes per
# column instead of four, eight tiles per workgroup; Emu3 4.65 -> 4.62 ms per step (bench.py, SJD_HEAD_CFG sweep, one box)
HEAD_CFG_WIDE = (2048, 8, True)

# ------------------------------------------------------------------------------------------ LlamaGen
LLAMAGEN_SETS = {      # (head_dim 100 stored 128 wide, max_rows) -> (G1_CFG, HEAD_CFG)
    # G1 launch shapes of the window forward (<= 64 rows): (split-K chunk, column tiles per workgroup, step-major packing) per projection and for
    # the output head.  `tools/llamagen_bench.py --sweep` at 32 rows, GPT-XL (profiles/llamagen_g1_sweep.jsonl): per projection the fastest shape
    # with at most eight split-K planes (one batch of plane loads in F1r / F2 / F3), us per launch q|k|v 5.36, o 4.46, gate|up 6.64, down 6.35,
    # head 10.09 (the launch-alone optimum, KC 128, is 0.3 - 1.4 us faster but leaves 10 - 28 planes for the consumer to sum)
    (False, 64): (dict(qkv=(256, 2, True), o=(256, 2, False), gate_up=(320, 2, False), down=(512, 2, False)), (640, 4, True)),
    # Several prompts per forward (SJDBatchEngine): 65..128 and 129..256 window rows run on G1's sub-tiled kernels / kernel G1w, whose workgroups
    # take 2, 3, 4, 6 or 8 column tiles.  The packed layout depends on the split-K chunk, so the set is chosen when the weights are packed:
    # enable_fused(..., max_rows=128 / 256); forward_window then serves windows of up to that many rows on the HIP path.
    # `tools/llamagen_bench.py --sweep --rows 128 / 256`, GPT-XL (profiles/llamagen_g1_sweep_128rows.jsonl, _256rows.jsonl): per projection the
    # fastest shape with at most eight planes -- us per launch at 128 rows q|k|v 6.92, o 5.36, gate|up 8.68, down 7.27, head 12.54; at 256 rows
    # 9.80, 8.16, 12.31, 11.18, 17.87 (the 32-row set at 256 rows would still run: every tile count above is one kernel G1w takes)
    (False, 128): (dict(qkv=(320, 2, False), o=(256, 2, False), gate_up=(320, 4, True), down=(512, 2, False)), (640, 4, True)),
    (False, 256): (dict(qkv=(256, 4, False), o=(256, 2, False), gate_up=(320, 4, True), down=(512, 4, False)), (640, 4, True)),
    # GPT-3B (dim 3200, 32 heads of 100 stored 128 wide: pad_head_dim=True; inter 8704; the o projection's K is 32 * 128 = 4096): the KC 256 / 320 / 512
    # of the sets above would leave 13 / 10 / 17 planes, so the chunks are the smallest multiples of 16 that give eight -- 400 for hidden 3200, 512 for
    # the o projection, 1088 for the down projection.  `tools/llamagen_bench.py --sweep --preset GPT-3B` at 32 rows (profiles/llamagen_g1_sweep_3b.jsonl):
    # per projection the fastest shape with at most eight planes, us per launch q|k|v 12.83 (five planes), o 8.28, gate|up 20.81 (three planes),
    # down 13.69, head 19.51; against the smallest-chunk set (400, 2) / (512, 2) / (400, 2) / (1088, 2) + head (640, 4) the fused step goes
    # 2.19 -> 1.89 ms (profiles/llamagen_3b.json)
    (True, 64): (dict(qkv=(640, 8, True), o=(512, 4, False), gate_up=(1088, 8, True), down=(1088, 4, True)), (1088, 8, True)),
    # GPT-3B with several prompts per forward (enable_fused(pad_head_dim=True, padded_batch=True, max_rows=128 / 256)): the same rule at 128 and 256 rows --
    # `tools/llamagen_bench.py --sweep --preset GPT-3B --rows 128 / 256` (profiles/llamagen_g1_sweep_3b_128rows.jsonl, _256rows.jsonl), per projection the
    # fastest shape with at most eight planes (chunk >= 400 / 512 / 1088 for K = 3200 / 4096 / 8704) among kernel G1w's column-tile counts; us per launch
    # at 128 rows q|k|v 16.80 (three planes), o 9.68, gate|up 26.54, down 16.56, head 24.82 (two planes); at 256 rows 25.45, 14.40, 37.97, 23.14, 35.56.
    # (q|k|v's 9600 columns are 300 tiles: 75 workgroups of four; the head's 512 tiles by four; fp16 at 65..128 rows keeps the sub-tiled kernels on these shapes)
    (True, 128): (dict(qkv=(1088, 4, False), o=(512, 4, False), gate_up=(1088, 8, False), down=(1088, 4, True)), (1600, 4, True)),
    (True, 256): (dict(qkv=(1088, 4, False), o=(512, 4, True), gate_up=(1088, 8, True), down=(1088, 4, True)), (1600, 4, True)),
}
# LlamaGenBackbone.enable_fused(weights="e4m3" / "mxfp4" / their "_as_bf16" twins): the sets above with what ONE quantised copy needs to serve every row
# count up to max_rows (quant_copy_errors checks it) -- every chunk a multiple of Q4_GRANULE (320 -> 384; GPT-3B's 1088 -> 1152, which keeps its plane
# counts: 3 for K = 3200, 8 for K = 8704), <= CHUNK_CAP_64ROW so that 33..64 rows stage it as it is, and above 64 rows 3, 4, 6 or 8 column tiles per
# workgroup (two tiles have no form at 65..96 rows: o 2 -> 3, the other two-tile shapes -> 4).  One set per key serves both formats (128 is a multiple of
# e4m3's 32).  UNTUNED: no launch-shape sweep was run on either stream.  The output head is not quantised and keeps the HEAD_CFG of LLAMAGEN_SETS.
LLAMAGEN_QUANT_SETS = {
    (False, 64): (dict(qkv=(256, 2, True), o=(256, 2, False), gate_up=(384, 2, False), down=(512, 2, False)), (640, 4, True)),
    (False, 128): (dict(qkv=(384, 4, False), o=(256, 3, False), gate_up=(384, 4, True), down=(512, 4, False)), (640, 4, True)),
    (False, 256): (dict(qkv=(256, 4, False), o=(256, 3, False), gate_up=(384, 4, True), down=(512, 4, False)), (640, 4, True)),
    (True, 64): (dict(qkv=(640, 8, True), o=(512, 4, False), gate_up=(1152, 8, True), down=(1152, 4, True)), (1088, 8, True)),
    (True, 128): (dict(qkv=(1152, 4, False), o=(512, 4, False), gate_up=(1152, 8, False), down=(1152, 4, True)), (1600, 4, True)),
    (True, 256): (dict(qkv=(1152, 4, False), o=(512, 4, True), gate_up=(1152, 8, True), down=(1152, 4, True)), (1600, 4, True)),
}
# LlamaGenBackbone.enable_fused(compress=True): the LOSSLESS 12-bit stream (ops.pack_weight_z, kernels G1z / G1sz) for the four projections and the output
# head, up to Z_MAX_ROWS rows -- there is no key for 256.  UNTUNED: the 16-bit sets above with every chunk capped at Z_MAX_KC (none of them reaches it, so
# today these ARE the 16-bit shapes, which makes the two streams comparable launch for launch); no launch-shape sweep was run on the 12-bit kernels at
# LlamaGen's widths.  z_copy_errors is the rule they pass.
LLAMAGEN_Z_SETS = {(pad, rows): ({name: (min(kc, Z_MAX_KC), tiles, sm) for name, (kc, tiles, sm) in cfg.items()}, (min(head[0], Z_MAX_KC),) + tuple(head[1:]))
                   for (pad, rows), (cfg, head) in LLAMAGEN_SETS.items() if rows <= Z_MAX_ROWS}
Z_REASONS = ("rows", "granule", "chunk", "tiles")


def z_copy_errors(cfg, dims, max_rows, head_cfg=None):
    """[(name, why)]: what keeps a set of launch shapes `cfg` (dims: the projections' (N, K); head_cfg: the output head's shape, its (N, K) in dims["head"])
    from being packed as ONE 12-bit copy that serves every row count up to max_rows -- the first of Z_REASONS that applies to each matrix.  why: "rows"
    (max_rows above Z_MAX_ROWS: kernels G1z / G1sz end there), "granule" (N no multiple of 32, K or the chunk no multiple of 16: whole MFMA tiles and
    k-steps), "chunk" (above Z_MAX_KC: an exception's k-step is 7 + 1 bits of its position -- ops.pack_weight_z would decline the matrix), "tiles" (column
    tiles per workgroup outside 1..16, or above 8 where max_rows > 64: the sub-tiled kernel of 65..128 rows runs at most eight waves)."""
    bad = []
    for name, (KC, tiles, _) in list(cfg.items()) + ([("head", tuple(head_cfg))] if head_cfg is not None else []):
        N_, K_ = dims[name]
        fault = dict(rows=max_rows > Z_MAX_ROWS, granule=bool(N_ % 32 or K_ % 16 or KC % 16 or KC < 16), chunk=KC > Z_MAX_KC,
                     tiles=not 1 <= tiles <= (8 if max_rows > 64 else 16))
        bad += [(name, why) for why in Z_REASONS if fault[why]][:1]
    return bad


def z_copy_refusal(name, why, shape, dims):
    """the sentence enable_fused(compress=True) refuses with: one of z_copy_errors' (name, why), the launch shape it names and that matrix's (N, K)"""
    what = "HEAD_CFG" if name == "head" else f"G1_CFG[{name!r}]"
    return dict(rows=f"the 12-bit stream serves windows of at most {Z_MAX_ROWS} rows (kernels G1z / G1sz)",
                granule="the 12-bit stream travels in whole 32-column tiles and 16-wide k-steps (N a multiple of 32, K and the chunk multiples of 16)",
                chunk=f"the 12-bit stream takes chunks of at most {Z_MAX_KC} columns (an exception's k-step is 7 + 1 bits of its position)",
                tiles="kernel G1z takes 1..16 column tiles per workgroup, at most 8 where the copy serves more than 64 rows")[why] \
        + f"; {what} = {tuple(shape)} with (N, K) = {tuple(dims[name])}"


def llamagen_dims(dim, n_head, head_dim, inter, head_pad=None):
    """the (N, K) of a LlamaGen layer's four projections (multi-head attention; head_pad: the o projection reads heads stored that wide)"""
    return dict(qkv=(3 * n_head * head_dim, dim), o=(dim, n_head * (head_pad or head_dim)), gate_up=(2 * inter, dim), down=(dim, inter))


def chameleon_dims(hidden, n_heads, n_kv_heads, head_dim, inter):
    """the (N, K) of a Chameleon / Emu3 layer's four projections"""
    return dict(qkv=((n_heads + 2 * n_kv_heads) * head_dim, hidden), o=(hidden, n_heads * head_dim), gate_up=(2 * inter, hidden), down=(hidden, inter))


QUANT_REASONS = ("granule", "chunk", "halved", "tiles")


def quant_copy_errors(cfg, dims, max_rows, granule, head_cfg=None, reasons=QUANT_REASONS):
    """[(name, why)]: what keeps ONE quantised copy packed on launch shapes `cfg` (dims: the projections' (N, K)) from serving every row count up to
    max_rows -- the first of `reasons` that applies to each projection.  why: "granule" (K or the chunk no multiple of `granule`: Q4_GRANULE for MXFP4,
    32 for e4m3's record pairs), "chunk" (above CHUNK_CAP_32ROW: kernels G1q / G1q4 stage it whole), "halved" (none that 33..64 rows can stage:
    <= CHUNK_CAP_64ROW, or halvable by halved_chunk to whole granules), "tiles" (max_rows > 64: kernels G1wq / G1wq4 take 3, 4, 6 or 8 column tiles per
    workgroup -- two have no form at 65..96 rows; head_cfg, which streams 16-bit weights on kernel G1w, any of WIDE_TILES).  The caller passes the
    head_cfg and the reasons its call site checks when the weights are packed."""
    bad = []
    for name, (KC, tiles, sm) in cfg.items():
        K_ = dims[name][1]
        kc = min(KC, K_)
        half = halved_chunk(kc, K_, sm)
        fault = dict(granule=K_ % granule or KC % granule, chunk=KC > CHUNK_CAP_32ROW, halved=half > CHUNK_CAP_64ROW or half % granule,
                     tiles=max_rows > 64 and (tiles not in WIDE_TILES or tiles == 2))
        bad += [(name, why) for why in reasons if fault[why]][:1]
    if head_cfg is not None and max_rows > 64 and head_cfg[1] not in WIDE_TILES:
        bad.append(("head", "tiles"))
    return bad


def llamagen_quant_errors(cfg, dims, max_rows, granule=128, head_cfg=None):          # (the names the format tests call the rule by)
    return quant_copy_errors(cfg, dims, max_rows, granule, head_cfg)


def q4_chunk_errors(cfg, dims):
    return quant_copy_errors(cfg, dims, Q4_MAX_ROWS, Q4_GRANULE)


def quant_copy_refusal(name, why, granule, shape, K):
    """the sentence enable_fused refuses with: one of quant_copy_errors' (name, why), the launch shape it names and that projection's K"""
    if name == "head":
        return f"the output head runs on kernel G1w at these row counts -- HEAD_CFG[1] must be one of {WIDE_TILES}; HEAD_CFG = {tuple(shape)}"
    return dict(granule=f"K and the chunk must be multiples of {granule}",
                chunk=f"kernels G1q / G1q4 stage the whole activation chunk in LDS -- every chunk must be <= {CHUNK_CAP_32ROW} columns",
                halved=f"windows of 33..64 rows need a chunk of <= {CHUNK_CAP_64ROW} columns, or a step-major packing whose halved chunk is a multiple of {granule}",
                tiles="windows of more than 64 rows take 3, 4, 6 or 8 column tiles per workgroup on the quantised streams (kernels G1wq / G1wq4 have no form of "
                      "three row tiles x two tiles)")[why] + f"; G1_CFG[{name!r}] = {tuple(shape)} with K = {K}"


def default_shapes(dtype, g1_given, head_given, wide_hidden, gqa, compress, weights, max_rows, vocab_size):
    """(G1_CFG, HEAD_CFG) ChameleonBackbone.enable_fused packs with; *_given: the caller's (it wins); wide_hidden: 30B class; gqa: Emu3; None: the class default stays"""
    z = compress and dtype == torch.bfloat16          # the 12-bit stream
    head = head_given or (HEAD_CFG_WIDE if vocab_size >= 131072 else None)
    s = stream_of(weights)[0]          # (None also for a name no stream has: enable_fused has refused it by now, so the 16-bit sets below are never reached with one)
    if s is not None:          # (e2m3 at the 30B class takes the Q4 copy of G1_CFG_30B_Z where the Q8 copy used to be named: equal values, and no swin route reaches it; 30B class: swin-norm backbones, enable_fused(swin_quant=True), at most 64 rows; a stream without a wide form keeps its sets)
        plain, emu3, big, wide, emu3_wide = s.sets
        wide = (emu3_wide if gqa else wide) if (max_rows or 64) > 64 else None
        return g1_given or dict(big if wide_hidden else wide or (emu3 if gqa else plain)), head
    g1 = g1_given or (dict(G1_CFG_30B_Z if z else G1_CFG_30B) if wide_hidden else dict(G1_CFG_EMU3) if gqa else dict(G1_CFG_Z) if z else None)
    return (dict(G1_CFG_EMU3_Z) if z and g1 == G1_CFG_EMU3 else g1), head          # (also when the caller named Emu3's set: the packing follows the stream)


def halved_chunk(kc, K, step_major):
    """`kc` halved until it is <= CHUNK_CAP_64ROW, as far as the packing allows (the caller checks the result)"""
    while kc > CHUNK_CAP_64ROW and step_major and K % 32 == 0 and kc % 64 == 0:
        kc //= 2
    return kc


# Under enable_fused(weights=...) kernel G1q stages the whole activation chunk in LDS: <= CHUNK_CAP_32ROW columns up to 32 rows, <= CHUNK_CAP_64ROW at
# 33..64.  A projection packed with a longer chunk (G1_CFG_Q8's gate|up: two K halves of 2048, the copy the fused 32-row launch streams) is read at
# 33..64 rows in HALVED chunks until they fit: a step-major packing whose chunks are whole record pairs (K and the chunk multiples of 32) is the same
# bytes under either chunking -- pair after pair, every tile per pair.  The "e4m3_as_bf16" twin takes the same chunks (pack_weight's step-major stream
# has the same property), so the two stay bit-identical.
def chunk_for_rows(name, shape, T, K, weights=None, max_rows=64):
    """split-K chunk of projection `name` (launch shape `shape`) for a T-row window; ValueError where no such chunk exists"""
    KC, _, sm = shape
    if weights is None or T <= 32 or min(KC, K) <= CHUNK_CAP_64ROW or (T > 64 and max_rows > 64):          # (G1wq / G1w stream the activation in stages)
        return KC
    kc = halved_chunk(KC, K, sm)
    if kc > CHUNK_CAP_64ROW:
        raise ValueError(f"weights={weights!r}: a {T}-row window needs {name} chunks of <= {CHUNK_CAP_64ROW} columns (kernel G1q stages the chunk in LDS), or a "
                         f"step-major packing with K and the chunk multiples of 32 / 64 that halved chunks can read; G1_CFG[{name!r}] = {tuple(shape)}")
    return kc


def check_set(cfg, head_cfg, head_name="head"):
    """[(name, "tiles")]: the launch shapes of a 16-bit set (head_cfg: the output head's, or None) whose column-tile count kernel G1w does not take: what keeps
    the set from windows of more than 64 rows (a quantised copy: quant_copy_errors)"""
    return ([(name, "tiles") for name, (_, tiles, _) in cfg.items() if tiles not in WIDE_TILES]
            + [(head_name, "tiles")] * (head_cfg is not None and head_cfg[1] not in WIDE_TILES))


def llamagen_row_limit(backbone):
    """window rows a LlamaGen backbone can be asked for: fp16 keeps 128 unless it was packed for more (enable_fused(max_rows=256, untuned_fp16=True))"""
    return WINDOW_MAX_ROWS if backbone.output.weight.dtype == torch.bfloat16 or getattr(backbone, "max_rows", 64) >= WINDOW_MAX_ROWS else Z_MAX_ROWS


def is_llamagen(backbone):
    return hasattr(backbone, "tok_embeddings") and hasattr(backbone, "embed_condition")


def serves_rows(backbone, rows, window=1, head=False):
    """None when the packed `backbone` serves `rows` window rows (`window` per batch row) on the HIP path, else (why, detail): "unfused", "max_rows" / "fp16" (the
    rows it was packed for), "12-bit" (that stream's limit), "tiles" (check_set's names; head: the output head's too) or "prefill" (library GEMMs take it)"""
    if is_llamagen(backbone):          # LlamaGen: up to the rows its weights were packed for, whatever the stream (enable_fused(weights=...): G1wq / G1wq4 above 64)
        if getattr(backbone, "_ops", None) is None:
            return "unfused", None
        limit, fp16 = getattr(backbone, "max_rows", 64), backbone.output.weight.dtype == torch.float16 and rows > Z_MAX_ROWS
        return ("fp16" if fp16 else "max_rows", limit) if rows > limit else None
    weights, packed = getattr(backbone, "weights", None), getattr(backbone, "_packed", None)
    (s, twin), limit = stream_of(weights), getattr(backbone, "max_rows", 64) if weights is not None else 64
    if s is not None and s.max_rows > 64 and not twin and limit < rows <= WINDOW_MAX_ROWS and window <= 32:
        return "max_rows", limit
    if s is not None and rows > s.max_rows <= 64:          # (neither a copy without a wide form nor its twin was packed for more: there is no other copy to serve them)
        return ("max_rows", s.max_rows) if rows <= WINDOW_MAX_ROWS and window <= 32 else ("prefill", None)
    if getattr(backbone, "_gemm", None) != "sjd" or rows > WINDOW_MAX_ROWS or (rows > 64 and window > 32) or (rows > Z_MAX_ROWS and not packed):
        return "prefill", None
    if rows <= Z_MAX_ROWS:
        return None
    if isinstance(packed[0]["qkv"], backbone._ops.PackedZ):
        return "12-bit", Z_MAX_ROWS
    bad = check_set(backbone.G1_CFG, backbone.HEAD_CFG if head and getattr(backbone, "_packed_head", None) is not None else None, head_name="lm_head (HEAD_CFG)")
    return ("tiles", [name for name, _ in bad]) if bad else None


# shapes kernel G1s serves (see sjd_gateup_silu): a <= 32-row window -- or a <= 64-row one (draft window 32 with CFG, two prompts per forward) at
# hidden >= 1024, or a <= 128-row one (three / four prompts per forward) at hidden 4096 over the uncompressed packing --, the gate|up weight packed in
# two K halves; over the 8-bit packing (packed_q8: kernel G1sq) a <= 32-row window only
def gateup_silu_ok(T, inter, hidden, KC, packed_z=False, packed_q8=False):
    rows_ok = T <= 32 or (not packed_q8 and ((T <= 64 and hidden >= 1024) or (T <= Z_MAX_ROWS and hidden == 4096 and not packed_z)))
    return rows_ok and hidden in (512, 1024, 2048, 4096) and 2 * KC == hidden and inter % 64 == 0


# the one shape the fused gate|up launch serves from a copy packed in MORE than two chunks (sjd_gateup_silu with SJD_G1S_CHUNKS(4), kernel
# g1q4_gateup_silu_k4): a <= 32-row window at hidden 8192 over the MXFP4 copy that G1q4 streams in four chunks of 2048.  The e4m3 stream has no such form.
def gateup_silu_chunked_ok(T, inter, hidden, KC, packed_q4=True):
    return bool(packed_q4) and T <= 32 and hidden == 8192 and KC == 2048 and inter % 64 == 0


def packed_nbytes(w):
    """bytes of one packed weight: a tensor (pack_weight) or an ops.Packed (the 12-bit stream, a row of STREAMS), which knows its own"""
    return w.numel() * w.element_size() if isinstance(w, torch.Tensor) else w.nbytes()
