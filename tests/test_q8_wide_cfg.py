"""CPU: the default launch-shape sets of enable_fused(weights=..., max_rows=128 / 256) pass its validation arithmetic at the real Lumina-mGPT-7B and
Emu3-Gen-8B shapes -- ONE 8-bit packed copy must serve every row count: G1q / G1sq up to 32 rows (chunks <= 2560), G1q at 33..64 (chunks of <= 1280
that the packing reads_as), G1wq at 65..256 (wide tile counts, K and the chunks multiples of 32).  No real-size weights: the backbones live on the
meta device."""
import pytest
import torch

import sjd_amd.backbones as BB
import sjd_amd.ops as ops


def _meta(args):
    with torch.device("meta"):
        return BB.ChameleonBackbone(args)


def _dims(a):
    D = a.hidden_size // a.num_attention_heads
    return dict(qkv=((a.num_attention_heads + 2 * a.num_key_value_heads) * D, a.hidden_size), o=(a.hidden_size, a.num_attention_heads * D),
                gate_up=(2 * a.intermediate_size, a.hidden_size), down=(a.hidden_size, a.intermediate_size))


@pytest.mark.parametrize("args,cfg_name", [(BB.LUMINA_7B, "G1_CFG_Q8_WIDE"), (BB.EMU3_8B, "G1_CFG_EMU3_Q8_WIDE")])
def test_default_wide_sets_serve_every_row_count(args, cfg_name):
    m = _meta(args)
    cfg = getattr(m, cfg_name)
    head = m.HEAD_CFG_WIDE if args.vocab_size >= 131072 else m.HEAD_CFG
    for max_rows in (128, 256):
        m._q8_wide_check(cfg, head, max_rows)                                  # what enable_fused runs, on the backbone's own shapes
    m.weights, m.G1_CFG = "e4m3", dict(cfg)
    for name, (N, K) in _dims(args).items():
        KC, tiles, sm = cfg[name]
        assert tiles in m.G1_WIDE_TILES and tiles != 2                         # 65..96 rows have no two-tile form
        assert K % 32 == 0 and KC % 32 == 0 and KC <= 2560 and N % 32 == 0
        pq = ops.PackedQ8(None, N, K, KC, sm)                                  # (reads_as is arithmetic on the packing's shape)
        m.max_rows = 256
        assert m._q8_chunk(name, 32, K) == KC
        kc64 = m._q8_chunk(name, 64, K)
        assert min(kc64, K) <= 1280 and kc64 % 32 == 0 and pq.reads_as(kc64)
        for rows in (65, 96, 128, 129, 256):
            assert m._q8_chunk(name, rows, K) == KC
        m.max_rows = 64                                                        # without max_rows the taller windows keep the halved chunks
        assert m._q8_chunk(name, 128, K) == kc64
    if cfg["gate_up"][0] * 2 == args.hidden_size:                              # the 32-row window keeps the fused gate|up launch
        assert ops.gateup_silu_ok(32, args.intermediate_size, args.hidden_size, cfg["gate_up"][0], packed_q8=True)
    assert head[1] in m.G1_WIDE_TILES


def test_wide_check_refusals():
    m = _meta(BB.LUMINA_7B)
    good = m.G1_CFG_Q8_WIDE
    for bad, what in ((dict(good, o=(1024, 2, True)), "column tiles"), (dict(good, qkv=(2048, 5, True)), "column tiles"),
                      (dict(good, down=(1408, 4, False)), "<= 1280"), (dict(good, down=(1376, 4, True)), "<= 1280"),      # 1376 / 2 = 688 is no multiple of 32
                      (dict(good, o=(528, 4, True)), "multiples of 32")):
        with pytest.raises(ValueError, match=what):
            m._q8_wide_check(bad, m.HEAD_CFG, 256)
    with pytest.raises(ValueError, match="HEAD_CFG"):
        m._q8_wide_check(good, (1024, 5, True), 256)
    m._q8_wide_check(good, (1024, 5, True), 128)                               # up to 128 rows the head keeps its own kernels
    assert "weights" not in m.__dict__ and "max_rows" not in m.__dict__
