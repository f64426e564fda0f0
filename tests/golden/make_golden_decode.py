#!/usr/bin/env python3
"""Generate the tokens -> pixels fixture of the Lumina-mGPT solver by IMPORTING THE REFERENCE in this container (CPU), as make_golden.py does.

Run:  python tests/golden/make_golden_decode.py          (writes decode_images.npz)

The reference's `FlexARItemProcessor.decode_image` (lumina_mgpt/data/item_processor.py:179-211) is called, unmodified, on a stub `self`
that carries what the method reads: the ids of the start / end tokens, patch_size, the device, an explicit BPE id -> VQ code table
(`chameleon_ori_translation.bpe2img`, a dict as in the reference) and the reference's own `ImageTokenizer` around the reference's own
`VQModel` at a small width with per-key synthetic weights (sjd_amd.synthetic.fill_state_dict_conv).  Two image spans: a 4 x 6 latent
(2 x 3 grids) and a 2 x 2 latent (1 x 1 grids).

What is restated here instead of imported: the CONSTRUCTORS of FlexARItemProcessor (it opens ./ckpts/chameleon/tokenizer/*.json and the
tokenizer of the hub) and of ImageTokenizer (it opens vqgan.yaml / vqgan.ckpt) -- the stub / `__new__` below set the attributes they
would set.  The decode path itself (decode_image, pil_from_img_toks, get_codebook_entry, VQModel.decode, _pil_from_chw_tensor) is the
reference's code.  The fixture's meta says so.

Only inputs (seeds, small integer arrays) and the reference's outputs are written; nothing at test time imports this script.
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (installs the reference shims; its sys.path rules apply)

START, END, LINE, GRID_BASE = 8197, 8196, 8803, 8804
N_CODES, SEED = 80, 21
DD = dict(double_z=False, z_channels=32, resolution=32, in_channels=3, out_ch=3, ch=32, ch_mult=[1, 2, 2], num_res_blocks=2,
          attn_resolutions=[8], dropout=0.0)


def _item_processor_class():
    """data.item_processor imports the conversation template and the xllmx data readers at module level; only decode_image is wanted"""
    for name in ("data.convertsation", "xllmx.data.data_reader", "xllmx.data.item_processor"):
        try:
            __import__(name)
        except Exception:                                   # a dependency of a module decode_image never touches
            mod = types.ModuleType(name)
            mod.Conversation, mod.read_general, mod.MMConvItemProcessor = object, None, object
            sys.modules[name] = mod
            parent, _, leaf = name.rpartition(".")
            if parent in sys.modules:
                setattr(sys.modules[parent], leaf, mod)
    from data.item_processor import FlexARItemProcessor
    return FlexARItemProcessor


def gen_decode_images():
    sys.path.insert(0, "/root/reference/lumina_mgpt")
    from model.chameleon_vae_ori import vqgan as CV
    from model.chameleon_vae_ori.image_tokenizer import ImageTokenizer
    IP = _item_processor_class()

    vq = CV.VQModel(ddconfig=DD, n_embed=N_CODES, embed_dim=16).eval()
    MG.synthetic.fill_state_dict_conv(vq, seed=SEED)
    tok = ImageTokenizer.__new__(ImageTokenizer)            # the constructor restated: it reads vqgan.yaml / vqgan.ckpt
    tok._vq_model, tok._device, tok._dtype = vq, "cpu", torch.float32

    # an explicit table that is NOT id - 4: image id t -> code (7 t + 3) mod 80
    table = np.full(8197, -1, dtype=np.int64)
    table[4:8196] = (7 * np.arange(4, 8196) + 3) % N_CODES
    bpe2img = {int(t): int(table[t]) for t in range(4, 8196)}

    class Stub:                                             # FlexARItemProcessor's constructor restated: the attributes decode_image reads
        image_start_token, image_end_token = IP.image_start_token, IP.image_end_token
        patch_size = 32
        device = "cpu"
        chameleon_ori_translation = types.SimpleNamespace(bpe2img=bpe2img)
        chameleon_ori_image_tokenizer = tok

        @staticmethod
        def token2id(token):
            return {IP.image_start_token: START, IP.image_end_token: END}[token]

    out = {}
    g = torch.Generator().manual_seed(5)
    cases = []
    for name, (hg, wg) in (("a", (2, 3)), ("b", (1, 1))):
        h_lat, w_lat = 2 * hg, 2 * wg
        body = torch.randint(4, 8196, (h_lat, w_lat), generator=g)
        body = torch.cat([body, torch.full((h_lat, 1), LINE)], dim=1).flatten().tolist()
        tokens = [START, GRID_BASE + hg, GRID_BASE + wg] + body + [END]
        with torch.no_grad():
            pil = IP.decode_image(Stub(), list(tokens))
        img = np.asarray(pil)
        assert img.dtype == np.uint8 and img.shape == (4 * h_lat, 4 * w_lat, 3), img.shape      # (three levels: 4 pixels per code)
        out[f"{name}_tokens"], out[f"{name}_image"] = np.asarray(tokens, dtype=np.int64), img
        cases.append(dict(name=name, h_grids=hg, w_grids=wg, h_latent=h_lat, w_latent=w_lat))
    dec_keys = {k: list(v.shape) for k, v in vq.state_dict().items() if not k.startswith(("encoder.", "quant_conv.", "loss."))}
    meta = dict(cases=cases, seed=SEED, keys=dec_keys,
                kwargs=dict(n_embed=N_CODES, embed_dim=16, z_channels=32, ch=32, ch_mult=[1, 2, 2], num_res_blocks=2, attn_resolutions=[8],
                            resolution=32),
                restated="the constructors of FlexARItemProcessor and ImageTokenizer (they open tokenizer / VQGAN files): a stub self and "
                         "ImageTokenizer.__new__ carry the attributes; decode_image, pil_from_img_toks and VQModel are the reference's code")
    np.savez_compressed(os.path.join(HERE, "decode_images.npz"), bpe_to_vq=table, meta=np.array(json.dumps(meta)), **out)
    print("decode_images.npz", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    gen_decode_images()
