"""Draft-window attention (K1) held to exact answers: the key census and the dominant-key probes of tests/attention_probe_cases.py on every K1
form of the product library (k1_partial with 8 / 4 / 1 key-parts, D = 64, head-dim 100, several chunks; k1_partial_ring with 4 / 8 pairs;
k1_dsplit, k1_dsplit_fp8, k1_partial_fp8, k1_f32; k1_combine against the direct output at 1 / 4 / 8 (16) key splits).

A census launch counts which keys were attended to, each exactly once: round(out N) == c_d as integers.  A dominant launch must return V[j*]
(the mean of tied rows) bit for bit.  Every launch goes through ops.draft_window_attention*, on a NaN-filled workspace, twice into
differently poisoned outputs.  tests/test_attention_probe_cases.py is the CPU evidence that the zero tolerance is legitimate.
"""
import pytest
import torch

from tests import attention_probe_cases as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _ops():
    import sjd_amd.ops as ops
    import sjd_amd._lib as L
    L.load()
    return ops, L


_REACHED = {}           # kernel detail -> set of probes that reached it
_RAN = set()


def _params_of(ops, L, dev, geo):
    if not geo["blob"]:
        return None
    if geo["nb"]:
        nb = geo["nb"]
        arr = ops.BlobArray(L.IterParams, geo["B"] // nb, dev)
        for j in range(geo["B"] // nb):
            view = arr.blobs[j].view
            view.kv_len, view.n_rows, view.batch_rows = int(geo["kv"][j * nb]), int(geo["nv"][j * nb]), nb
        arr.upload()
        return arr
    blob = ops.DeviceBlob(L.IterParams, dev)
    blob.view.kv_len, blob.view.n_rows = int(geo["kv"][0]), int(geo["nv"][0])
    blob.upload()
    return blob


def _launch(ops, dev, form, geo, inp, n_split, params, poison):
    q, kc, vc = inp["q"].to(dev), inp["kc"].to(dev), inp["vc"].to(dev)
    ks = torch.tensor(geo["ks"], dtype=torch.int32, device=dev)
    out = torch.full_like(q, poison)
    kv = -1 if params is not None else geo["kv"][0]
    B, n, H, D = q.shape
    if form["colsplit"]:
        assert ops.colsplit_ok(B, n, H, form["Hkv"], D, kc.dtype)
        ops.draft_window_attention_colsplit(q, kc, vc, out, ks, params, kv, kv_scale=form["scales"], head_dim=form["head_dim"])
    else:
        ws = ops.attention_workspace(B, H, n, D, n_split, dev).fill_(float("nan"))
        if form["cache"] == "fp8":
            ops.draft_window_attention_fp8(q, kc, vc, out, form["scales"][0], form["scales"][1], ks, params, kv, n_split, ws, merged=False)
        else:
            ops.draft_window_attention(q, kc, vc, out, ks, params, kv, n_split, ws, merged=False, head_dim=form["head_dim"])
    torch.cuda.synchronize()
    return out.cpu()


def _run(dev, form, rng, layouts=P.LAYOUTS, splits=None):
    ops, L = _ops()
    geo = P.geometry(form, rng)
    assert geo["S"] <= 1312 or rng["name"] == "kv4101"
    params = _params_of(ops, L, dev, geo)
    ran = {"census": 0, "dominant": 0}
    excess = []
    for n_split in splits or P.splits_of(form):
        r = P.route(form, n_split)
        for probe, layout in [("census", None)] + [("dominant", lay) for lay in layouts]:
            inp = P.build(form, geo, probe, layout, n_split)
            if isinstance(inp, str):
                continue
            a = _launch(ops, dev, form, geo, inp, n_split, params, 7.0)
            b = _launch(ops, dev, form, geo, inp, n_split, params, float("nan"))
            view = torch.int32 if a.dtype == torch.float32 else torch.int16
            what = f"{form['name']} {rng['name']} {n_split} splits [{r['detail']}] {layout or 'census'}"
            assert torch.equal(a.view(view), b.view(view)), f"{what}: a repeated launch gave other bytes"
            if probe == "census":
                fails = P.census_failures(form, geo, inp["expect"], a.double().numpy())
                if form["dtype"] != "f32":
                    excess.append(P.census_literal_excess(form, inp["expect"], a.double().numpy()))
            else:
                fails = P.dominant_failures(form, geo, inp["expect"], a)
            assert not fails, what + ":\n  " + "\n  ".join(fails)
            ran[probe] += 1
            for det in [r["detail"]] + (["k1_combine"] if r["combine"] else []):
                _REACHED.setdefault(det, set()).add(probe)
    if excess:
        print(f"\n  {form['name']} {rng['name']}: share of census outputs beyond (u / 2 + 2^-22) c / N: {max(excess):.3f} (half an ulp is up to u c / N)")
    assert ran["census"] and ran["dominant"], f"{form['name']} {rng['name']}: no probe applied"
    _RAN.add((form["name"], rng["name"]))


def _grid():
    return [pytest.param(f, r, id=f"{f['name']}-{r['name']}") for f in P.FORMS for r in P.ranges_of(f)]


@pytest.mark.parametrize("form,rng", _grid())
def test_k1_probes(dev, form, rng):
    """every form x key range: the census and every dominant-key layout that applies, at every key-split count of the form"""
    _run(dev, form, rng)


@pytest.mark.parametrize("name", ["partial8_bf16", "dsplit_bf16", "fp8_mha"])
def test_k1_probes_blob_array(dev, name):
    """four slots of different kv_len / n_rows in one launch (the path of test_k1_k3_blob_array): another slot's length is a wrong count"""
    _run(dev, P.FORM[name], P.BLOB_ARRAY_RANGE, layouts=["own_key", "hostile_invisible", "stair_up"])


def test_k1_probes_ring_130_tiles_over_16_splits(dev):
    """Emu3's window late in an image on the ring kernel in fp16: 130 tiles over 16 splits of 9, the sixteenth gets none"""
    _run(dev, P.FORM["ring8_n32"], P.RING_4101_RANGE, splits=[16])


def test_every_form_was_reached():
    """every named kernel form is reached by a census and by a dominant-key case: by the table (the dispatch restated in P.route) and, when the
    whole module ran, by the launches recorded"""
    table = {}
    for f in P.FORMS:
        for s in P.splits_of(f):
            r = P.route(f, s)
            for det in [r["detail"]] + (["k1_combine"] if r["combine"] else []):
                table.setdefault(det, set()).update(("census", "dominant"))
    missing = [d for d in P.REQUIRED_DETAILS if table.get(d) != {"census", "dominant"}]
    assert not missing, missing
    if len(_RAN) >= len(_grid()):
        missing = [d for d in P.REQUIRED_DETAILS if _REACHED.get(d) != {"census", "dominant"}]
        assert not missing, (missing, _REACHED)
        print("\n  reached: " + ", ".join(sorted(_REACHED)))
