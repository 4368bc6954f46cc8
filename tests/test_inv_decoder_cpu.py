"""decoder_type "deepsdf" (the invariant-decoder ablation) on the host side: weight packing and checkpoint loading (no GPU)."""
import numpy as np
import pytest
import torch
import yaml

from livingscenes_amd import _lib, packing, synth


def _folded_ref(dec_w, cfg, layer):
    """The reference's weight-normed layer (nn.utils.weight_norm, dim 0: W = g v / |v|_row) in fp64."""
    if cfg["weight_norm"] and layer in cfg["norm_layers"]:
        g, v = dec_w[f"lin{layer}.weight_g"].double(), dec_w[f"lin{layer}.weight_v"].double()
        return (g * v / v.norm(dim=1, keepdim=True)).numpy()
    return dec_w[f"lin{layer}.weight"].double().numpy()


def _tab(blob, off, shape):
    return blob[off:off + int(np.prod(shape))].reshape(shape).astype(np.float64)


@pytest.mark.parametrize("which", ["ablation", "small"])
def test_pack_model_invariant_decoder_folds(which):
    ecfg, dcfg = ((synth.default_encoder_cfg(), synth.inv_decoder_cfg()) if which == "ablation"
                  else (synth.small_encoder_cfg(), synth.small_inv_decoder_cfg()))
    ew, dw = synth.make_encoder_weights(ecfg, 0), synth.make_decoder_weights(dcfg, 0)
    d, blob = packing.pack_model(ew, ecfg, dw, dcfg)
    lat, width, li = dcfg["latent_size"], dcfg["dims"][0], dcfg["latent_in"][0]
    u = lat + 3
    assert d.dec_input == _lib.DEC_XYZ and d.dec_width == width and d.dec_latent_in == li and d.dec_num_linear == len(dcfg["dims"]) + 1
    hprev = width - u
    pad = (hprev + 3) // 4 * 4
    for layer in (0, li):
        W = _folded_ref(dw, dcfg, layer)
        code_cols = W[:, -u:] if layer == li else W
        assert np.abs(_tab(blob, d.off_dec_inv_t[layer], (lat, width)) - code_cols[:, :lat].T).max() < 1e-6
        assert np.abs(_tab(blob, d.off_dec_xyz_t[layer], (3, width)) - code_cols[:, lat:].T).max() < 1e-6
        assert np.abs(_tab(blob, d.off_dec_b[layer], (width,)) - dw[f"lin{layer}.bias"].double().numpy()).max() < 1e-6
    # the layer before the skip: hprev = width - u outputs, zero-padded to a multiple of 4 rows
    W3 = _folded_ref(dw, dcfg, li - 1)
    assert W3.shape == (hprev, width)
    w3p, b3p = _tab(blob, d.off_dec_w[li - 1], (pad, width)), _tab(blob, d.off_dec_b[li - 1], (pad,))
    assert np.abs(w3p[:hprev] - W3).max() < 1e-6 and not w3p[hprev:].any()
    assert np.abs(b3p[:hprev] - dw[f"lin{li - 1}.bias"].double().numpy()).max() < 1e-6 and not b3p[hprev:].any()
    # the skip layer: its h part [width, hprev] zero-padded to pad columns
    W4 = _folded_ref(dw, dcfg, li)
    w4p = _tab(blob, d.off_dec_w[li], (width, pad))
    assert np.abs(w4p[:, :hprev] - W4[:, :hprev]).max() < 1e-6 and not w4p[:, hprev:].any()
    # the plain hidden layers and the last one
    for layer in range(1, len(dcfg["dims"]) + 1):
        if layer in (li - 1, li):
            continue
        W = _folded_ref(dw, dcfg, layer)
        assert np.abs(_tab(blob, d.off_dec_w[layer], W.shape) - W).max() < 1e-6, layer


def test_pack_model_released_decoder_keeps_the_inner_kind():
    ecfg, dcfg = synth.small_encoder_cfg(), synth.small_decoder_cfg()
    d, _ = packing.pack_model(synth.make_encoder_weights(ecfg, 0), ecfg, synth.make_decoder_weights(dcfg, 0), dcfg)
    assert d.dec_input == _lib.DEC_INNER and list(d.off_dec_xyz_t) == [0] * 12
    bad = dict(dcfg, pe_dim=5)
    with pytest.raises(AssertionError):
        packing.pack_model(synth.make_encoder_weights(ecfg, 0), ecfg, synth.make_decoder_weights(bad, 0), bad)


def test_inv_decoder_cfg_is_the_ablation_shape():
    cfg = synth.inv_decoder_cfg()
    assert cfg["latent_size"] == 256 and cfg["pe_dim"] == 3 and cfg["dims"] == [512] * 8 and cfg["latent_in"] == [4]
    assert cfg["weight_norm"] and cfg["norm_layers"] == list(range(8))
    dims = synth.decoder_layer_dims(cfg)
    assert dims[0] == (259, 512) and dims[3] == (512, 253) and dims[4] == (512, 512) and dims[8] == (512, 1)


def _write_log(tmp_path, ecfg, dcfg, decoder_type, ew, dw):
    (tmp_path / "checkpoint").mkdir(exist_ok=True)
    (tmp_path / "files_backup").mkdir(exist_ok=True)
    torch.save(synth.to_checkpoint(ew, dw, epoch=5), tmp_path / "checkpoint" / "x_latest.pt")
    field = {"model": {"encoder": ecfg, "decoder": dcfg, "encoder_type": "vecdgcnn_atten", "decoder_type": decoder_type,
                       "sdf2occ_factor": -1.0}, "dataset": {"n_pcl": 256}}
    (tmp_path / "files_backup" / "model_config.yaml").write_text(yaml.safe_dump(field))
    return {"working_dir": "/", "field_cfg": str(tmp_path / "files_backup" / "model_config.yaml"),
            "field_pt": str(tmp_path / "checkpoint" / "x_latest.pt")}


def test_shape_prior_loads_a_deepsdf_checkpoint(tmp_path):
    from livingscenes_amd.model_utils import Shape_Prior
    ecfg, dcfg = synth.small_encoder_cfg(), synth.small_inv_decoder_cfg()
    ew, dw = synth.make_encoder_weights(ecfg, 3), synth.make_decoder_weights(dcfg, 3)
    sp = Shape_Prior(_write_log(tmp_path, ecfg, dcfg, "deepsdf", ew, dw), "chair", use_double=False)
    assert sp.decoder_type == "deepsdf" and sp.decoder.decoder_type == "deepsdf" and sp.decoder.sdf2occ_factor == -1.0
    sd = sp.decoder.F.state_dict()
    assert set(sd) == set(dw)
    for layer in range(len(dcfg["dims"]) + 1):
        wn = layer in dcfg["norm_layers"]
        assert (f"lin{layer}.weight_g" in sd) == wn and (f"lin{layer}.weight" in sd) == (not wn)
        for k in (("weight_g", "weight_v", "bias") if wn else ("weight", "bias")):
            assert torch.equal(sd[f"lin{layer}.{k}"], dw[f"lin{layer}.{k}"]), (layer, k)
    for k, v in ew.items():
        assert torch.equal(sp.encoder.state_dict()[k], v)


@pytest.mark.parametrize("dtype", ["inner", "decoder", "cbatchnorm", "inv_mlp"])
def test_unsupported_decoder_types_still_raise(tmp_path, dtype):
    from livingscenes_amd.model_utils import Shape_Prior
    ecfg, dcfg = synth.small_encoder_cfg(), synth.small_inv_decoder_cfg()
    cfg = _write_log(tmp_path, ecfg, dcfg, dtype, synth.make_encoder_weights(ecfg, 3), synth.make_decoder_weights(dcfg, 3))
    with pytest.raises(NotImplementedError, match="inner_deepsdf.*deepsdf"):
        Shape_Prior(cfg, "chair", use_double=False)
    with pytest.raises(NotImplementedError):
        Shape_Prior.from_state(ecfg, dcfg, {}, {}, device="cpu", decoder_type=dtype)


def test_decoder_type_must_match_the_query_width(tmp_path):
    """A released-shape decoder (pe_dim = latent + 1) under decoder_type "deepsdf", or the reverse, is refused."""
    from livingscenes_amd.model_utils import Shape_Prior
    ecfg = synth.small_encoder_cfg()
    for dcfg, dtype in ((synth.small_decoder_cfg(), "deepsdf"), (synth.small_inv_decoder_cfg(), "inner_deepsdf")):
        cfg = _write_log(tmp_path, ecfg, dcfg, dtype, synth.make_encoder_weights(ecfg, 3), synth.make_decoder_weights(dcfg, 3))
        with pytest.raises(ValueError, match="pe_dim"):
            Shape_Prior(cfg, "chair", use_double=False)
