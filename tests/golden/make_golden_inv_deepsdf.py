#!/usr/bin/env python3
"""Generate tests/golden/inv_deepsdf.npz: decoder_type "deepsdf" (the invariant-decoder ablation,
lib_shape_prior/configs/decoder/dgcnn_attn_inv_deepsdf.yaml) through the reference's UNMODIFIED model_utils.Shape_Prior.

    python tests/golden/make_golden_inv_deepsdf.py      # rewrites tests/golden/inv_deepsdf.npz

Same recipe as make_golden.py section 3 (its stubs are imported, not copied): the reference modules are loaded by path, the
weights are the deterministic synthetic ones (livingscenes_amd.synth, seed 0).  Two configurations, keys prefixed "full_"
(the ablation yaml as shipped) and "small_" (synth.small_encoder_cfg + synth.small_inv_decoder_cfg):
  z_so3, z_inv, s, t        the codes of 2 instances (Shape_Prior.encode, fp32)
  query                     2 x 256 world-frame queries
  sdf                       FieldWrapper.forward(query, None, code, return_sdf=True)
  w, g_query, g_z_inv       fixed weights w and the autograd gradients of sum(w * sdf) w.r.t. query and z_inv
  none_grads                [z_so3, s, t].grad is None after that backward (1 = None)
Data only: nothing from the reference's source text is stored.
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch
import yaml

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (stubs, loader, REF, REPO on sys.path)
from livingscenes_amd import synth  # noqa: E402

YAML = "lib_shape_prior/configs/decoder/dgcnn_attn_inv_deepsdf.yaml"


def load_reference_model_utils():
    mg.install_stubs()
    VS = "lib_shape_prior/core/lib/vec_sim3/"
    IF = "lib_shape_prior/core/lib/implicit_func/"
    mg.load_by_path("vec_layers", VS + "vec_layers.py")
    att = mg.load_by_path("ref_vec_dgcnn_atten", VS + "vec_dgcnn_atten.py")
    dsdf = mg.load_by_path("ref_deepsdf_decoder", IF + "deepsdf_decoder.py")
    sys.path.insert(0, mg.REF)
    for dotted in ["lib_shape_prior", "lib_shape_prior.core", "lib_shape_prior.core.lib",
                   "lib_shape_prior.core.lib.implicit_func", "lib_shape_prior.core.lib.vec_sim3",
                   "lib_shape_prior.core.models", "lib_shape_prior.core.models.utils",
                   "lib_shape_prior.core.models.utils.occnet_utils"]:
        m = types.ModuleType(dotted)
        m.__path__ = []
        sys.modules[dotted] = m
    mg.load_by_path("lib_shape_prior.core.lib.implicit_func.onet_decoder", IF + "onet_decoder.py")
    sys.modules["lib_shape_prior.core.lib.implicit_func.deepsdf_decoder"] = dsdf
    mg.load_by_path("lib_shape_prior.core.lib.vec_sim3.vec_dgcnn", VS + "vec_dgcnn.py")
    sys.modules["lib_shape_prior.core.lib.vec_sim3.vec_dgcnn_atten"] = att
    mg.load_by_path("lib_shape_prior.core.lib.vec_sim3.pcnet", VS + "pcnet.py")
    me = types.ModuleType("lib_shape_prior.core.models.utils.occnet_utils.mesh_extractor2")
    me.Generator3D = object
    sys.modules[me.__name__] = me
    import model_utils  # the reference's file, unmodified
    return model_utils


def record(model_utils, field_cfg, ecfg, dcfg, td, tag):
    enc_w, dec_w = synth.make_encoder_weights(ecfg, seed=0), synth.make_decoder_weights(dcfg, seed=0)
    ck, yp = os.path.join(td, tag + ".pt"), os.path.join(td, tag + ".yaml")
    torch.save(synth.to_checkpoint(enc_w, dec_w), ck)
    with open(yp, "w") as f:
        yaml.safe_dump(field_cfg, f)
    sp = model_utils.Shape_Prior({"working_dir": "/", "field_cfg": yp, "field_pt": ck}, "chair", use_double=False).eval()
    assert sp.decoder_type == "deepsdf"
    xi = synth.make_instances(2, 1024, seed=0)
    with torch.no_grad():
        emb = sp.encode(xi)
    q = (synth.make_queries(2, 256, seed=0) * emb["s"][:, None, None] + emb["t"]).detach()
    with torch.no_grad():
        sdf = sp.decoder(q, None, emb, return_sdf=True)
    w = torch.from_numpy(np.random.Generator(np.random.Philox(key=[0, 4242])).uniform(-1.0, 1.0, (2, 256)).astype(np.float32))
    code = {k: v.detach().clone().requires_grad_(True) for k, v in emb.items()}
    qg = q.clone().requires_grad_(True)
    (w * sp.decoder(qg, None, code, return_sdf=True)).sum().backward()
    none = np.array([code[k].grad is None for k in ("z_so3", "s", "t")], dtype=np.int8)
    assert none.all(), "the invariant decoder must leave z_so3 / s / t without a gradient"
    out = {"z_so3": emb["z_so3"], "z_inv": emb["z_inv"], "s": emb["s"], "t": emb["t"], "query": q, "sdf": sdf, "w": w,
           "g_query": qg.grad, "g_z_inv": code["z_inv"].grad, "none_grads": none}
    return {f"{tag}_{k}": v for k, v in mg.t2n(out).items()}


def main():
    torch.set_num_threads(8)
    torch.manual_seed(0)
    model_utils = load_reference_model_utils()
    with open(os.path.join(mg.REF, YAML)) as f:
        abl = yaml.full_load(f)
    ecfg, dcfg = synth.default_encoder_cfg(), synth.inv_decoder_cfg()
    assert abl["model"]["decoder_type"] == "deepsdf" and abl["model"]["encoder_type"] == "vecdgcnn_atten"
    assert {k: abl["model"]["encoder"][k] for k in ecfg} == ecfg, "synth encoder cfg != ablation config"
    assert abl["model"]["decoder"] == dcfg, "synth.inv_decoder_cfg() != the ablation yaml's model.decoder"
    small = {"model": dict(abl["model"], encoder=synth.small_encoder_cfg(), decoder=synth.small_inv_decoder_cfg()),
             "dataset": dict(abl["dataset"])}
    out = {}
    with tempfile.TemporaryDirectory() as td:
        out.update(record(model_utils, abl, ecfg, dcfg, td, "full"))
        out.update(record(model_utils, small, synth.small_encoder_cfg(), synth.small_inv_decoder_cfg(), td, "small"))
    np.savez_compressed(os.path.join(HERE, "inv_deepsdf.npz"), **out)


if __name__ == "__main__":
    main()
