"""What the GPU tests of the scene memory's operators share (tests/test_hip_cloud_{merge,nearest,icp,plane}.py): the device and conversion
helpers, random poses, the scan's tile from ls_scan.h, and the small solver, prior and scene of the solve_sequence tests with the key sets
of a step.  A plain module: the test files import what they use by name, the fixture small_prior included."""
import os
import re

import numpy as np
import pytest
import torch

from livingscenes_amd import synth

REPO = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
F = np.float32


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32).reshape(-1, 3)).to(_dev())


def _g(g):
    return None if g is None else torch.from_numpy(np.ascontiguousarray(g, dtype=np.float32)).to(_dev())


def _bits(x):
    return np.ascontiguousarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x).view(np.uint32)


def _rot(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    return q * np.sign(np.linalg.det(q))


def _pose(rng, t=1.0):
    return np.concatenate([_rot(rng), rng.uniform(-t, t, (3, 1))], 1).astype(np.float32)


def _scan_tile():
    src = open(os.path.join(REPO, "livingscenes_amd", "csrc", "ls_scan.h")).read()
    t, items = (int(re.search(rf"\b{k}\s*=\s*(\d+)", src).group(1)) for k in ("SCAN_T", "SCAN_ITEMS"))
    return t * items


TILE = _scan_tile()


# ------------------------------------------------------------------------------------------------ the layers above
def _solver(model, cfg=None):
    from livingscenes_amd.lib_more.more_solver import More_Solver
    base = {"shape_priors": {"n_input_point": 128, "prior_name": "chair", "ckpt_dir": ""}, "fps": {"n_init": 1}}
    base.update(cfg or {})
    return More_Solver(base, model=model)


@pytest.fixture(scope="module")
def small_prior():
    from livingscenes_amd.model_utils import Shape_Prior
    ecfg, dcfg = synth.small_encoder_cfg(), synth.small_decoder_cfg()
    ew, dw = synth.make_encoder_weights(ecfg, 4), synth.make_decoder_weights(dcfg, 4)
    return Shape_Prior.from_state(ecfg, dcfg, ew, dw, device=_dev(), n_pcl=128)


def _scene(x):
    """[n,N,3] -> the scene dict of _solve_end2end"""
    x = x.to(_dev())
    return {"pc": x.transpose(1, 2).contiguous(), "pc_mask": torch.ones(x.shape[0], 1, x.shape[1], dtype=torch.bool, device=x.device)}


STEP_KEYS = {"ref_pc_lst", "rescan_pc_lst", "matches", "registration", "codes", "mesh_lst", "merged_sizes", "n_new_points", "unmatched_rescan"}
GATE_KEYS = {"overlap", "overlap_rmse", "memory_seen", "rejected"}
REFINE_KEYS = {"refine_stop", "refine_iters", "registration_init"}
CODE_KEYS = ("z_so3", "z_inv", "s", "t")
