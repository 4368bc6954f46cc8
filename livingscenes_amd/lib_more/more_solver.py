"""Mirror of /root/reference/lib_more/more_solver.py (class More_Solver) for the accelerated path:
_solve_object_matching, _solve_pairwise_registration(optim=False), _transform_latent and the encode / match / register
part of _solve_end2end, plus batched variants the reference lacks (it registers one pair at a time with B=1 encoder
calls, eval_flyingshape.py:130).  _optimize_code and the optim=True registration branch run with the decoder
forward / backward and the Sinkhorn softmins in the HIP library; torchlie / geomloss / roma are not installed, so the SE(3)
update and the Sinkhorn divergence of that branch follow this build's documented definitions (parity unpinned); mesh extraction (_mesh_from_latent / _mesh_from_pc, 8 f-2) runs MISE and marching cubes on the device
(livingscenes_amd/mesh_extractor2.py)."""
import logging
import math

import numpy as np

import torch

from .. import ops
from ..lib_math.torch_se3 import Rt_to_SE3, inverse, transform
from ..mesh_extractor2 import Generator3D as Generator3D_MC
from ..model_utils import fps, load_ckpt_from_log, mesh_from_latent, place_mesh
from .matcher_new import (eq_seq_matcher, eq_seq_matcher_batch, nn_matcher, nn_matcher_batch, sequential_matcher, sequential_matcher_batch,
                          sim3_seq_matcher, sim3_seq_matcher_batch, sinkhorn_matcher, sinkhorn_matcher_batch)
from .pose_estimation import kabsch_transformation_estimation


class More_Solver:
    def __init__(self, cfg, model=None):
        """cfg as configs/more_3rscan.yaml; ``model`` (a Shape_Prior) may be injected instead of loading
        cfg['shape_priors']['ckpt_dir'] (more_solver.py:26-34)."""
        logging.info("Configuring MoRE solver")
        self.cfg = cfg
        # Generator3D (device MISE + marching cubes): more_solver.py:30
        self.mesh_extractor = Generator3D_MC(**cfg["mesh_extractor"]) if "mesh_extractor" in cfg else None
        if model is None:
            model = load_ckpt_from_log(cfg["shape_priors"]["ckpt_dir"])[cfg["shape_priors"]["prior_name"]]
        self.model = model

    # -------------------------------------------------------------------------------------------- matching
    def _solve_object_matching(self, src_codes, tgt_codes, method):
        """more_solver.py:71-93."""
        inv_src = src_codes["z_inv"].detach().clone()
        inv_tgt = tgt_codes["z_inv"].detach().clone()
        if method == "nn":
            return nn_matcher(inv_src.T[None], inv_tgt.T[None])
        if method == "sinkhorn":
            return sinkhorn_matcher(inv_src.T[None], inv_tgt.T[None])
        if method == "sequential":
            return sequential_matcher(inv_src, inv_tgt)
        if method == "sim3_seq":
            return sim3_seq_matcher(src_codes, tgt_codes)
        if method == "eq_seq":
            return eq_seq_matcher(src_codes, tgt_codes)

    def _solve_object_matching_batch(self, src_codes_list, tgt_codes_list, method):
        """_solve_object_matching for MANY scene pairs in one ragged call per stage (the reference matches one pair at a time):
        -> list of {'matches0', 'matches1'}, entry p equal to _solve_object_matching(src_codes_list[p], tgt_codes_list[p], method)."""
        if len(src_codes_list) != len(tgt_codes_list):
            raise ValueError(f"{len(src_codes_list)} source scenes for {len(tgt_codes_list)} target scenes")
        if not src_codes_list:
            return []
        if method in ("nn", "sinkhorn"):
            inv_src = [c["z_inv"].detach().T[None] for c in src_codes_list]
            inv_tgt = [c["z_inv"].detach().T[None] for c in tgt_codes_list]
            return nn_matcher_batch(inv_src, inv_tgt) if method == "nn" else sinkhorn_matcher_batch(inv_src, inv_tgt)
        if method == "sequential":
            return sequential_matcher_batch([c["z_inv"].detach() for c in src_codes_list], [c["z_inv"].detach() for c in tgt_codes_list])
        if method == "sim3_seq":
            return sim3_seq_matcher_batch(src_codes_list, tgt_codes_list)
        if method == "eq_seq":
            return eq_seq_matcher_batch(src_codes_list, tgt_codes_list)
        raise ValueError(f"unknown matching method {method!r}")

    # -------------------------------------------------------------------------------------------- registration
    def _register_from_codes(self, code1, code2):
        """more_solver.py:114-116: Kabsch on the 256 equivariant pseudo-points z_so3 + t."""
        return ops.kabsch_codes(code1["z_so3"], code1["t"], code2["z_so3"], code2["t"])   # z_so3 + t formed inside the launch

    def _icp(self, pc1, pc2, R, t):
        """more_solver.py:181-187: ICP refinement from the Kabsch initialisation (row-vector convention inside)."""
        Ri, Ti, _, _ = ops.icp(pc1, pc2, R.transpose(-1, -2).contiguous(), t.squeeze(2).contiguous())
        return Ri.transpose(-1, -2), Ti.unsqueeze(2)

    def _solve_pairwise_registration(self, pc1_full, pc2_full, optim=False):
        """more_solver.py:95-189.  pc1 [1,N,3], pc2 [1,M,3] -> R [1,3,3], t [1,3,1] mapping pc1 -> pc2."""
        if optim:
            return self._solve_pairwise_registration_optim(pc1_full, pc2_full)
        return self._solve_pairwise_registration_batch([pc1_full[0]], [pc2_full[0]])

    def _solve_pairwise_registration_optim(self, pc1_full, pc2_full):
        """more_solver.py:118-189 (optim=True) for ONE pair: the batched path with P = 1 (same arithmetic: a pair's trajectory does
        not depend on the batch it rides in)."""
        return self._solve_pairwise_registration_optim_batch([pc1_full[0]], [pc2_full[0]])

    def _solve_pairwise_registration_optim_batch(self, pcs1, pcs2, icp=True, return_info=False):
        """more_solver.py:118-189 (optim=True) for P pairs IN LOCK-STEP -- what eval_3rscan.py:381 runs per matched instance: keep the
        code that explains its own points better (:124-135), refine the Kabsch pose by Adam on SE(3) against
        SmoothL1(sdf(g.src; shared code)) + Sinkhorn(g.src, tgt) (:137-173: MultiStepLR [300, 340, 380], best-loss snapshot after the
        step, geodesic early stop), invert for the reversed direction (:175-179), then ICP (:181-187).
        Per step the host only sequences launches: decoder forward + backward on P x N queries (ls_sdf_decode_train /
        ls_sdf_backward), per-pair SmoothL1 + its gradient, the batched Sinkhorn softmins, and ONE kernel for the tangent gradient,
        the Adam moments, the retraction, the snapshot, the early-stop test and the next transformed cloud (csrc/optim.hip).
        torchlie / geomloss / roma are not installed: the manifold update (left-multiplicative retraction g <- exp(-step) g, Adam
        moments on the 6-vector (v, omega) of the left tangent space) and the Sinkhorn divergence follow this build's documented
        definitions -- PARITY UNPINNED.  lists of clouds [Ni,3] / [Mi,3] -> R [P,3,3], t [P,3,1] mapping pc1 -> pc2."""
        from .. import _lib
        from ..sinkhorn import divergence_batch
        n_in = self.cfg["shape_priors"]["n_input_point"]
        assert self.cfg.get("fps", {}).get("n_init", 1) == 1, "fps.n_init > 1 is not used by the released configs"
        reg = self.cfg["registration"]
        lr0, n_steps, stop = reg["step_size"]["so3"], reg["n_steps"], reg["early_stop_threshold"]
        P = len(pcs1)
        pc1, pc2 = self._sample(pcs1, n_in), self._sample(pcs2, n_in)
        hip = self.model.hip_model()
        with torch.no_grad():
            code = self.model.encode(torch.cat([pc1, pc2], 0).transpose(-1, -2).contiguous())
            c1 = {k: v[:P] for k, v in code.items()}
            c2 = {k: v[P:] for k, v in code.items()}
            se1, se2 = c1["z_so3"] + c1["t"], c2["z_so3"] + c2["t"]
            R12, t12, _, _ = kabsch_transformation_estimation(se1, se2)
            R21, t21, _, _ = kabsch_transformation_estimation(se2, se1)
            err1 = self.model.decoder(pc1, None, c1, return_sdf=True).abs().mean(1)
            err2 = self.model.decoder(pc2, None, c2, return_sdf=True).abs().mean(1)
            reverse = err1 < err2                                 # keep the code that explains its own points better (:124-135)

            def pick(a, b):                                       # a where reversed, b otherwise
                return torch.where(reverse.view(-1, *([1] * (a.dim() - 1))), a, b)
            shared = {k: pick(c1[k], c2[k]).contiguous() for k in ("z_so3", "z_inv", "s", "t")}
            src, tgt = pick(pc2, pc1).contiguous(), pick(pc1, pc2).contiguous()
            g0 = torch.cat([pick(R21, R12), pick(t21, t12)], 2).contiguous()
            two_piece = int(reg.get("decoder_bf16_pieces", 3)) == 2
            opt, steps_run = self._refine_se3(shared, src, tgt, g0, n_steps, lr0, stop, two_piece=two_piece)
            best = opt.best_g
            Rb = best[:, :, :3].transpose(1, 2)
            inv = torch.cat([Rb, -(Rb @ best[:, :, 3:4])], 2)
            best = pick(inv, best)
            R, t = best[:, :, :3].contiguous(), best[:, :, 3:4].contiguous()
        if icp:
            R, t = self._icp(pc1, pc2, R, t)
        if return_info:
            return R, t, {"reverse": reverse, "min_loss": opt.min_loss, "active": opt.active, "steps": steps_run, "pre_icp": best}
        return R, t

    def _refine_se3(self, shared, src, tgt, g0, n_steps, lr0, stop, two_piece=False, trace=None):
        """The refinement loop of more_solver.py:137-173 for P pairs in lock-step (csrc/optim.hip; oracle twin: oracle/optim.py
        registration_loop): shared = the code dict the decoder is conditioned on (P rows), src / tgt [P,N,3] / [P,M,3], g0 [P,3,4].
        -> (ops.Se3Adam state, steps run).  ``trace`` (list) receives (g [P,3,4], loss [P]) after every step (tests)."""
        from .. import _lib
        from ..sinkhorn import divergence_batch
        hip = self.model.hip_model()
        # batch-invariant decoder arithmetic (P pairs == each pair alone); opt-in (not in the reference's yaml):
        # registration.decoder_bf16_pieces = 2 runs the refinement's decoder GEMMs with two-piece bf16 products (2^-16 per product).
        # The handle's previous settings are restored afterwards (a caller-chosen option is not clobbered).
        prev_split = hip.set_option(_lib.OPT_SDF_TRAIN_SPLITK, 0)
        prev_x2 = hip.set_option(_lib.OPT_SDF_BF16X2, 1) if two_piece else None
        try:
            opt = ops.Se3Adam(g0, src, stop)
            steps_run = 0
            # length of the Sinkhorn epsilon-schedule loop: read back once, then guessed as (largest seen + 1) and VERIFIED at the
            # host read every 16 steps (a schedule grows by one entry when a pair's bounding-box diameter doubles; 16 steps of
            # at most lr radians / units each cannot do that) -- no device -> host round trip inside a step
            sched_len, needs = None, []
            for i in range(n_steps):
                lr = lr0 * (0.1 ** sum(i >= ms for ms in (300, 340, 380)))          # MultiStepLR([300, 340, 380], 0.1), :143
                sdf, saved = hip.sdf_decode_train(opt.query, shared["z_so3"], shared["z_inv"], shared["s"], shared["t"])
                loss, gsdf = ops.smooth_l1(sdf)
                gq = hip.sdf_backward(saved, gsdf, need_code_grad=False)[0]              # the code is fixed here (:137-141)
                sl, sg, need = divergence_batch(opt.query, tgt, lmax=sched_len, return_need=True)
                if sched_len is None:
                    sched_len = int(need) + 1
                needs.append(need)
                opt.step(gq + sg, loss + sl, lr)
                steps_run = i + 1
                if trace is not None:
                    trace.append((opt.g.clone(), (loss + sl).clone()))
                if i % 16 == 15:                                            # one host read per 16 steps
                    worst = int(torch.stack(needs).max())
                    if worst > sched_len:
                        # a pose ran away far enough to double a bounding box within 16 steps: those steps used a schedule one
                        # entry short (a coarser final epsilon for that pair); widen and carry on rather than abort the whole batch
                        import warnings
                        warnings.warn(f"Sinkhorn schedule grew from {sched_len} to {worst} entries within 16 steps (diverging pose?)")
                    sched_len, needs = worst + 1, []
                    if not bool(opt.active.any()):                          # every pair stopped early
                        break
        finally:
            hip.set_option(_lib.OPT_SDF_TRAIN_SPLITK, prev_split)
            if two_piece:
                hip.set_option(_lib.OPT_SDF_BF16X2, prev_x2)
        return opt, steps_run

    def _sample(self, pcs, n_in):
        """Ragged FPS of a list of clouds [Ni,3] to n_in points each: ONE launch."""
        dev = pcs[0].device
        lens = torch.tensor([p.shape[0] for p in pcs], device=dev)
        buf = torch.zeros(len(pcs), int(lens.max()), 3, device=dev)
        for i, p in enumerate(pcs):
            buf[i, : p.shape[0]] = p
        idx = ops.fps(buf, n_in, lengths=lens)
        return torch.gather(buf, 1, idx.long()[..., None].expand(-1, -1, 3))

    def _solve_pairwise_registration_batch(self, pcs1, pcs2, icp=True):
        """Batched form: lists of clouds [Ni,3] / [Mi,3] -> R [P,3,3], t [P,3,1].  One ragged FPS launch per side,
        ONE encoder batch of 2P instances, one Kabsch launch, one ICP launch."""
        n_in = self.cfg["shape_priors"]["n_input_point"]
        assert self.cfg.get("fps", {}).get("n_init", 1) == 1, "fps.n_init > 1 is not used by the released configs"
        P = len(pcs1)
        pc1, pc2 = self._sample(pcs1, n_in), self._sample(pcs2, n_in)
        with torch.no_grad():
            code = self.model.encode(torch.cat([pc1, pc2], 0).transpose(-1, -2).contiguous())
        c1 = {k: v[:P] for k, v in code.items()}
        c2 = {k: v[P:] for k, v in code.items()}
        R, t = self._register_from_codes(c1, c2)
        if icp:
            R, t = self._icp(pc1, pc2, R, t)
        return R, t

    def _optimize_code(self, code, pc, mask, n_steps=200):
        """more_solver.py:191-228 for one instance (the batched path with P = 1)."""
        valid_pc = pc.T[mask.squeeze()].squeeze()
        best, improved = self._optimize_code_batch(code, [valid_pc], n_steps=n_steps)
        return best if bool(improved[0]) else None

    def _optimize_code_batch(self, code, pcs, n_steps=200):
        """more_solver.py:191-228 for P instances at once (eval_3rscan.py:489 calls it per instance): Adam on (z_inv, t, z_so3) against
        MSE(sdf(pc; code), 0), lr 1e-5 / 1e-4 / 5e-4, x0.1 at step 160.  `code` holds P rows; pcs = list of P clouds [Ni,3].  The
        loss is the SUM over instances of their mean-squared SDF, so every instance sees exactly the gradients (and, Adam being
        element-wise, exactly the updates) of its own run; the decoder forward / backward run in the HIP library for all P x N
        queries per step (ls_sdf_decode_train / ls_sdf_backward, split-K off: a row's value does not depend on the batch).
        The reference snapshots `best_code` with .detach() WITHOUT .clone(), i.e. the snapshot aliases the live parameters and ends
        up holding the FINAL values whenever the loss improved at least once (min_loss starts at 100): returned here as (code dict
        of the final values, improved [P] bool) -- an instance that never improved has best_code = None in the reference."""
        from .. import _lib
        n_in = self.cfg["shape_priors"]["n_input_point"]
        pc = self._sample(pcs, n_in)
        P = pc.shape[0]
        dev = pc.device
        # the live parameters (updated in place by the device Adam; written back into the caller's tensors at the end: in the reference
        # the caller's code tensors ARE the optimizer's parameters, more_solver.py:195-200)
        z_inv = code["z_inv"].detach().float().contiguous().clone()
        t = code["t"].detach().float().reshape(P, 3).contiguous().clone()
        z_so3 = code["z_so3"].detach().float().contiguous().clone()
        s_ = code["s"].detach().float().contiguous()
        hip = self.model.hip_model()
        # decoder_type "deepsdf": the SDF does not depend on t or z_so3, their .grad stays None and the reference's Adam never moves them
        inv_only = hip.desc.dec_input == _lib.DEC_XYZ
        opt = ops.Adam([(z_inv, 1e-5)] if inv_only else [(z_inv, 1e-5), (t, 1e-4), (z_so3, 5e-4)])   # more_solver.py:199-203
        min_loss = torch.full((P,), 100.0, device=dev)                        # :205
        improved = torch.zeros(P, dtype=torch.int32, device=dev)
        prev_split = hip.set_option(_lib.OPT_SDF_TRAIN_SPLITK, 0)
        try:
            # per step: decoder forward (activations kept), MSE + its gradient + the best-loss bookkeeping, decoder backward w.r.t. the
            # code, ONE Adam launch for the three tensors -- no autograd graph, no ATen kernel, no host read inside the loop
            for i in range(n_steps):
                sdf, saved = hip.sdf_decode_train(pc, z_so3, z_inv, s_, t)
                _, gsdf = ops.mse(sdf, min_loss, improved)                       # MSELoss(sdf, 0) of every instance (:213), :219-221
                _, gso3, ginv, _, gt = hip.sdf_backward(saved, gsdf, need_query_grad=False)
                opt.step([ginv] if inv_only else [ginv, gt, gso3], lr_scale=0.1 if i >= 160 else 1.0)   # MultiStepLR([160], 0.1) (:204)
        finally:
            hip.set_option(_lib.OPT_SDF_TRAIN_SPLITK, prev_split)
        with torch.no_grad():
            code["z_inv"].copy_(z_inv.reshape(code["z_inv"].shape))
            code["z_so3"].copy_(z_so3.reshape(code["z_so3"].shape))
            code["t"].copy_(t.reshape(code["t"].shape))
        improved = improved.bool()
        return {k: code[k].detach() for k in ("z_inv", "z_so3", "s", "t")}, improved

    def _optimize_code_on_fusion_batch(self, code, fusion, slots=None, n_band=None, n_free=None, n_steps=200, min_obs=1, seed=0):
        """Scene memory, the FUSED STATE as the training signal of the code optimisation (an extension beyond the released reference, whose
        only supervision is MSE(sdf(points), 0): the surface, which says nothing about which side is outside nor about the space the
        cameras looked through; off-surface samples and the clamp of free space are DeepSDF's, Park et al. 2019).  The loop of
        _optimize_code_batch with the _sample call replaced by ONE draw (ops.tsdf_draw_batch, csrc/tsdffit.hip) and ops.mse by
        ops.tsdf_fit_loss: equality with the fused distance inside the band, a one-sided hinge "at least trunc" in observed free space,
        both in the decoder's units (THIS BUILD'S DEFINITION: the decoder's value times s is a metric distance).  Everything else is the
        same: the parameter groups and learning rates, the x0.1 at step 160, the inv_only case of decoder_type "deepsdf", split-K off, the
        write-back, the same four launches per Adam step.  `code` holds P rows; fusion = the dict of _fuse_batch (sum, n: int32
        [n,res,res,res]; origin, voxel, trunc); slots = the P slots of the fusion the rows belong to (None: the fusion has P slots, in
        order).  n_band / n_free default to n_input_point // 2 each -- DERIVED, NOT TUNED: the decoder batch then has the size the point
        path gives it.  The seed of slot i is seed + i, so a slot's draw does not depend on which other slots are optimised with it.  No
        weight between the kinds, no clamp of the band error, and s is not optimised (the reference's loop does not move it either).
        -> (code dict of the final values, improved [P] bool, report: dict of per-row lists loss_first, loss_last (float64: the loss at
        the first and at the last step), n_band, n_free (columns actually taken)).  A slot whose state holds no eligible sample has no
        column: its loss is 0, its gradient 0, it never improves and keeps its code.  NO QUOTA, min_obs OR fuse_res IS RECOMMENDED, and
        whether the fitted code matches or meshes better than the point-fitted one is unmeasured: nothing here can measure it."""
        from .. import _lib
        n_in = self.cfg["shape_priors"]["n_input_point"]
        n_band = n_in // 2 if n_band is None else int(n_band)
        n_free = n_in // 2 if n_free is None else int(n_free)
        P = code["z_inv"].shape[0]
        slots = list(range(fusion["sum"].shape[0])) if slots is None else [int(i) for i in slots]
        if len(slots) != P:
            raise ValueError(f"{P} code rows for {len(slots)} slots of the fusion")
        S, N = fusion["sum"], fusion["n"]
        dev = S.device
        origin, voxel, trunc = (np.asarray(fusion[k], dtype=np.float64) for k in ("origin", "voxel", "trunc"))
        if slots != list(range(S.shape[0])):
            rows = torch.tensor(slots, device=dev)
            S, N = S[rows].contiguous(), N[rows].contiguous()
            origin, voxel, trunc = origin[slots], voxel[slots], trunc[slots]
        pc, target, kind, _, counts = ops.tsdf_draw_batch((S, N), origin=origin, voxel=voxel, trunc=trunc, n_band=n_band, n_free=n_free,
                                                          seeds=np.array([int(seed) + i for i in slots], dtype=np.uint64), min_obs=min_obs)
        trunc_dev = torch.as_tensor(np.ascontiguousarray(trunc), device=dev)
        z_inv = code["z_inv"].detach().float().contiguous().clone()
        t = code["t"].detach().float().reshape(P, 3).contiguous().clone()
        z_so3 = code["z_so3"].detach().float().contiguous().clone()
        s_ = code["s"].detach().float().contiguous()
        s_row = s_.reshape(P).contiguous()
        hip = self.model.hip_model()
        inv_only = hip.desc.dec_input == _lib.DEC_XYZ
        opt = ops.Adam([(z_inv, 1e-5)] if inv_only else [(z_inv, 1e-5), (t, 1e-4), (z_so3, 5e-4)])   # more_solver.py:199-203
        min_loss = torch.full((P,), 100.0, dtype=torch.float64, device=dev)   # :205
        improved = torch.zeros(P, dtype=torch.int32, device=dev)
        first = last = torch.zeros(P, dtype=torch.float64, device=dev)
        prev_split = hip.set_option(_lib.OPT_SDF_TRAIN_SPLITK, 0)
        try:
            # per step the four launches of _optimize_code_batch: decoder forward, the loss + its gradient + the best-loss bookkeeping,
            # decoder backward w.r.t. the code, ONE Adam launch -- no autograd graph, no ATen kernel, no host read inside the loop
            for i in range(n_steps):
                sdf, saved = hip.sdf_decode_train(pc, z_so3, z_inv, s_, t)
                last, gsdf = ops.tsdf_fit_loss(sdf, s_row, trunc_dev, target, kind, min_loss, improved)
                if i == 0:
                    first = last
                _, gso3, ginv, _, gt = hip.sdf_backward(saved, gsdf, need_query_grad=False)
                opt.step([ginv] if inv_only else [ginv, gt, gso3], lr_scale=0.1 if i >= 160 else 1.0)   # MultiStepLR([160], 0.1) (:204)
        finally:
            hip.set_option(_lib.OPT_SDF_TRAIN_SPLITK, prev_split)
        with torch.no_grad():
            code["z_inv"].copy_(z_inv.reshape(code["z_inv"].shape))
            code["z_so3"].copy_(z_so3.reshape(code["z_so3"].shape))
            code["t"].copy_(t.reshape(code["t"].shape))
        report = {"loss_first": first.cpu().tolist(), "loss_last": last.cpu().tolist(),
                  "n_band": np.minimum(counts[:, 1], n_band).tolist(), "n_free": np.minimum(counts[:, 2], n_free).tolist()}
        # a slot without a column has loss 0.0, which is below the starting min_loss: it did not improve, it has nothing to fit
        improved = improved.bool() & torch.as_tensor(counts[:, 0] > 0, device=dev)
        return {k: code[k].detach() for k in ("z_inv", "z_so3", "s", "t")}, improved, report

    @staticmethod
    def _memory_pose(T, g, P):
        """the pose the scene-memory operators receive (observation -> memory frame) from either the registration T (memory -> rescan, as
        _solve_pairwise_registration* / Rt_to_SE3 return it: inverse(T)) or g, that pose given directly; both None: None"""
        if T is not None and g is not None:
            raise ValueError("give the registration T (memory -> rescan) or the memory-frame pose g (rescan -> memory), not both")
        if g is not None:
            if g.dim() != 3 or g.shape[0] != P or g.shape[1] not in (3, 4) or g.shape[2] != 4:
                raise ValueError(f"g must be [P,4,4] or [P,3,4] with P = {P}, got {tuple(g.shape)}")
            return g.detach().float().contiguous()
        if T is None:
            return None
        if T.dim() != 3 or T.shape[0] != P or T.shape[1] not in (3, 4) or T.shape[2] != 4:
            raise ValueError(f"T must be [P,4,4] or [P,3,4] with P = {P}, got {tuple(T.shape)}")
        return inverse(T.detach().float()).contiguous()

    def _accumulate_batch(self, mem_pcs, new_pcs, T, voxel=None, g=None):
        """Scene memory, an extension beyond the released reference (its README promises "the accumulation of point clouds originating from
        the same instance"; more_solver.py:246-299 stops after the registration): merge P kept instance clouds mem_pcs[p] [a_p,3] (in
        the memory's frame) with the matched observations new_pcs[p] [b_p,3] in ONE ragged call (ops.cloud_merge_batch, csrc/cloudmerge.hip).
        T [P,4,4] or [P,3,4] is the registration exactly as _solve_pairwise_registration* / Rt_to_SE3 return it: it maps memory -> rescan, so
        the operator receives inverse(T), the inverse _solve_end2end forms for _transform_latent (T None: the observations are in the
        memory's frame already and are used bit for bit).  A point is kept iff no earlier point of (memory rows, then transformed
        observation rows) lies in its voxel, so what the memory holds always wins and an instance seen any number of times stays at one
        point per voxel.  voxel: the edge in metres, default cfg['accumulate']['voxel_size'], else 0.01 -- AN UNMEASURED CHOICE: roughly a
        third of the point spacing of a 1 024-point, 1 m object, so a sampled cloud passes nearly whole while repeated observations of a
        surface do not pile up.  g (keyword, [P,4,4] or [P,3,4]): the pose rescan -> memory given directly instead of T -- what
        _refine_on_memory_batch returns, so a refined pose reaches the merge without an inverse of an inverse; T and g together are an error.
        -> list of P merged clouds [n_p,3]."""
        if voxel is None:
            voxel = self.cfg.get("accumulate", {}).get("voxel_size", 0.01)
        if len(mem_pcs) != len(new_pcs):
            raise ValueError(f"{len(mem_pcs)} memory clouds for {len(new_pcs)} observations")
        g = self._memory_pose(T, g, len(mem_pcs))
        return [pts for pts, _ in ops.cloud_merge_batch([p.detach() for p in mem_pcs], [p.detach() for p in new_pcs], g=g, voxel=voxel)]

    def _overlap_batch(self, mem_pcs, new_pcs, T, radius=None, g=None):
        """Scene memory, the question before a merge (an extension beyond the released reference, like _accumulate_batch): how well do P
        registered observations new_pcs[p] [b_p,3] agree with the kept clouds mem_pcs[p] [a_p,3]?  ONE ragged fixed-radius nearest-neighbour
        call (ops.cloud_nearest_batch, csrc/cloudnear.hip).  T [P,4,4] or [P,3,4] is the registration exactly as
        _solve_pairwise_registration* / Rt_to_SE3 return it: it maps memory -> rescan, so the operator receives inverse(T), exactly as
        _accumulate_batch does (T None: the observations are in the memory's frame already).  radius: default
        cfg['accumulate']['overlap_radius'], else 2 * voxel with the voxel of _accumulate_batch -- A DERIVED DEFAULT, not a tuned one: a
        point the merge drops shares a voxel of edge h with a kept one, so a perfectly registered re-observation of a surface the memory
        already holds lies within sqrt(3) h < 2 h of a kept point.  g (keyword): the pose rescan -> memory given directly instead of T,
        as for _accumulate_batch; T and g together are an error.
        -> dict of per-pair lists: overlap = matched / finite observation points (0.0 with no finite point), rmse = sqrt(sum d2 / matched)
        (nan with none), memory_seen = memory points that are some observation point's neighbour / a_p (0.0 for an empty memory), counts =
        the raw int64 triples (finite queries, matched, memory points hit), nn_idx [b_p] int32 = the memory row nearest to every
        observation point within the radius, -1: none -- the points that are new."""
        acc = self.cfg.get("accumulate", {})
        if radius is None:
            radius = acc.get("overlap_radius", 2 * acc.get("voxel_size", 0.01))
        if len(mem_pcs) != len(new_pcs):
            raise ValueError(f"{len(mem_pcs)} memory clouds for {len(new_pcs)} observations")
        g = self._memory_pose(T, g, len(mem_pcs))
        res = ops.cloud_nearest_batch([p.detach() for p in mem_pcs], [p.detach() for p in new_pcs], g=g, radius=radius)
        return self._overlap_figures(mem_pcs, res)

    @staticmethod
    def _overlap_figures(mem_pcs, searches):
        """the dict of _overlap_batch from per-pair search results (idx, d2, counts, sum_d2)"""
        out = {"overlap": [], "rmse": [], "memory_seen": [], "counts": [], "nn_idx": []}
        for mem_pc, (idx, _, counts, sum_d2) in zip(mem_pcs, searches):
            finite, matched, seen = (int(c) for c in counts)
            out["overlap"].append(matched / finite if finite else 0.0)
            out["rmse"].append(math.sqrt(sum_d2 / matched) if matched else float("nan"))
            out["memory_seen"].append(seen / mem_pc.shape[0] if mem_pc.shape[0] else 0.0)
            out["counts"].append(counts)
            out["nn_idx"].append(idx)
        return out

    def _memory_normals_batch(self, mem_pcs, radius=None, min_nbrs=5):
        """Scene memory, a normal per kept point (an extension beyond the released reference, like _accumulate_batch): ONE ragged call
        (ops.cloud_normals_batch, csrc/cloudnear.hip) over the P kept clouds mem_pcs[p] [a_p,3].  radius: default 3 * the voxel of
        _accumulate_batch (cfg['accumulate']['voxel_size'], else 0.01) -- A DERIVED DEFAULT, not a tuned one: at one point per voxel of
        edge h on a surface, a ball of radius 3 h holds about 9 pi = 28 points.  min_nbrs = 5 is NOT TUNED; the rank rule of the operator
        does the real work.  -> list of P (normals [a_p,3], nbr_cnt [a_p] int32, variation [a_p], counts host int64 [2]) as
        ops.cloud_normals_batch returns them: a row without a normal is (0, 0, 0)."""
        if radius is None:
            radius = 3 * self.cfg.get("accumulate", {}).get("voxel_size", 0.01)
        return ops.cloud_normals_batch([p.detach() for p in mem_pcs], radius=radius, min_nbrs=min_nbrs)

    def _consolidate_batch(self, mem_pcs, radius=None, voxel=None, min_nbrs=5, max_variation=1 / 3, max_shift=float("inf")):
        """Scene memory, a consolidation on request (an extension beyond the released reference, like _accumulate_batch): the memory
        keeps the first point of every voxel with the sensor noise of the scan that delivered it, and noisy rescans fill the voxels on
        both sides of the true surface.  ONE ops.cloud_project_batch call (csrc/cloudnear.hip) projects every kept point of the P clouds
        mem_pcs[p] [a_p,3] onto the plane of its neighbourhood, from the input positions; ONE ops.cloud_merge_batch call of the projected
        clouds against empty observations at `voxel` (the merge unchanged: first wins, one point per voxel) drops the rows that now share
        a voxel.  It MOVES kept points, which no merge does, so nothing calls it unasked; and a projection shrinks a curved surface a
        little each time, so it is meant to run ONCE, not after every merge (solve_sequence's docstring has the figures).
        voxel: as _accumulate_batch (cfg['accumulate']['voxel_size'], else 0.01).  radius: default 3 * voxel, the default of
        _memory_normals_batch -- A DERIVED DEFAULT, not tuned: about 9 pi = 28 points at one point per voxel on a surface.  min_nbrs,
        max_variation (1/3: no limit) and max_shift (inf: no limit) are ops.cloud_project_batch's: no value of either limit is recommended.
        -> (list of P consolidated clouds [n_p,3],
            dict of per-slot lists: rows_before, rows_after, moved, held, no_plane (rows per state of the projection) and rms_shift =
            sqrt(sum_shift2 / moved), the RMS distance the moved rows travelled (nan when nothing moved))."""
        if voxel is None:
            voxel = self.cfg.get("accumulate", {}).get("voxel_size", 0.01)
        if radius is None:
            radius = 3 * voxel
        clouds = [p.detach() for p in mem_pcs]
        proj = ops.cloud_project_batch(clouds, radius=radius, min_nbrs=min_nbrs, max_variation=max_variation, max_shift=max_shift)
        merged = ops.cloud_merge_batch([pts for pts, _, _, _, _ in proj], [c[:0] for c in clouds], voxel=voxel)
        info = {"rows_before": [], "rows_after": [], "moved": [], "held": [], "no_plane": [], "rms_shift": []}
        for c, (_, _, _, counts, sum_shift2), (pts, _) in zip(clouds, proj, merged):
            moved = int(counts[3])
            info["rows_before"].append(c.shape[0])
            info["rows_after"].append(pts.shape[0])
            info["moved"].append(moved)
            info["held"].append(int(counts[2]))
            info["no_plane"].append(int(counts[1]))
            info["rms_shift"].append(math.sqrt(sum_shift2 / moved) if moved else float("nan"))
        return [pts for pts, _ in merged], info

    @staticmethod
    def _memory_cameras(world_to_cam, to_obs):
        """world_to_cam [V,3,4] float64 of the observation's frame composed with to_obs [3,4] float64 (memory -> observation; None: the
        views are in the memory's frame already) -> world_to_cam from the memory's frame, float64"""
        E = world_to_cam.to(torch.float64)
        if to_obs is None:
            return E.contiguous()
        M = to_obs.to(E.device)
        return torch.cat([E[:, :, :3] @ M[:, :3], E[:, :, :3] @ M[:, 3:4] + E[:, :, 3:4]], dim=-1).contiguous()

    def _carve_batch(self, mem_pcs, views, T=None, g=None, *, tol, window=1, min_free=1, max_seen=0, empty="unknown", znear=0.05):
        """Scene memory, the one step that REMOVES kept points (an extension beyond the released reference, like _accumulate_batch): carve
        P kept clouds mem_pcs[p] [a_p,3] (in the memory's frame) by posed depth views of the matched observations in ONE ragged call
        (ops.cloud_carve_batch, csrc/cloudcarve.hip).  A kept point that a view looks THROUGH lies in observed free space and is dropped;
        a point a view confirms, a point it cannot see and a point it cannot judge stay.  views[p] = dict(depth [V,H,W] fp32, intrinsics
        [V,4] or [4], world_to_cam [V,3,4]) in the OBSERVATION's frame (HIP tensors).  T [P,4,4] or [P,3,4] is the registration as
        _solve_pairwise_registration* return it (memory -> rescan), or g (keyword-compatible with _accumulate_batch: rescan -> memory, what
        _refine_on_memory_batch returns); T and g together are an error, both None: the views are in the memory's frame.  The cameras
        the operator receives are world_to_cam o T, or world_to_cam o inverse(g), formed in float64.  window = 1 is ops.cloud_carve_batch's
        derived default; tol HAS NO DEFAULT AND NONE IS RECOMMENDED, nor any min_free or max_seen: none has been measured on real scans.
        -> (list of P carved clouds [n_p,3]: subsequences of mem_pcs[p], the same bits,
            dict: src (list of P int32 [n_p]: the kept rows), n_carved (list of P ints), seen / free (lists of P int32 [a_p]), counts (host
            int64 [P,4]) and view_counts (list of P host int64 [V_p,5]) as ops.cloud_carve_batch returns them)."""
        P = len(mem_pcs)
        if len(views) != P:
            raise ValueError(f"{P} memory clouds for {len(views)} sets of views")
        if T is not None and g is not None:
            raise ValueError("give the registration T (memory -> rescan) or the memory-frame pose g (rescan -> memory), not both")
        to_obs = None
        for name, pose in (("T", T), ("g", g)):
            if pose is None:
                continue
            if pose.dim() != 3 or pose.shape[0] != P or pose.shape[1] not in (3, 4) or pose.shape[2] != 4:
                raise ValueError(f"{name} must be [P,4,4] or [P,3,4] with P = {P}, got {tuple(pose.shape)}")
            to_obs = pose.detach().to(torch.float64)[:, :3, :]
            if name == "g":
                to_obs = inverse(to_obs)
        cams = [self._memory_cameras(v["world_to_cam"], None if to_obs is None else to_obs[p]) for p, v in enumerate(views)]
        res, f = ops.cloud_carve_batch([p.detach() for p in mem_pcs], [v["depth"] for v in views], [v["intrinsics"] for v in views], cams,
                                       tol=tol, window=window, min_free=min_free, max_seen=max_seen, empty=empty, znear=znear)
        f["src"] = [s for _, s in res]
        f["n_carved"] = [int(c) for c in f["counts"][:, 2]]
        return [pts for pts, _ in res], f

    @staticmethod
    def _fusion_grids(clouds, res, trunc_voxels=4):
        """Scene memory, the grids the depth fusion works on (an extension beyond the released reference, like _carve_batch): one cubic grid
        of res^3 samples per cloud [n_p,3], in float64 on the host.  With the bounding box of the cloud, h = (largest extent) /
        (res - 1 - 2 trunc_voxels), the grid is centred on the box: origin = centre - h (res - 1) / 2 (the centre of voxel (0,0,0)), and
        trunc = trunc_voxels h.  The padding equals the truncation band, which is DERIVED: a surface on a face of the box keeps its whole
        band inside the grid.  trunc_voxels = 4 is AN UNMEASURED DEFAULT (what the CPU experiment of DESIGN.md used); no res is
        recommended.  res < 2 trunc_voxels + 2 is refused.  -> dict(origin [P,3], voxel [P], trunc [P]: host float64 tensors, dims)."""
        res, trunc_voxels = int(res), int(trunc_voxels)
        if trunc_voxels < 1 or res < 2 * trunc_voxels + 2:
            raise ValueError(f"_fusion_grids: res must be at least 2 * trunc_voxels + 2 = {2 * max(trunc_voxels, 1) + 2} with trunc_voxels >= 1, "
                             f"got res = {res}, trunc_voxels = {trunc_voxels}")
        origin, voxel = [], []
        for p, c in enumerate(clouds):
            if c.shape[0] == 0:
                raise ValueError(f"_fusion_grids: cloud {p} is empty: it has no bounding box")
            c64 = c.detach().to(torch.float64)
            lo, hi = c64.min(0).values.cpu(), c64.max(0).values.cpu()
            h = (hi - lo).max() / float(res - 1 - 2 * trunc_voxels)
            origin.append((lo + hi) / 2 - h * float(res - 1) / 2)
            voxel.append(h)
        voxel = torch.stack(voxel)
        return {"origin": torch.stack(origin), "voxel": voxel, "trunc": float(trunc_voxels) * voxel, "dims": (res, res, res)}

    def _fuse_batch(self, fusion, views, T=None, g=None, empty="unknown", znear=0.05):
        """Scene memory, the surface side of the carve (an extension beyond the released reference): fuse posed depth views of the matched
        observations into the truncated signed distance state of P instances, IN PLACE, in ONE ragged call (ops.depth_fuse_batch,
        csrc/depthfuse.hip).  fusion = dict(sum, n: int32 [P,res,res,res] HIP tensors -- ops.tsdf_state --, origin [P,3], voxel [P],
        trunc [P]: host float64, as _fusion_grids makes them), the grids in the memory's frame.  views[p] = dict(depth [V,H,W] fp32,
        intrinsics [V,4] or [4], world_to_cam [V,3,4]) in the OBSERVATION's frame, or None: the slot is left as it is.  T, g: exactly the
        conventions of _carve_batch (T: memory -> rescan, g: rescan -> memory, not both, both None: the views are in the memory's frame);
        the cameras the operator receives are _memory_cameras(world_to_cam, T) or (world_to_cam, inverse(g)), formed in float64.
        -> list of P device int64 [V_p,6]: voxels per class of ops.FUSE_CLASS and view."""
        P = fusion["sum"].shape[0]
        if len(views) != P:
            raise ValueError(f"{P} fusion states for {len(views)} sets of views")
        if T is not None and g is not None:
            raise ValueError("give the registration T (memory -> rescan) or the memory-frame pose g (rescan -> memory), not both")
        to_obs = None
        for name, pose in (("T", T), ("g", g)):
            if pose is None:
                continue
            if pose.dim() != 3 or pose.shape[0] != P or pose.shape[1] not in (3, 4) or pose.shape[2] != 4:
                raise ValueError(f"{name} must be [P,4,4] or [P,3,4] with P = {P}, got {tuple(pose.shape)}")
            to_obs = pose.detach().to(torch.float64)[:, :3, :]
            if name == "g":
                to_obs = inverse(to_obs)
        cams = [None if v is None else self._memory_cameras(v["world_to_cam"], None if to_obs is None else to_obs[p]) for p, v in enumerate(views)]
        shared = next((v["intrinsics"] for v in views if v is not None), None)
        return ops.depth_fuse_batch((fusion["sum"], fusion["n"]), [None if v is None else v["depth"] for v in views],
                                    [shared if v is None else v["intrinsics"] for v in views], cams, origin=fusion["origin"],
                                    voxel=fusion["voxel"], trunc=fusion["trunc"], empty=empty, znear=znear)

    def _fuse_weighted_batch(self, fusion, views, T=None, g=None, *, weights, value="plane", max_jump=None, empty="unknown", znear=0.05):
        """_fuse_batch with integer weights and, for value="plane", the point-to-plane value inside the band (ops.depth_fuse_weighted_batch,
        csrc/depthplane.hip; an extension beyond the released reference, opt-in).  fusion, views, T, g, empty and znear: exactly the
        conventions of _fuse_batch.  weights = (w_plane, w_proj, w_free, w_empty), four integers in 1 .. 255: NO DEFAULT, NONE IS
        RECOMMENDED.  value="plane": ONE ops.depth_normals call for all views of the batch (the normals live in the camera frame, so no
        pose enters), then ONE fuse call; max_jump = one value or one per problem, in the depth's unit; None: each problem's trunc -- what
        the experiment on the analytic sphere used, AN UNMEASURED DEFAULT.  value="projective": no normals, the weights alone.
        -> list of P device int64 [V_p,7]: voxels per class of ops.FUSE_WEIGHTED_CLASS and view."""
        P = fusion["sum"].shape[0]
        if len(views) != P:
            raise ValueError(f"{P} fusion states for {len(views)} sets of views")
        if value not in ("plane", "projective"):
            raise ValueError(f"value must be 'plane' or 'projective', got {value!r}")
        to_obs = self._to_observation(P, T, g)
        cams = [None if v is None else self._memory_cameras(v["world_to_cam"], None if to_obs is None else to_obs[p]) for p, v in enumerate(views)]
        shared = next((v["intrinsics"] for v in views if v is not None), None)
        normals = None
        have = [(p, v) for p, v in enumerate(views) if v is not None and v["depth"].shape[0]]
        if value == "plane" and have:
            jump = fusion["trunc"] if max_jump is None else max_jump
            jump = torch.as_tensor(jump, dtype=torch.float64).detach().cpu().reshape(-1)
            if jump.numel() not in (1, P):
                raise ValueError(f"max_jump is one value or one per problem (P = {P}), got {jump.numel()}")
            jump = jump.expand(P) if jump.numel() == 1 else jump
            D = torch.cat([v["depth"] for _, v in have]) if len(have) > 1 else have[0][1]["depth"]
            K = [v["intrinsics"].to(torch.float64).reshape(-1, 4).expand(v["depth"].shape[0], 4) for _, v in have]
            per_view = np.concatenate([np.full(v["depth"].shape[0], float(jump[p])) for p, v in have])
            normals = ops.depth_normals(D, torch.cat(K) if len(K) > 1 else K[0], max_jump=per_view)[0]
        return ops.depth_fuse_weighted_batch((fusion["sum"], fusion["n"]), [None if v is None else v["depth"] for v in views],
                                             [shared if v is None else v["intrinsics"] for v in views], cams, origin=fusion["origin"],
                                             voxel=fusion["voxel"], trunc=fusion["trunc"], weights=weights, normals=normals, empty=empty, znear=znear)

    @staticmethod
    def _to_observation(P, T, g):
        """the conventions of _carve_batch / _fuse_batch: T (memory -> rescan) or g (rescan -> memory), not both -> memory -> observation
        [P,3,4] float64, or None when both are None (the views are in the memory's frame)"""
        if T is not None and g is not None:
            raise ValueError("give the registration T (memory -> rescan) or the memory-frame pose g (rescan -> memory), not both")
        to_obs = None
        for name, pose in (("T", T), ("g", g)):
            if pose is None:
                continue
            if pose.dim() != 3 or pose.shape[0] != P or pose.shape[1] not in (3, 4) or pose.shape[2] != 4:
                raise ValueError(f"{name} must be [P,4,4] or [P,3,4] with P = {P}, got {tuple(pose.shape)}")
            to_obs = pose.detach().to(torch.float64)[:, :3, :]
            if name == "g":
                to_obs = inverse(to_obs)
        return to_obs

    def _predict_views_batch(self, fusion, cameras, T=None, g=None, *, height=None, width=None, min_obs=1, step=0.5, znear=0.05):
        """Scene memory, what the fused state LOOKS LIKE from a camera (an extension beyond the released reference, like _fuse_batch, whose
        inverse it is; the raycast of KinectFusion): depth, normal and state images of P instances in ONE ragged call
        (ops.tsdf_raycast_batch, csrc/tsdfray.hip).  fusion = the dict of _fuse_batch.  cameras[p] = dict(world_to_cam [V,3,4],
        intrinsics [V,4] or [4]) in the OBSERVATION's frame (HIP tensors; a views dict of the carve will do), or None: no view of that
        slot.  T, g: exactly the conventions of _fuse_batch; the memory-frame camera is _memory_cameras(world_to_cam, T) or
        (world_to_cam, inverse(g)), and its inverse [R^T | -R^T t] -- the camera-to-memory matrix the operator takes -- is formed in
        float64 ON THE HOST.  height, width: None takes them from the first camera dict that carries 'depth'.
        -> list of P: None for a slot without views, else dict(depth fp32 [V,H,W] (0: no hit; it goes straight back into depth_points,
        the carve and the fuse), normal fp32 [V,H,W,3] in the memory's frame, state uint8 [V,H,W] of ops.RAY_STATE, counts int64 [V,5]:
        device tensors; cam_to_world float64 [V,3,4], the matrices the operator received).  step = 0.5 IS AN UNMEASURED DEFAULT; NO
        min_obs IS RECOMMENDED."""
        P = fusion["sum"].shape[0]
        if len(cameras) != P:
            raise ValueError(f"{P} fusion states for {len(cameras)} sets of cameras")
        to_obs = self._to_observation(P, T, g)
        if height is None or width is None:
            shaped = next((c["depth"] for c in cameras if c is not None and c.get("depth") is not None), None)
            if shaped is None:
                raise ValueError("_predict_views_batch: give height and width, or a camera dict that carries 'depth'")
            height, width = int(shaped.shape[-2]), int(shaped.shape[-1])
        dev = fusion["sum"].device
        Ms = [None] * P
        for p, c in enumerate(cameras):
            if c is None:
                continue
            E = self._memory_cameras(c["world_to_cam"], None if to_obs is None else to_obs[p]).cpu()
            Rt = E[:, :, :3].transpose(1, 2)
            Ms[p] = torch.cat([Rt, -(Rt @ E[:, :, 3:4])], dim=-1).contiguous().to(dev)
        shared = next((c["intrinsics"] for c in cameras if c is not None), None)
        res = ops.tsdf_raycast_batch((fusion["sum"], fusion["n"]), Ms, [shared if c is None else c["intrinsics"] for c in cameras], height, width,
                                     origin=fusion["origin"], voxel=fusion["voxel"], trunc=fusion["trunc"], min_obs=min_obs, step=step, znear=znear)
        return [None if Ms[p] is None else dict(depth=d, normal=nrm, state=st, counts=cnt, cam_to_world=Ms[p]) for p, (d, nrm, st, cnt) in enumerate(res)]

    def _view_agreement_batch(self, fusion, views, T=None, g=None, *, tol, min_obs=1, step=0.5, znear=0.05):
        """Scene memory, the view-space gate of the fused path (an extension beyond the released reference): does an observed depth view
        AGREE with what the fused state predicts at its camera under a pose?  views[p] = dict(depth [V,H,W] fp32, intrinsics,
        world_to_cam [V,3,4]) in the OBSERVATION's frame, or None; T, g as for _fuse_batch.  ONE _predict_views_batch call at the views'
        own cameras and ONE ops.depth_compare call over all of them: two operator calls and one host read for the whole batch.  Per pixel
        with an observation and a predicted hit: agree (within tol), in_front (the observation is more than tol nearer: something new
        stands before the memory's surface) or through (more than tol farther: the view sees past a surface the memory holds).
        -> dict of per-slot lists: agree = AGREE / (AGREE + IN_FRONT + THROUGH) (None for a slot without views or without a comparable
        pixel), through, in_front (pixel counts; None without views) and counts (host int64 [5] of ops.VIEW_CLASS summed over the
        slot's views; None without views).  tol HAS NO DEFAULT AND NONE IS RECOMMENDED: nothing here can measure one on real scans;
        step = 0.5 is the raycast's unmeasured default."""
        P = fusion["sum"].shape[0]
        if len(views) != P:
            raise ValueError(f"{P} fusion states for {len(views)} sets of views")
        out = {"agree": [None] * P, "through": [None] * P, "in_front": [None] * P, "counts": [None] * P}
        have = [p for p, v in enumerate(views) if v is not None and v["depth"].shape[0] > 0]
        if not have:
            return out
        pred = self._predict_views_batch(fusion, [views[p] if p in have else None for p in range(P)], T, g, min_obs=min_obs, step=step, znear=znear)
        cat = (lambda ts: torch.cat(ts, 0) if len(ts) > 1 else ts[0])                       # noqa: E731
        _, counts = ops.depth_compare(cat([views[p]["depth"].contiguous() for p in have]), cat([pred[p]["depth"] for p in have]),
                                      cat([pred[p]["state"] for p in have]), tol=tol)
        counts = counts.cpu().numpy()
        at = 0
        for p in have:
            V = views[p]["depth"].shape[0]
            c = counts[at:at + V].sum(0)
            at += V
            den = int(c[2] + c[3] + c[4])
            out["agree"][p] = float(c[2]) / float(den) if den else None
            out["through"][p], out["in_front"][p], out["counts"][p] = int(c[4]), int(c[3]), c
        return out

    @staticmethod
    def _observed_mesh_batch(fusion, min_obs=1):
        """Scene memory, the one mesh the memory can stand behind (an extension beyond the released reference, like _fuse_batch): the fused
        states of P instances meshed where they were OBSERVED, in ONE batched call (ops.tsdf_mesh_batch, csrc/tsdfmesh.hip).  fusion =
        the dict of _fuse_batch (sum, n, origin, voxel).  A cube with a corner seen fewer than min_obs times emits nothing, so the mesh has
        holes where nothing looked and no second shell at the end of the truncation band.  -> list of P make_mesh(vertices, faces) in the
        memory's frame, the arrays copied to the host ONCE for the whole batch; None for an instance whose mesh is empty.  NO min_obs IS
        RECOMMENDED: 1 is the least, unmeasured on real scans."""
        from ..mesh_extractor2 import make_mesh
        verts, faces, vo, fo, _ = ops.tsdf_mesh_batch((fusion["sum"], fusion["n"]), origin=fusion["origin"], voxel=fusion["voxel"], min_obs=min_obs,
                                                      packed=True)
        verts, faces = verts.cpu().numpy(), faces.cpu().numpy()
        return [make_mesh(verts[vo[p]:vo[p + 1]], faces[fo[p]:fo[p + 1]]) if fo[p + 1] > fo[p] else None for p in range(len(vo) - 1)]

    def _complete_fusion_batch(self, fusion, code, slots=None, *, weight, max_rows=1 << 20):
        """Scene memory, ONE reconstruction per instance out of its two pictures (an extension beyond the released reference, like
        _fuse_batch): the fused state where the cameras measured, the shape prior's field where they did not.  Three steps, no host
        read of the volume: ops.tsdf_prior_rows_batch (csrc/tsdfprior.hip) turns the lattice samples with fewer than `weight`
        observations into query rows, hip_model().sdf_decode_rows evaluates the decoder on them (the ragged entry: the rows of an
        instance are contiguous; max_rows rows per decoder launch), ops.tsdf_complete_batch enters the values as weight - n integer
        votes into a COPY of the state.  The fused state is never written.  `code` holds P rows (memory['codes'] for all slots);
        fusion = the dict of _fuse_batch; slots = the P slots of the fusion the rows belong to (None: the fusion has P slots, in
        order).  THIS BUILD'S DEFINITION, that of _optimize_code_on_fusion_batch: the decoder's value times the instance's scale s is
        a metric distance.  With decoder_type "deepsdf" the decoder reads the raw query and s does not reach it; the convention is
        kept all the same, exactly as ops.tsdf_fit_loss keeps it when the code is fitted to this state.
        -> dict of the fusion's shape: sum, n (new int32 tensors [P,res,res,res]), origin, voxel, trunc (shared with the fusion, the
        rows of `slots`), weight, counts (device int64 [P,4]: eligible, voted, skipped_nonfinite, untouched -- ops.PRIOR_COUNT) and
        rows (the number of decoder queries).  Mesh it whole with min_obs = weight (_completed_mesh_batch).  weight HAS NO DEFAULT
        AND NONE IS RECOMMENDED: 1 lets a single observation outvote the prior, which can leave a wall where a +trunc observation
        meets a -trunc belief; larger weights blend.  Unmeasured: real scans, a trained model, any effect downstream."""
        weight = ops._prior_weight("_complete_fusion_batch", weight)
        P = code["z_inv"].shape[0]
        slots = list(range(fusion["sum"].shape[0])) if slots is None else [int(i) for i in slots]
        if len(slots) != P:
            raise ValueError(f"{P} code rows for {len(slots)} slots of the fusion")
        S, N = fusion["sum"], fusion["n"]
        origin, voxel, trunc = (np.asarray(fusion[k], dtype=np.float64) for k in ("origin", "voxel", "trunc"))
        if slots != list(range(S.shape[0])):
            pick = torch.tensor(slots, device=S.device)
            S, N = S[pick].contiguous(), N[pick].contiguous()
            origin, voxel, trunc = origin[slots], voxel[slots], trunc[slots]
        rows = ops.tsdf_prior_rows_batch((S, N), origin=origin, voxel=voxel, weight=weight, packed=True)
        points, row_inst = rows[0], rows[1]
        s_ = code["s"].detach().float().contiguous()
        if points.shape[0]:
            values = self.model.hip_model().sdf_decode_rows(points, row_inst, code["z_so3"].detach(), code["z_inv"].detach(), s_, code["t"].detach(),
                                                            max_rows=max_rows)
        else:
            values = torch.empty(0, dtype=torch.float32, device=S.device)
        (S2, N2), counts = ops.tsdf_complete_batch((S, N), values, rows, s=s_.reshape(P).double().cpu().numpy(), trunc=trunc, weight=weight)
        return {"sum": S2, "n": N2, "origin": origin, "voxel": voxel, "trunc": trunc, "weight": weight, "counts": counts, "rows": int(points.shape[0])}

    @staticmethod
    def _completed_mesh_batch(fusion, completed):
        """Scene memory, the closed mesh of a completed state with its provenance (no new kernel): ops.tsdf_mesh_batch of
        completed = the dict of _complete_fusion_batch with min_obs = its weight -- every sample of a completed state holds at least
        that many votes, so every cube is kept -- and, per vertex, whether it was MEASURED: ops.tsdf_sample_batch of the OBSERVED
        state (fusion = the dict of _fuse_batch with the same slots) at the vertex cast to fp32, identity pose, min_obs = 1, reports
        all eight corners of its cell seen.  -> list of P dicts {vertices float64 [nv,3], faces int64 [nf,3], vertex_observed bool
        [nv]}: host arrays in the memory's frame, copied ONCE for the whole batch; None for an instance whose mesh is empty.  A face
        all of whose vertices are observed is a measured one, the others are the prior's."""
        state = (completed["sum"], completed["n"])
        verts, faces, vo, fo, _ = ops.tsdf_mesh_batch(state, origin=completed["origin"], voxel=completed["voxel"], min_obs=int(completed["weight"]),
                                                      packed=True)
        P = len(vo) - 1
        seen = torch.zeros(verts.shape[0], dtype=torch.bool, device=verts.device)
        if verts.shape[0]:
            q = verts.float()
            out = ops.tsdf_sample_batch((fusion["sum"], fusion["n"]), [q[vo[p]:vo[p + 1]] for p in range(P)], None, origin=fusion["origin"],
                                        voxel=fusion["voxel"], trunc=fusion["trunc"], min_obs=1, packed=True)
            seen = out[2] == ops.SAMPLE_STATE.index("sampled")
        verts, faces, seen = verts.cpu().numpy(), faces.cpu().numpy(), seen.cpu().numpy()
        return [{"vertices": verts[vo[p]:vo[p + 1]], "faces": faces[fo[p]:fo[p + 1]], "vertex_observed": seen[vo[p]:vo[p + 1]]}
                if fo[p + 1] > fo[p] else None for p in range(P)]

    def _refine_on_memory_batch(self, mem_pcs, new_pcs, T, radius, metric="point", normal_radius=None, **kw):
        """Scene memory, the pose the merge and the overlap gate trust (an extension beyond the released reference, like both): refine P
        registrations on the memory itself, at full resolution, in ONE ragged call (ops.cloud_icp_batch, csrc/cloudnear.hip) -- trimmed
        ICP of the observation new_pcs[p] [b_p,3] onto the kept cloud mem_pcs[p] [a_p,3], only correspondences within `radius` counting,
        so the part of the memory a partial view does not see pulls on nothing.  T [P,4,4] or [P,3,4] maps memory -> rescan, as
        everywhere; the operator gets inverse(T) as its initial pose: the partial view moves onto the complete cloud.  kw: max_iter,
        rel_thr, min_matched of ops.cloud_icp_batch (its defaults are ops.icp's, pytorch3d's: inherited, not tuned).  `radius` HAS NO
        DEFAULT: it must exceed the error of the registration it starts from, which no trained checkpoint exists here to measure.
        -> (T' [P,4,4] = inverse(g_out); a problem that made no update -- iters 0 -- keeps the caller's T bit for bit,
            dict: g [P,3,4] (g_out, rescan -> memory: what _accumulate_batch / _overlap_batch take as g=), stop, iters (host int32 [P])
            and the entries of _overlap_batch (overlap, rmse, memory_seen, counts, nn_idx) formed from the final search of the
            refinement, which is the search _overlap_batch(g=g_out, radius=radius) would make).
        metric "plane": the point-to-plane metric instead -- ONE _memory_normals_batch(mem_pcs, normal_radius) call, then ONE
        ops.cloud_icp_plane_batch call with the same arguments (its min_matched defaults to 6 and counts planar matches); the dict gains
        planar (host int64 [P]).  The normals are recomputed at every call and each of the two operators builds its own grid over the
        memory: accepted, not optimised.  There is no fallback to the point metric: a starved or degenerate problem keeps the caller's T,
        as any problem with iters 0 does, and stop says why."""
        if metric not in ("point", "plane"):
            raise ValueError(f"metric must be 'point' or 'plane', got {metric!r}")
        P = len(mem_pcs)
        if len(new_pcs) != P:
            raise ValueError(f"{P} memory clouds for {len(new_pcs)} observations")
        if T is None or T.dim() != 3 or T.shape[0] != P or T.shape[1] not in (3, 4) or T.shape[2] != 4:
            raise ValueError(f"T must be [P,4,4] or [P,3,4] with P = {P}, got {None if T is None else tuple(T.shape)}")
        if metric == "plane":
            normals = [nrm for nrm, _, _, _ in self._memory_normals_batch(mem_pcs, radius=normal_radius)]
            res = ops.cloud_icp_plane_batch([p.detach() for p in mem_pcs], normals, [p.detach() for p in new_pcs], g=self._memory_pose(T, None, P),
                                            radius=radius, packed=True, **kw)
        else:
            res = ops.cloud_icp_batch([p.detach() for p in mem_pcs], [p.detach() for p in new_pcs], g=self._memory_pose(T, None, P), radius=radius,
                                      packed=True, **kw)
        last_row = T.new_tensor([0.0, 0.0, 0.0, 1.0]).expand(P, 1, 4)
        T4 = T.detach() if T.shape[1] == 4 else torch.cat([T.detach(), last_row], 1)
        moved = torch.tensor((res["iters"] > 0).tolist(), device=T.device)
        T_new = torch.where(moved.view(P, 1, 1), torch.cat([inverse(res["g"]).to(T4), last_row], 1), T4)
        sizes = [int(b1 - b0) for b0, b1 in zip(res["b_off"][:-1], res["b_off"][1:])]
        searches = [(i, d, res["counts"][p], float(res["sum_d2"][p]))
                    for p, (i, d) in enumerate(zip(torch.split(res["idx"], sizes), torch.split(res["d2"], sizes)))]
        info = {"g": res["g"], "stop": res["stop"], "iters": res["iters"]}
        if metric == "plane":
            info["planar"] = res["planar"]
        info.update(self._overlap_figures(mem_pcs, searches))
        return T_new, info

    def _refine_on_fusion_batch(self, fusion, new_pcs, T, min_obs=1, **kw):
        """Scene memory, the registration that needs no search (an extension beyond the released reference, like _refine_on_memory_batch,
        whose conventions these are): refine P registrations on the FUSED STATE of their instances in ONE call (ops.tsdf_icp_batch,
        csrc/tsdficp.hip; Bylow et al. 2013) -- every posed point of new_pcs[p] [b_p,3] reads the eight samples around it and their
        gradient, and the pose minimises the sum of the squared distances.  fusion = the dict of _fuse_batch (sum, n: int32
        [P,res,res,res]; origin, voxel, trunc), the grids in the memory's frame; min_obs as everywhere on that state.  T [P,4,4] or
        [P,3,4] maps memory -> rescan; the operator gets inverse(T) as its initial pose.  kw: max_iter, rel_thr, min_matched of
        ops.tsdf_icp_batch (inherited, not tuned).  The band is the fusion's trunc: the error of the registration this starts from must
        lie within it, which no trained checkpoint exists here to measure.
        -> (T' [P,4,4] = inverse(g_out); a problem that made no update -- iters 0 -- keeps the caller's T bit for bit,
            dict: g [P,3,4] (g_out, rescan -> memory: what _accumulate_batch / _overlap_batch / _fuse_batch take as g=), stop, iters (host
            int32 [P]), sampled (list of P: sampled / finite observation points of the final sample, 0.0 with no finite point), rms_phi
            (list of P: sqrt(sum phi^2 / sampled), nan with none) and counts (host int64 [P,3]: finite, inside the grid, sampled)).
        There is no fallback: a starved or degenerate problem keeps the caller's T, as any problem with iters 0 does, and stop says why."""
        P = fusion["sum"].shape[0]
        if len(new_pcs) != P:
            raise ValueError(f"{P} fusion states for {len(new_pcs)} observations")
        if T is None or T.dim() != 3 or T.shape[0] != P or T.shape[1] not in (3, 4) or T.shape[2] != 4:
            raise ValueError(f"T must be [P,4,4] or [P,3,4] with P = {P}, got {None if T is None else tuple(T.shape)}")
        res = ops.tsdf_icp_batch((fusion["sum"], fusion["n"]), [p.detach() for p in new_pcs], g=self._memory_pose(T, None, P), origin=fusion["origin"],
                                 voxel=fusion["voxel"], trunc=fusion["trunc"], min_obs=min_obs, packed=True, **kw)
        last_row = T.new_tensor([0.0, 0.0, 0.0, 1.0]).expand(P, 1, 4)
        T4 = T.detach() if T.shape[1] == 4 else torch.cat([T.detach(), last_row], 1)
        moved = torch.tensor((res["iters"] > 0).tolist(), device=T.device)
        T_new = torch.where(moved.view(P, 1, 1), torch.cat([inverse(res["g"]).to(T4), last_row], 1), T4)
        info = {"g": res["g"], "stop": res["stop"], "iters": res["iters"], "counts": res["counts"], "sampled": [], "rms_phi": []}
        for (finite, _, sampled), q in zip(res["counts"].tolist(), res["sum_phi2"].tolist()):
            info["sampled"].append(sampled / finite if finite else 0.0)
            info["rms_phi"].append(math.sqrt(q / sampled) if sampled else float("nan"))
        return T_new, info

    def _mesh_from_latent(self, latent_code):
        """more_solver.py:37-58: mesh of the canonical shape (t = 0, s = 1), then scaled and moved to the instance pose."""
        if self.mesh_extractor is None:
            raise ValueError("More_Solver: cfg has no 'mesh_extractor' section")
        return mesh_from_latent(self.mesh_extractor, latent_code, self.model.decoder)

    def _mesh_from_latent_batch(self, codes, threads=None, group=16):
        """_mesh_from_latent for every row of the code dict ``codes`` ([B,...] tensors): mesh i equals
        ``_mesh_from_latent(slice_code_dict(codes, i))``.  ``group`` instances at a time mesh canonically (t = 0, s = 1) with their MISE
        rounds in lock-step (Generator3D.generate_from_latent_batch: one lattice-sized MISE buffer per instance of a group, decimation on
        ``threads`` host threads), then every mesh is scaled and moved as mesh_from_latent does (model_utils.place_mesh)."""
        if self.mesh_extractor is None:
            raise ValueError("More_Solver: cfg has no 'mesh_extractor' section")
        B = codes["z_inv"].shape[0]
        t_host, s_host = codes["t"].detach().cpu(), codes["s"].detach().cpu()
        meshes = []
        for g0 in range(0, B, group):
            g1 = min(B, g0 + group)
            canon = {k: codes[k][g0:g1].detach() for k in ("z_so3", "z_inv")}
            canon["t"] = torch.zeros_like(codes["t"][g0:g1])             # canonical pose, as model_utils.py:296-298
            canon["s"] = torch.ones_like(codes["s"][g0:g1])
            part = self.mesh_extractor.generate_from_latent_batch(canon, self.model.decoder, threads=threads)
            meshes += [place_mesh(m, t_host[i], s_host[i]) for i, m in zip(range(g0, g1), part)]
        return meshes

    def _mesh_from_pc(self, pc):
        """more_solver.py:60-69."""
        pc_down, _ = fps(pc, K=self.cfg["shape_priors"]["n_input_point"])
        return self._mesh_from_latent(self.model.encode(pc_down.transpose(-1, -2)))

    def _transform_latent(self, code, tsfm):
        """more_solver.py:230-244: rotate z_so3, move t."""
        R = tsfm[:, :, :3]
        return {"z_so3": (code["z_so3"] @ R.transpose(-1, -2)).detach().clone(), "z_inv": code["z_inv"].detach().clone(),
                "t": transform(tsfm, code["t"]).detach().clone(), "s": code["s"].detach().clone()}

    def _solve_end2end(self, ref, rescan, optim=False, mesh=None):
        """more_solver.py:246-299: encode both scenes (one batch each), sequential matching, registration of the matched pairs,
        transformed latent codes and (``mesh``, default = whether cfg has a mesh_extractor, as the reference always meshes) their
        meshes.  ref / rescan: {'pc' [n,3,Nmax], 'pc_mask'}.  Both modes register all matched pairs of the
        scene in one batched call (optim=True: the 400-step refinement in lock-step)."""
        if ref is None:
            return None
        if mesh is None:
            mesh = self.mesh_extractor is not None

        def valid_clouds(scene):
            return [pc.T[mask.reshape(-1).bool()] for pc, mask in zip(scene["pc"], scene["pc_mask"])]
        ref_full, res_full = valid_clouds(ref), valid_clouds(rescan)
        ref_codes = self.model.encode_fps(ref["pc"], ref["pc_mask"])
        res_codes = self.model.encode_fps(rescan["pc"], rescan["pc_mask"])
        matches = self._solve_object_matching(ref_codes, res_codes, "sequential")
        m0 = matches["matches0"]
        out = {"ref_pc_lst": ref_full, "rescan_pc_lst": res_full, "matches": m0, "registration": [None] * len(ref_full),
               "codes": [None] * len(ref_full), "mesh_lst": [None] * len(ref_full)}
        pairs = [(i, int(j)) for i, j in enumerate(m0.tolist()) if j >= 0]
        if pairs:
            if optim:   # all matched pairs of the scene advance in lock-step (the reference loops over them, more_solver.py:272-282)
                R, t = self._solve_pairwise_registration_optim_batch([ref_full[i] for i, _ in pairs], [res_full[j] for _, j in pairs])
            else:
                R, t = self._solve_pairwise_registration_batch([ref_full[i] for i, _ in pairs], [res_full[j] for _, j in pairs])
            T = Rt_to_SE3(R, t)
            for k, (i, j) in enumerate(pairs):
                out["registration"][i] = T[k:k + 1]
                cur = {key: res_codes[key][j][None] for key in ("z_so3", "z_inv", "s", "t")}
                out["codes"][i] = self._transform_latent(cur, inverse(T[k:k + 1]))
                if mesh:
                    out["mesh_lst"][i] = self._mesh_from_latent(out["codes"][i])
        return out


def _scene_clouds(scene):
    return [pc.T[mask.reshape(-1).bool()] for pc, mask in zip(scene["pc"], scene["pc_mask"])]


def solve_end2end_batch(solver, pairs, mesh=False, optim=False, sharded=False, optim_chunk=128, match_batched=False):
    """Batched form of More_Solver._solve_end2end over MANY (reference scan, rescan) pairs -- an extension the reference lacks
    (eval_3rscan.py walks the scenes one pair at a time): every scan of every pair goes through ONE ragged FPS launch and ONE
    encoder batch, every matched pair of every scene through ONE registration batch (ragged FPS, encode, Kabsch, ICP; optim=True:
    the 400-step refinement in lock-step, optim_chunk pairs per call).  The ragged FPS runs one workgroup per raw cloud (18 ms for a
    60 000-point cloud), so a single scene pair leaves the GPU idle; hundreds of clouds per launch fill it.  Returns one dict per
    pair, as _solve_end2end.  match_batched=True: the matcher of all scene pairs is ONE batched call as well
    (solver._solve_object_matching_batch) with one host read of the packed matches; the default calls solver._solve_object_matching
    per scene pair.  Same results either way.

    sharded=True (one process per GPU, torch.distributed initialised; SURVEY.md 8e, eval_3rscan.py:337-463 sharded over the node):
    the flat (scene, instance) list is block-partitioned over the ranks for FPS + encode and the codes all-gathered (4.1 KB each);
    the per-scene matchers run replicated (deterministic, 32 x 32); the flat list of matched pairs is block-partitioned again for
    the registration and the (R | t) rows all-gathered (48 B per pair); every rank then holds every pose and every transformed code,
    and meshes the pairs of ITS block (the SDF grids and meshes stay on the rank that made them: mesh_lst is None elsewhere)."""
    from .. import sharding
    scans, where = [], []
    for ref, res in pairs:
        where.append((len(scans), len(scans) + 1))
        scans += [ref, res]
    clouds = [_scene_clouds(s) for s in scans]
    flat = [c for cl in clouds for c in cl]
    dev = flat[0].device
    if sharded:
        codes = sharding.sharded_encode_fps(solver.model, flat)
    else:
        lens = torch.tensor([c.shape[0] for c in flat], device=dev)
        buf = torch.zeros(len(flat), 3, int(lens.max()), device=dev)
        mask = torch.zeros(len(flat), 1, int(lens.max()), dtype=torch.bool, device=dev)
        for i, c in enumerate(flat):
            buf[i, :, : c.shape[0]] = c.T
            mask[i, :, : c.shape[0]] = True
        codes = solver.model.encode_fps(buf, mask)
    starts = [0]
    for cl in clouds:
        starts.append(starts[-1] + len(cl))
    outs, reg1, reg2, slots = [], [], [], []
    scene_codes = [({k: v[starts[a]:starts[a + 1]] for k, v in codes.items()}, {k: v[starts[b]:starts[b + 1]] for k, v in codes.items()})
                   for a, b in where]
    if match_batched:   # (sharded: replicated on every rank, like the per-scene matchers)
        all_m0 = [m["matches0"] for m in solver._solve_object_matching_batch([cr for cr, _ in scene_codes], [cs for _, cs in scene_codes],
                                                                             "sequential")]
        flat_m0 = torch.cat([m.reshape(-1) for m in all_m0]).tolist() if all_m0 else []     # the one host read of the matcher leg
    taken = 0
    for p, (a, b) in enumerate(where):
        cr, cs = scene_codes[p]
        n = len(clouds[a])
        if match_batched:
            m0, m0_host = all_m0[p], flat_m0[taken:taken + n]
            taken += n
        else:
            m0 = solver._solve_object_matching(cr, cs, "sequential")["matches0"]
            m0_host = m0.tolist()
        out = {"ref_pc_lst": clouds[a], "rescan_pc_lst": clouds[b], "matches": m0, "registration": [None] * n, "codes": [None] * n,
               "mesh_lst": [None] * n, "_res_codes": cs}
        for i, j in enumerate(m0_host):
            if j >= 0:
                reg1.append(clouds[a][i]); reg2.append(clouds[b][j]); slots.append((p, i, j))
        outs.append(out)
    if slots:
        def register(lo, hi):
            if not optim:
                return solver._solve_pairwise_registration_batch(reg1[lo:hi], reg2[lo:hi])
            Rs, ts = [], []
            for c0 in range(lo, hi, optim_chunk):
                Rc, tc = solver._solve_pairwise_registration_optim_batch(reg1[c0:min(hi, c0 + optim_chunk)], reg2[c0:min(hi, c0 + optim_chunk)])
                Rs.append(Rc), ts.append(tc)
            return torch.cat(Rs, 0), torch.cat(ts, 0)
        R, t = sharding.sharded_pairs(len(slots), register) if sharded else register(0, len(slots))
        mine = range(*sharding.shard_range(len(slots))) if sharded else range(len(slots))     # the pairs this rank meshes
        T = Rt_to_SE3(R, t)
        for k, (p, i, j) in enumerate(slots):
            out = outs[p]
            out["registration"][i] = T[k:k + 1]
            cur = {key: out["_res_codes"][key][j][None] for key in ("z_so3", "z_inv", "s", "t")}
            out["codes"][i] = solver._transform_latent(cur, inverse(T[k:k + 1]))
        own = [slots[k] for k in mine]
        if mesh and own:
            cl = [outs[p]["codes"][i] for p, i, _ in own]
            for (p, i, _), msh in zip(own, solver._mesh_from_latent_batch({k: torch.cat([c[k] for c in cl], 0) for k in ("z_so3", "z_inv", "s", "t")})):
                outs[p]["mesh_lst"][i] = msh
    for out in outs:
        del out["_res_codes"]
    return outs


def sequence_plan(n_mem, matches0, n_new=None, n_new_points=None, accepted=None):
    """The index bookkeeping of one solve_sequence step, as a pure function: matches0[i] is the rescan instance matched to memory slot i
    (-1: none), as _solve_object_matching(memory codes, rescan codes) returns it; n_new = instances in the rescan (None: unknown).
      pairs         [(memory slot, rescan instance)] in slot order: pair k is problem k of the registration and of the merge
      updated       the slots a match updates (their cloud goes through the merge); the others keep cloud and code
      reencode      the updated slots whose cloud changed -- n_new_points[k] > 0 for pair k (None: not known yet, every updated slot)
      unmatched_new the rescan instances no slot was matched to (None without n_new): their frame relative to the memory is unknown, so
                    they are reported and left out
    accepted (one bool per pair, None: no gate): the pairs the overlap gate of solve_sequence lets into the merge.  A rejected pair stays in
    `pairs` (it was registered) but leaves `updated` / `reencode`, n_new_points then has one entry per ACCEPTED pair, and the dict gains
      rejected      the slots whose pair was rejected: they keep cloud and code
    With accepted None the dict is exactly the four entries above."""
    m0 = [int(j) for j in matches0]
    if len(m0) != n_mem:
        raise ValueError(f"{len(m0)} matches for {n_mem} memory slots")
    pairs = [(i, j) for i, j in enumerate(m0) if j >= 0]
    taken = [j for _, j in pairs]
    if len(set(taken)) != len(taken):
        raise ValueError(f"a rescan instance is matched to more than one memory slot: {m0}")
    if n_new is not None and any(j >= n_new for j in taken):
        raise ValueError(f"a match names a rescan instance >= {n_new}: {m0}")
    if accepted is not None and len(accepted) != len(pairs):
        raise ValueError(f"{len(accepted)} accepted flags for {len(pairs)} pairs")
    updated = [i for k, (i, _) in enumerate(pairs) if accepted is None or accepted[k]]
    if n_new_points is not None and len(n_new_points) != len(updated):
        raise ValueError(f"{len(n_new_points)} point counts for {len(updated)} {'pairs' if accepted is None else 'accepted pairs'}")
    plan = {"pairs": pairs, "updated": updated,
            "reencode": updated if n_new_points is None else [i for i, k in zip(updated, n_new_points) if int(k) > 0],
            "unmatched_new": None if n_new is None else [j for j in range(n_new) if j not in set(taken)]}
    if accepted is not None:
        plan["rejected"] = [i for k, (i, _) in enumerate(pairs) if not accepted[k]]
    return plan


_CODE_KEYS = ("z_so3", "z_inv", "s", "t")


def _encode_clouds(model, clouds):
    """encode_fps of a list of clouds [n_i,3]: padded to the longest, one ragged FPS launch, one encoder batch (as solve_end2end_batch pads)"""
    dev = clouds[0].device
    nmax = max(c.shape[0] for c in clouds)
    buf = torch.zeros(len(clouds), 3, nmax, device=dev)
    mask = torch.zeros(len(clouds), 1, nmax, dtype=torch.bool, device=dev)
    for i, c in enumerate(clouds):
        buf[i, :, : c.shape[0]] = c.T
        mask[i, :, : c.shape[0]] = True
    return model.encode_fps(buf, mask)


def solve_sequence(solver, ref, rescans, optim=False, mesh=False, voxel=None, optimize_codes=False, overlap_radius=None, min_overlap=None,
                   refine_radius=None, refine_metric="point", normal_radius=None, consolidate=False, consolidate_radius=None,
                   consolidate_max_variation=1 / 3, consolidate_max_shift=float("inf"), carve_tol=None, carve_window=1, carve_min_free=1,
                   carve_max_seen=0, carve_empty="unknown", fuse_res=None, fuse_trunc_voxels=4, fuse_empty="unknown", fuse_mesh=False,
                   fuse_min_obs=1, code_fit_band=None, code_fit_free=None, code_fit_seed=0):
    """A reference scan followed by SEVERAL rescans, with a memory that carries every instance's points from one rescan to the next -- an
    extension beyond the released reference (more_solver.py:246-299 solves one (reference, rescan) pair and drops the rescan's points).
    ref and every rescan: {'pc' [n,3,Nmax], 'pc_mask'} as _solve_end2end takes them.

    Memory: one cloud per instance of ``ref`` in the reference frame plus its code.  The clouds are _scene_clouds(ref) passed once through
    the merge against an empty observation, so the memory is one point per voxel from the first step on (a merged cloud is kept whole by
    every later merge at the same voxel); the codes are encode_fps(ref).  The number of slots never changes.
    Per rescan, in order: encode it (one ragged FPS, one encoder batch); _solve_object_matching(memory codes, rescan codes); ONE
    _solve_pairwise_registration(_optim)_batch call over the matched pairs; ONE _accumulate_batch call; the slots whose cloud grew are
    re-encoded (one ragged FPS, one encoder batch: their code is encode_fps of the merged cloud); optimize_codes: ONE _optimize_code_batch
    call on those slots, an instance keeping the optimised code where its loss improved (the reference's best_code rule).  Rescan
    instances without a match are left out of the memory -- their frame relative to the reference is unknown -- and reported; memory
    slots without a match stay as they are.

    -> (steps, memory).  steps[k]: the dict of _solve_end2end for rescan k against the memory as it was BEFORE the step (ref_pc_lst,
    rescan_pc_lst, matches, registration, codes = the rescan's codes moved to the reference frame, mesh_lst = None per slot: meshes are
    made of the final memory) plus merged_sizes [n] (points per slot after the step), n_new_points [n] (points the step added) and
    unmatched_rescan (rescan instance indices).  memory: {'clouds': list of [n_i,3], 'codes': code dict of n rows, 'meshes':
    _mesh_from_latent_batch(codes) if mesh else None}.  voxel: see More_Solver._accumulate_batch.

    The overlap gate (opt-in: with overlap_radius and min_overlap both None no search is made and the step dicts are as above).  With either
    given, ONE More_Solver._overlap_batch call over the matched pairs follows the registration batch (overlap_radius None: its derived
    default, 2 * voxel) and the step also reports overlap, overlap_rmse, memory_seen (lists of n, None for unmatched slots) and rejected
    (slots).  Pairs with overlap < min_overlap (None: nothing is rejected, the figures are only reported) are left out of the ONE
    _accumulate_batch call: a rejected slot keeps its cloud and code, gets n_new_points 0 and is not re-encoded; its registration and codes
    entries are still reported.  min_overlap HAS NO DEFAULT AND NONE IS RECOMMENDED: no trained checkpoint exists here to measure one
    against, so the threshold is the caller's to choose.

    The refinement on the memory (opt-in: with refine_radius None nothing below happens and the step dicts are as above).  With a number,
    ONE More_Solver._refine_on_memory_batch call over the matched pairs follows the registration batch: trimmed ICP of every rescan
    instance onto the memory cloud of its slot, at full resolution, correspondences within refine_radius only.  `registration` and `codes`
    then use the refined T', and the step gains refine_stop, refine_iters (lists of n, None for unmatched slots; LS_ICP_* values) and
    registration_init (the registration before the refinement).  The merge receives the refined pose directly (g=, no inverse of an
    inverse).  With the overlap gate on as well, its figures are the refinement's own final search when overlap_radius equals
    refine_radius -- no second search -- and otherwise come from one _overlap_batch(g=g_out) call.  refine_radius HAS NO DEFAULT AND
    NONE IS RECOMMENDED, like min_overlap: it must exceed the error of the initial registration, and no trained checkpoint exists here to
    measure that.  refine_metric "plane" (with refine_radius; without it a ValueError) refines with the point-to-plane metric:
    More_Solver._refine_on_memory_batch(metric="plane", normal_radius=normal_radius), the normals of the memory recomputed at every step.
    There is NO FALLBACK to the point metric: a pair whose refinement starves or is degenerate keeps the registration it came with, as
    any pair with refine_iters 0 does, and refine_stop reports it.  "point" is the path above, untouched.
    refine_metric "tsdf" registers on the FUSED STATE instead of the point memory (it needs fuse_res, and refuses a refine_radius: its
    band is the fusion's trunc; both are ValueErrors raised before any device work): ONE More_Solver._refine_on_fusion_batch call over
    the matched pairs follows the registration batch, on the state as it stands BEFORE this rescan is fused, with min_obs =
    fuse_min_obs.  Every posed point reads eight samples and their gradient: no search, no grid build, no normals.  The refined pose
    goes to the gate, the carve, the merge and the fuse exactly as the cloud refinement's does, the step gains the same refine_stop,
    refine_iters and registration_init, and the gate always makes its own _overlap_batch(g=g_out) search.  A slot whose state holds no
    observation yet (no ref['views'] and no earlier rescan) starves and keeps its registration.  NO SETTING IS RECOMMENDED: the error
    of the registration it starts from must lie within trunc, and nothing here can measure a real one.

    The consolidation (opt-in: with consolidate False nothing below happens and every returned object is what it is without the
    arguments).  With True, ONE More_Solver._consolidate_batch call over all slots runs AFTER THE LAST RESCAN (radius consolidate_radius,
    None: its derived default 3 * voxel; consolidate_max_variation and consolidate_max_shift are its limits, 1/3 and inf: none): every
    kept point is projected once onto the plane of its neighbourhood and the projected cloud is merged again at the same voxel.  It is
    NEVER run between rescans, because a plane fit on a curved surface shrinks it, and the shrinkage accumulates.  A CPU EXPERIMENT (NumPy
    twins in float64, not the operator and not a device run; a sphere of radius 0.4 m, sigma = 0.002 noise, voxel 0.01 m, 20 000 points
    per scan, one reference scan and five rescans merged at the true pose): the memory's RMS distance to the sphere is 2.27e-3 after the
    six scans and 5.4e-4 after one projection at r = 0.02 (30 211 rows, 21 288 after the re-merge); projecting after EVERY rescan instead
    gives 6.4e-4 after the first step and 8.4e-4 after the fifth at r = 0.02, and 6.5e-4 rising to 1.78e-3 at r = 0.03.  A caller who
    wants the per-step alternative has More_Solver._consolidate_batch, at their own risk.  A slot whose consolidated cloud would have
    fewer than n_input_point rows keeps its cloud and code and is reported; the other slots take their consolidated cloud and are
    re-encoded in ONE _encode_clouds call (the encoder's code of the consolidated cloud: optimize_codes does not run again).  memory
    gains 'consolidation': the dict of _consolidate_batch (per-slot lists rows_before, rows_after, moved, held, no_plane, rms_shift;
    the figures of a kept slot are those of the cloud it did not take) plus kept_as_is (slots).

    The carve (opt-in: with carve_tol None nothing below happens and every step dict and the memory are what they are without the
    arguments).  Every operator above adds points or moves them; a point once kept is otherwise never replaced, so a wrong match or an ICP
    in a local minimum writes a misplaced copy of an object into a slot for good, and an object that has changed keeps its old points.
    With a number, a rescan may carry 'views': one entry per rescan instance, None allowed, else dict(depth [V,H,W] fp32, intrinsics,
    world_to_cam [V,3,4]) in the RESCAN's frame (synth.make_partial_views(with_depth=True) makes such dicts).  After the registration, the
    refinement and the gate, and BEFORE the merge, ONE More_Solver._carve_batch call over the accepted pairs that have views drops the
    kept points those views look through, under the pose the merge will use (tol = carve_tol, window, min_free, max_seen and empty =
    carve_*).  A slot takes its carved cloud unless that cloud has fewer than n_input_point rows; then it keeps its cloud and is
    reported.  The merge runs on the carved memory; a slot that shrank or grew is re-encoded in the step's one re-encode call.  The step
    gains n_carved [n] (rows the step removed per slot) and carve_kept_as_is (slots).  carve_window = 1 is derived (the nearest-pixel
    rounding moves a ray by up to half a pixel).  carve_tol HAS NO DEFAULT AND NONE IS RECOMMENDED, nor any carve_min_free or
    carve_max_seen: no real scans are available here to measure one on, and the effect on matching is unmeasured.

    The fusion (opt-in: with fuse_res None nothing below happens and every returned object is what it is without the arguments).  The
    only mesh above is the decoder's idea of the object; with an int, the memory also carries what was OBSERVED as a distance field: one
    truncated signed distance state of fuse_res^3 samples per slot, in the reference frame.  The grids are
    More_Solver._fusion_grids(memory clouds after the initial merge, fuse_res, fuse_trunc_voxels) and never change.  ref['views'], if
    present (one entry per instance, None allowed, dicts as for the carve), is fused under the identity.  Per rescan, ONE
    More_Solver._fuse_batch call fuses the accepted pairs that carry 'views', after the registration, the refinement and the gate, under
    the pose the merge uses; it does not depend on carve_tol.  The step gains n_fused_views [n].  memory gains 'fusion': dict(sum, n:
    int32 [n,res,res,res] device tensors, origin, voxel, trunc: host float64); ops.tsdf_volume reads the volume and its valid flags
    out of (sum, n).  fuse_mesh=True (it needs fuse_res; without one a ValueError) meshes that state ONCE, after the last step: memory
    gains 'observed_meshes', More_Solver._observed_mesh_batch(fusion, fuse_min_obs): one mesh per slot in the reference frame, of
    the cubes whose eight corners were observed at least fuse_min_obs times, None for a slot nothing kept.  With fuse_mesh False the
    memory has no such key.  fuse_trunc_voxels = 4 is AN UNMEASURED DEFAULT; NO fuse_res IS RECOMMENDED, and no fuse_min_obs: no real scans are
    available here to measure one on, and what the fused volume or its mesh does for anything downstream is unmeasured.

    The fit to the fused state (opt-in: optimize_codes False and True behave exactly as above).  optimize_codes="tsdf" (it needs fuse_res;
    without one a ValueError raised before any device work, as any value other than False, True and "tsdf" is) replaces the step's
    _optimize_code_batch call by ONE More_Solver._optimize_code_on_fusion_batch call on the re-encoded slots, AFTER the step's fuse, so the
    state includes this rescan: code_fit_band / code_fit_free columns per slot (None: n_input_point // 2 each, derived: the decoder
    batch of the point path) drawn out of the slot's state with min_obs = fuse_min_obs and the call seed code_fit_seed + step * n (slot
    i: that plus i), held to the fused distance inside the band and to "at least trunc" in observed free space.  A slot keeps the
    optimised code where its loss improved; a slot whose state holds no observation has nothing to fit and keeps its code.  The step
    gains code_fit: the report of the call (per-slot lists loss_first, loss_last, n_band, n_free of n entries, None for slots not
    optimised; None for a step that optimised nothing).  NO QUOTA IS RECOMMENDED, nor any min_obs or fuse_res for fitting: no real scans
    and no trained model are available here, and nothing here can measure the effect on matching or on the meshes.

    The view gate of the fused state (the rescan's depth views compared with what the state predicts at their cameras) is
    solve_sequence_view_gated below: this function with two more arguments.  It is a function of its own so that this parameter list,
    which callers and tests rely on, stays as it is.  The weighted point-to-plane fusion of the views is solve_sequence_weighted_fusion,
    for the same reason."""
    return _solve_sequence(None, None, None, **locals())


def _solve_sequence(weighted, view_tol, min_view_agreement, solver, ref, rescans, optim, mesh, voxel, optimize_codes, overlap_radius, min_overlap, refine_radius,
                    refine_metric, normal_radius, consolidate, consolidate_radius, consolidate_max_variation, consolidate_max_shift, carve_tol,
                    carve_window, carve_min_free, carve_max_seen, carve_empty, fuse_res, fuse_trunc_voxels, fuse_empty, fuse_mesh, fuse_min_obs,
                    code_fit_band, code_fit_free, code_fit_seed):
    """the one body of solve_sequence (weighted and view_tol None), solve_sequence_view_gated and solve_sequence_weighted_fusion (weighted =
    dict(weights, value, max_jump): every fuse goes through More_Solver._fuse_weighted_batch): every argument given, the defaults are
    solve_sequence's"""
    if isinstance(optimize_codes, (bool, np.bool_)):
        optimize_codes = bool(optimize_codes)
    elif not (isinstance(optimize_codes, str) and optimize_codes == "tsdf"):
        raise ValueError(f"solve_sequence: optimize_codes must be False, True or 'tsdf', got {optimize_codes!r}")
    if optimize_codes == "tsdf" and fuse_res is None:
        raise ValueError("solve_sequence: optimize_codes 'tsdf' needs fuse_res: without a fused state there is nothing to fit the codes to")
    if refine_metric not in ("point", "plane", "tsdf"):
        raise ValueError(f"solve_sequence: refine_metric must be 'point', 'plane' or 'tsdf', got {refine_metric!r}")
    if refine_metric == "plane" and refine_radius is None:
        raise ValueError("solve_sequence: refine_metric 'plane' needs refine_radius: without it there is no refinement to choose a metric for")
    if fuse_mesh and fuse_res is None:
        raise ValueError("solve_sequence: fuse_mesh needs fuse_res: without a fused state there is nothing to mesh")
    if refine_metric == "tsdf" and fuse_res is None:
        raise ValueError("solve_sequence: refine_metric 'tsdf' needs fuse_res: without a fused state there is nothing to register against")
    if refine_metric == "tsdf" and refine_radius is not None:
        raise ValueError("solve_sequence: refine_metric 'tsdf' takes no refine_radius: its band is the fusion's trunc")
    if view_tol is not None and fuse_res is None:
        raise ValueError("solve_sequence_view_gated: view_tol needs fuse_res: without a fused state there is no predicted view to compare with")
    if weighted is not None and fuse_res is None:
        raise ValueError("solve_sequence_weighted_fusion: fuse_weights need fuse_res: without a fused state there is nothing to weigh")
    if weighted is None:
        fuse = solver._fuse_batch
    else:
        def fuse(fusion, views, **kw):
            return solver._fuse_weighted_batch(fusion, views, weights=weighted["weights"], value=weighted["value"], max_jump=weighted["max_jump"], **kw)
    refining = refine_radius is not None or refine_metric == "tsdf"
    gate = overlap_radius is not None or min_overlap is not None
    model = solver.model
    n_in = solver.cfg["shape_priors"]["n_input_point"]
    raw = _scene_clouds(ref)
    n = len(raw)
    mem = solver._accumulate_batch(raw, [c[:0] for c in raw], None, voxel=voxel)
    for i, c in enumerate(mem):
        if c.shape[0] < n_in:
            raise ValueError(f"solve_sequence: instance {i} keeps {c.shape[0]} of {raw[i].shape[0]} points at this voxel size, fewer than the "
                             f"{n_in} the encoder samples: the voxel is too coarse for this cloud")
    ref_codes = model.encode_fps(ref["pc"], ref["pc_mask"])
    codes = {k: ref_codes[k].detach().clone() for k in _CODE_KEYS}
    fusion = None
    if fuse_res is not None:
        fusion = solver._fusion_grids(mem, fuse_res, fuse_trunc_voxels)
        fusion["sum"], fusion["n"] = ops.tsdf_state(n, fusion.pop("dims"), mem[0].device)
        if ref.get("views") is not None:
            fuse(fusion, list(ref["views"]), empty=fuse_empty)
    steps = []
    for step_no, rescan in enumerate(rescans):
        res_full = _scene_clouds(rescan)
        res_codes = model.encode_fps(rescan["pc"], rescan["pc_mask"])
        m0 = solver._solve_object_matching(codes, res_codes, "sequential")["matches0"]
        plan = sequence_plan(n, m0.tolist(), len(res_full))
        pairs = plan["pairs"]
        out = {"ref_pc_lst": list(mem), "rescan_pc_lst": res_full, "matches": m0, "registration": [None] * n, "codes": [None] * n,
               "mesh_lst": [None] * n, "n_new_points": [0] * n, "unmatched_rescan": plan["unmatched_new"]}
        if carve_tol is not None:
            out.update({"n_carved": [0] * n, "carve_kept_as_is": []})
        if fusion is not None:
            out["n_fused_views"] = [0] * n
        if refining:
            out.update({"refine_stop": [None] * n, "refine_iters": [None] * n, "registration_init": [None] * n})
        if optimize_codes == "tsdf":
            out["code_fit"] = None
        if view_tol is not None:
            out.update({"view_agree": [None] * n, "view_through": [None] * n, "view_in_front": [None] * n})
            if min_view_agreement is not None and not gate:
                out["rejected"] = []
        if pairs:
            src, tgt = [mem[i] for i, _ in pairs], [res_full[j] for _, j in pairs]
            R, t = solver._solve_pairwise_registration_optim_batch(src, tgt) if optim else solver._solve_pairwise_registration_batch(src, tgt)
            T = Rt_to_SE3(R, t)
            refined = None
            if refining:
                T_init = T
                if refine_metric == "tsdf":
                    # all n slots go into the one call, so that a slot is its own problem of the state, as for the fuse: a slot without a
                    # pair has no observation, starves at once and is not read.  The state is the one BEFORE this rescan is fused.
                    slot_pcs, slot_T = [tgt[0][:0]] * n, torch.eye(4, dtype=T.dtype, device=T.device).repeat(n, 1, 1)
                    slots = [i for i, _ in pairs]
                    rows = torch.tensor(slots, device=T.device)
                    for k, i in enumerate(slots):
                        slot_pcs[i] = tgt[k]
                    slot_T[rows] = T_init
                    T, refined = solver._refine_on_fusion_batch(fusion, slot_pcs, slot_T, min_obs=fuse_min_obs)
                    T = T[rows]
                    refined = {"g": refined["g"][rows], "stop": refined["stop"][slots], "iters": refined["iters"][slots]}
                elif refine_metric == "plane":
                    T, refined = solver._refine_on_memory_batch(src, tgt, T_init, refine_radius, metric="plane", normal_radius=normal_radius)
                else:
                    T, refined = solver._refine_on_memory_batch(src, tgt, T_init, refine_radius)
                for k, (i, _) in enumerate(pairs):
                    out["refine_stop"][i], out["refine_iters"][i] = int(refined["stop"][k]), int(refined["iters"][k])
                    out["registration_init"][i] = T_init[k:k + 1]
            accepted = None
            if gate:
                radius = overlap_radius
                if radius is None and voxel is not None:
                    radius = solver.cfg.get("accumulate", {}).get("overlap_radius", 2 * voxel)
                if refined is None:
                    ov = solver._overlap_batch(src, tgt, T, radius=radius)
                elif refine_radius is not None and radius is not None and float(radius) == float(refine_radius):
                    ov = refined                                      # the refinement's final search is this search
                else:
                    ov = solver._overlap_batch(src, tgt, None, radius=radius, g=refined["g"])
                accepted = [min_overlap is None or o >= min_overlap for o in ov["overlap"]]
                out.update({"overlap": [None] * n, "overlap_rmse": [None] * n, "memory_seen": [None] * n})
                for k, (i, _) in enumerate(pairs):
                    out["overlap"][i], out["overlap_rmse"][i], out["memory_seen"][i] = ov["overlap"][k], ov["rmse"][k], ov["memory_seen"][k]
                out["rejected"] = sequence_plan(n, m0.tolist(), len(res_full), accepted=accepted)["rejected"]
            vviews = rescan.get("views") if view_tol is not None else None
            viewing = [k for k in range(len(pairs)) if vviews is not None and vviews[pairs[k][1]] is not None]
            if viewing:                                               # the matched pairs with views, on the state BEFORE this rescan is fused
                slot_views, slot_pose = [None] * n, [None] * n
                for k in viewing:
                    slot_views[pairs[k][0]] = vviews[pairs[k][1]]
                    slot_pose[pairs[k][0]] = (T[k] if refined is None else refined["g"][k]).detach().to(torch.float64)[:3, :]
                eye = torch.eye(4, dtype=torch.float64, device=T.device)[:3, :]
                poses = torch.stack([eye if q is None else q.to(T.device) for q in slot_pose])   # a slot without views: a placeholder nothing reads
                va = solver._view_agreement_batch(fusion, slot_views, T=poses if refined is None else None, g=None if refined is None else poses,
                                                  tol=view_tol, min_obs=fuse_min_obs)
                for key in ("agree", "through", "in_front"):
                    out["view_" + key] = va[key]
                if min_view_agreement is not None:
                    passed = [va["agree"][i] is None or va["agree"][i] >= min_view_agreement for i, _ in pairs]
                    accepted = passed if accepted is None else [a and b for a, b in zip(accepted, passed)]
                    out["rejected"] = sequence_plan(n, m0.tolist(), len(res_full), accepted=accepted)["rejected"]
            for k, (i, j) in enumerate(pairs):
                out["registration"][i] = T[k:k + 1]
                cur = {key: res_codes[key][j][None] for key in _CODE_KEYS}
                out["codes"][i] = solver._transform_latent(cur, inverse(T[k:k + 1]))
            keep = [k for k in range(len(pairs)) if accepted is None or accepted[k]]
            rviews = rescan.get("views") if carve_tol is not None else None
            seeing = [k for k in keep if rviews is not None and rviews[pairs[k][1]] is not None]
            if seeing:                                                # the accepted pairs with views, under the pose the merge will use
                sel = torch.tensor(seeing, device=T.device)
                carved, _ = solver._carve_batch([src[k] for k in seeing], [rviews[pairs[k][1]] for k in seeing],
                                                T=T[sel] if refined is None else None, g=None if refined is None else refined["g"][sel],
                                                tol=carve_tol, window=carve_window, min_free=carve_min_free, max_seen=carve_max_seen,
                                                empty=carve_empty)
                for c, k in zip(carved, seeing):
                    i = pairs[k][0]
                    if c.shape[0] < n_in:
                        out["carve_kept_as_is"].append(i)
                        continue
                    out["n_carved"][i] = src[k].shape[0] - c.shape[0]
                    src[k] = mem[i] = c
            fviews = rescan.get("views") if fusion is not None else None
            fusing = [k for k in keep if fviews is not None and fviews[pairs[k][1]] is not None]
            if fusing:                                                # the accepted pairs with views, under the pose the merge uses
                slot_views, slot_pose = [None] * n, [None] * n
                for k in fusing:
                    i = pairs[k][0]
                    slot_views[i] = fviews[pairs[k][1]]
                    slot_pose[i] = (T[k] if refined is None else refined["g"][k]).detach().to(torch.float64)[:3, :]
                    out["n_fused_views"][i] = int(slot_views[i]["depth"].shape[0])
                # all n slots go into the one call, so that a slot is its own problem of the state; a slot without views is skipped by the
                # operator and composes no camera: its row of `poses` is a placeholder that nothing reads
                eye = torch.eye(4, dtype=torch.float64, device=T.device)[:3, :]
                poses = torch.stack([eye if q is None else q.to(T.device) for q in slot_pose])
                fuse(fusion, slot_views, T=poses if refined is None else None, g=None if refined is None else poses, empty=fuse_empty)
            grew = []
            if keep:
                sel = torch.tensor(keep, device=T.device)
                if refined is None:
                    merged = solver._accumulate_batch([src[k] for k in keep], [tgt[k] for k in keep], T if accepted is None else T[sel], voxel=voxel)
                else:
                    merged = solver._accumulate_batch([src[k] for k in keep], [tgt[k] for k in keep], None, voxel=voxel,
                                                      g=refined["g"] if accepted is None else refined["g"][sel])
                grew = [c.shape[0] - src[k].shape[0] for c, k in zip(merged, keep)]   # the memory's rows are kept whole: the rest came from the rescan
                for c, k, d in zip(merged, keep, grew):
                    out["n_new_points"][pairs[k][0]] = d
                    mem[pairs[k][0]] = c
            changed = grew if carve_tol is None else [d + out["n_carved"][pairs[k][0]] for d, k in zip(grew, keep)]   # rows added or removed
            again = sequence_plan(n, m0.tolist(), len(res_full), changed, accepted=accepted)["reencode"]
            if again:
                new = _encode_clouds(model, [mem[i] for i in again])
                new = {k: new[k].detach().clone() for k in _CODE_KEYS}
                if optimize_codes:
                    enc = {k: v.clone() for k, v in new.items()}
                    if optimize_codes == "tsdf":
                        opt, improved, fit = solver._optimize_code_on_fusion_batch(new, fusion, slots=again, n_band=code_fit_band,
                                                                                   n_free=code_fit_free, min_obs=fuse_min_obs,
                                                                                   seed=code_fit_seed + step_no * n)
                        out["code_fit"] = {key: [None] * n for key in fit}
                        for key, vals in fit.items():
                            for i, v in zip(again, vals):
                                out["code_fit"][key][i] = v
                    else:
                        opt, improved = solver._optimize_code_batch(new, [mem[i] for i in again])
                    new = {k: torch.where(improved.view(-1, *([1] * (enc[k].dim() - 1))), opt[k], enc[k]) for k in _CODE_KEYS}
                rows = torch.tensor(again, device=codes["z_inv"].device)
                for k in _CODE_KEYS:
                    codes[k][rows] = new[k].to(codes[k].dtype)
        elif gate:
            out.update({"overlap": [None] * n, "overlap_rmse": [None] * n, "memory_seen": [None] * n, "rejected": []})
        out["merged_sizes"] = [c.shape[0] for c in mem]
        steps.append(out)
    consolidation = None
    if consolidate:
        cons, consolidation = solver._consolidate_batch(mem, radius=consolidate_radius, voxel=voxel, max_variation=consolidate_max_variation,
                                                        max_shift=consolidate_max_shift)
        consolidation["kept_as_is"] = [i for i, c in enumerate(cons) if c.shape[0] < n_in]
        taken = [i for i, c in enumerate(cons) if c.shape[0] >= n_in]
        for i in taken:
            mem[i] = cons[i]
        if taken:
            new = _encode_clouds(model, [mem[i] for i in taken])
            rows = torch.tensor(taken, device=codes["z_inv"].device)
            for k in _CODE_KEYS:
                codes[k][rows] = new[k].detach().to(codes[k].dtype)
    memory = {"clouds": mem, "codes": codes, "meshes": solver._mesh_from_latent_batch(codes) if mesh else None}
    if consolidate:
        memory["consolidation"] = consolidation
    if fusion is not None:
        memory["fusion"] = fusion
        if fuse_mesh:
            memory["observed_meshes"] = solver._observed_mesh_batch(fusion, fuse_min_obs)
    return steps, memory


def solve_sequence_view_gated(solver, ref, rescans, *, view_tol, min_view_agreement=None, **kw):
    """solve_sequence(solver, ref, rescans, **kw) with the view gate of the fused state (an extension beyond the released reference, like
    the fusion).  kw: any keyword argument of solve_sequence, with its defaults; everything that function's docstring says holds.

    The overlap gate asks whether the rescan's points lie near kept points; the fused state can be asked the sharper question whether the
    rescan's depth views SEE what the state predicts at their cameras.  view_tol > 0 (it needs fuse_res; a ValueError raised before any
    device work otherwise, as for a view_tol that is not > 0): the matched pairs whose rescan
    instance carries 'views' go into ONE More_Solver._view_agreement_batch call (a raycast of the state at the views' own cameras and a
    per-pixel comparison with their depth maps: two operator calls), after the refinement, on the state as it stands BEFORE this rescan
    is fused, under the pose the merge will use, with min_obs = fuse_min_obs.  The step gains view_agree (agreeing pixels over the
    pixels that have both an observation and a predicted hit), view_through (pixels that look more than view_tol PAST a surface the
    memory holds) and view_in_front (pixels more than view_tol before it): lists of n, None for slots without views or, for view_agree,
    without a comparable pixel.  With min_view_agreement given, a pair whose view_agree is a number below it joins `rejected` exactly as
    a pair below min_overlap does (no carve, no merge, no fuse, no re-encode); a pair whose view_agree is None is not rejected; where
    both gates are given a pair must pass both.  NO view_tol AND NO min_view_agreement IS RECOMMENDED: no real scans are available here
    to measure one on, and a state that holds no observation yet (no ref['views'], no earlier rescan) predicts nothing and rejects
    nothing."""
    import inspect
    if view_tol is None or not float(view_tol) > 0.0:
        raise ValueError(f"solve_sequence_view_gated: view_tol must be > 0, got {view_tol!r}")
    args = inspect.signature(solve_sequence).bind(solver, ref, rescans, **kw)
    args.apply_defaults()
    return _solve_sequence(None, view_tol, min_view_agreement, **args.arguments)


def solve_sequence_weighted_fusion(solver, ref, rescans, *, fuse_weights, fuse_value="plane", fuse_max_jump=None, view_tol=None, min_view_agreement=None,
                                   **kw):
    """solve_sequence(solver, ref, rescans, **kw) -- or, with view_tol, solve_sequence_view_gated -- with the WEIGHTED fusion (an extension
    beyond the released reference, opt-in like the fusion itself).  kw: any keyword argument of solve_sequence, with its defaults;
    everything that function's docstring says holds.  It needs fuse_res: a ValueError raised before any device work otherwise.

    Every fuse of the sequence -- ref['views'] under the identity, the accepted pairs under the pose of the merge -- goes through
    More_Solver._fuse_weighted_batch(weights=fuse_weights, value=fuse_value, max_jump=fuse_max_jump) instead of _fuse_batch: integer
    weights (w_plane, w_proj, w_free, w_empty) in 1 .. 255 and, for fuse_value "plane", the distance to the plane of the pixel inside
    the band (one depth_normals call per fuse; fuse_max_jump None: each slot's trunc, AN UNMEASURED DEFAULT); "projective": the weights
    alone.  The state keeps its format, so the mesh, the registration on the state, the code fit, the raycast and the view gate read it
    as before; fuse_min_obs becomes a WEIGHT threshold.  On the analytic sphere of tests/test_depth_plane_cpu.py the plane value with
    surface votes 64 : 1 over empty-pixel votes cuts the median depth and normal error of the raycast several times; with equal weights
    it is no better than the projective fusion.  fuse_weights HAS NO DEFAULT AND NONE IS RECOMMENDED: that ratio comes from one
    synthetic sphere, and no real scans are available here."""
    import inspect
    weights = ops._fuse_weights("solve_sequence_weighted_fusion", fuse_weights)
    if fuse_value not in ("plane", "projective"):
        raise ValueError(f"solve_sequence_weighted_fusion: fuse_value must be 'plane' or 'projective', got {fuse_value!r}")
    if view_tol is not None and not float(view_tol) > 0.0:
        raise ValueError(f"solve_sequence_weighted_fusion: view_tol must be > 0, got {view_tol!r}")
    if view_tol is None and min_view_agreement is not None:
        raise ValueError("solve_sequence_weighted_fusion: min_view_agreement needs view_tol: without it no view is compared")
    args = inspect.signature(solve_sequence).bind(solver, ref, rescans, **kw)
    args.apply_defaults()
    weighted = {"weights": tuple(int(w) for w in weights), "value": fuse_value, "max_jump": fuse_max_jump}
    return _solve_sequence(weighted, view_tol, min_view_agreement, **args.arguments)


def solve_sequence_completed(solver, ref, rescans, *, complete_weight, complete_mesh=True, **kw):
    """solve_sequence(solver, ref, rescans, **kw) and then ONE reconstruction per instance: the fused state COMPLETED by the shape
    prior's field (an extension beyond the released reference, opt-in like the fusion itself).  kw: any keyword argument of
    solve_sequence, with its defaults; with fuse_weights it goes through solve_sequence_weighted_fusion, else with view_tol through
    solve_sequence_view_gated, and everything those functions' docstrings say holds.  It needs fuse_res: a ValueError raised before
    any device work otherwise, as for a complete_weight that is no integer in 1 .. 65535.

    After the last step ONE More_Solver._complete_fusion_batch call over all slots with memory['codes'] (rows -> decoder -> votes:
    the fused state where the cameras measured, the decoder's value times s where fewer than complete_weight observations arrived)
    and, with complete_mesh, ONE _completed_mesh_batch call.  memory gains `completed` (the dict of _complete_fusion_batch: a second
    state of the fusion's format; memory['fusion'] is not written) and `completed_meshes` (list of n dicts {vertices, faces,
    vertex_observed}, or None for an empty mesh; None without complete_mesh).  The steps and every other entry of memory are those of
    the wrapped function, bit for bit.  With optimize_codes="tsdf" the codes that vote were fitted to the very state they complete.
    complete_weight HAS NO DEFAULT AND NONE IS RECOMMENDED: unmeasured on real scans and with a trained model."""
    weight = ops._prior_weight("solve_sequence_completed", complete_weight)
    if kw.get("fuse_res") is None:
        raise ValueError("solve_sequence_completed: the completion needs the fused state: give fuse_res")
    if kw.get("fuse_weights") is not None:
        steps, memory = solve_sequence_weighted_fusion(solver, ref, rescans, **kw)
    elif kw.get("view_tol") is not None:
        steps, memory = solve_sequence_view_gated(solver, ref, rescans, **kw)
    else:
        for k in ("fuse_weights", "view_tol"):
            kw.pop(k, None)
        if kw.get("min_view_agreement") is not None:
            raise ValueError("solve_sequence_completed: min_view_agreement needs view_tol: without it no view is compared")
        kw.pop("min_view_agreement", None)
        steps, memory = solve_sequence(solver, ref, rescans, **kw)
    memory["completed"] = solver._complete_fusion_batch(memory["fusion"], memory["codes"], weight=weight)
    memory["completed_meshes"] = solver._completed_mesh_batch(memory["fusion"], memory["completed"]) if complete_mesh else None
    return steps, memory


def _se3_exp(xi):  # host twin of the retraction in csrc/optim.hip (tests compare both with torch.matrix_exp)
    """exp of the twist (v, omega) in R^6 -> [4,4] (Rodrigues + the left Jacobian for the translation)."""
    v, w = xi[:3], xi[3:]
    th = w.norm()
    K = xi.new_zeros(3, 3)
    K[0, 1], K[0, 2], K[1, 0], K[1, 2], K[2, 0], K[2, 1] = -w[2], w[1], w[2], -w[0], -w[1], w[0]
    eye = torch.eye(3, device=xi.device, dtype=xi.dtype)
    if float(th) < 1e-6:
        R, V = eye + K, eye + 0.5 * K
    else:
        a, b, c = torch.sin(th) / th, (1 - torch.cos(th)) / th ** 2, (th - torch.sin(th)) / th ** 3
        R, V = eye + a * K + b * (K @ K), eye + b * K + c * (K @ K)
    out = torch.eye(4, device=xi.device, dtype=xi.dtype)
    out[:3, :3], out[:3, 3] = R, V @ v
    return out

