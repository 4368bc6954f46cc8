"""The build's counterpart of the reference's FlyingShape evaluation loops:
/root/reference/eval_flyingshape.py:62-107 (eval_matching) and :110-173 (eval_relocalization), on synthetic scenes with
the same npz semantics ({'pc': [n_obj,N,3], 'transform': [n_obj,4,4]}; GT = rescan_T @ inv(ref_T), :129; GT match =
identity permutation, :87; symmetry-folded RRE min(r, |180-r|, |90-r|), :140; recalls at 5/10 degrees, :160-168).
All instances of a scene are encoded in ONE batch and all pairs registered in ONE batched call (the reference loops
pair by pair with B=1 encoder calls, :130).  No dataset I/O: the real FlyingShape npz files are not in the tree.
The reconstruction legs (eval_reconstruction, eval_3rscan_reconstruction) score meshes with the device metrics of evaluate.py."""
import numpy as np
import torch

from .lib_math.torch_se3 import concatenate, inverse
from .lib_more.pose_estimation import compute_transformation_error, rotation_error, translation_error


def scene_recall(ratios):
    r = np.asarray(ratios) * 100
    return {f"scene_recall@{t}": float((r >= t).mean() * 100) for t in (25, 50, 75, 100)}


@torch.no_grad()
def eval_matching(scenes, solver, method="sequential", batched=False):
    """scenes: list of dicts from synth.make_scene_pair.  -> metrics dict (eval_flyingshape.py:62-107).  batched=True: the scenes are
    encoded as before, then matched in ONE solver._solve_object_matching_batch call (same metrics)."""
    n_correct = n_total = 0
    ratios = []
    pending = []
    for sc in scenes:
        dev = next(solver.model.parameters()).device
        ref = sc["ref"].to(dev).transpose(1, 2).contiguous()
        res = sc["rescan"].to(dev).transpose(1, 2).contiguous()
        n = ref.shape[0]
        code = solver.model.encode(torch.cat([ref, res], 0))
        cr = {k: v[:n] for k, v in code.items()}
        cs = {k: v[n:] for k, v in code.items()}
        pending.append((cr, cs) if batched else solver._solve_object_matching(cr, cs, method)["matches0"])
    if batched and pending:
        pending = [r["matches0"] for r in solver._solve_object_matching_batch([cr for cr, _ in pending], [cs for _, cs in pending], method)]
    for sc, m in zip(scenes, pending):
        n = sc["ref"].shape[0]
        ok = int((m == torch.arange(n, device=m.device)).sum())
        n_correct += ok
        n_total += n
        ratios.append(ok / n)
    out = {"object_recall": 100.0 * n_correct / max(n_total, 1)}
    out.update(scene_recall(ratios))
    return out


@torch.no_grad()
def eval_relocalization(scenes, solver, icp=True, batched=False, chunk=128):
    """Pairwise registration of every (ref_i, rescan_i) instance pair (eval_flyingshape.py:110-173).  batched=True: the pairs of ALL scenes
    are registered in one ``solver._solve_pairwise_registration_batch`` call per ``chunk`` pairs and scored by ONE
    ``evaluate.registration_metrics_batch`` call with one host read (rre, rte and te in float64); the same dict."""
    rre, rte, te, poses = [], [], [], []
    if batched:
        return _eval_relocalization_batched(scenes, solver, icp, chunk)
    for sc in scenes:
        dev = next(solver.model.parameters()).device
        ref, res = sc["ref"].to(dev), sc["rescan"].to(dev)
        n = ref.shape[0]
        R, t = solver._solve_pairwise_registration_batch([ref[i] for i in range(n)], [res[i] for i in range(n)], icp=icp)
        gt = concatenate(sc["rescan_T"].to(dev)[:, :3], inverse(sc["ref_T"].to(dev)[:, :3]))
        r = rotation_error(R, gt[:, :, :3]).reshape(-1)
        r = torch.minimum(torch.minimum(r, (180 - r).abs()), (90 - r).abs())  # symmetry fold (:140)
        rre.append(r.cpu())
        rte.append(translation_error(t, gt[:, :, 3:4]).reshape(-1).cpu())
        pred = torch.cat([R, t], 2)
        poses.append(pred.cpu())
        te.append(torch.stack([compute_transformation_error(ref[i:i + 1], res[i:i + 1], pred[i:i + 1], gt[i:i + 1]) for i in range(n)]).cpu())
    return _relocalization_summary(torch.cat(rre).numpy(), torch.cat(rte).numpy(), torch.cat(te).numpy(), torch.cat(poses).numpy())


def _relocalization_summary(rre, rte, te, poses):
    def med(x):
        return float(np.median(x)) if len(x) else float("nan")
    return {"recall_rre5": float((rre < 5).mean() * 100), "recall_rre10": float((rre < 10).mean() * 100),
            "median_rre_5": med(rre[rre < 5]), "median_rte_5": med(rte[rre < 5]), "te_cm_5": med(te[rre < 5]) * 100,
            "median_rre_all": med(rre), "rre": rre, "rte": rte, "te": te,
            "poses": poses}   # [n,3,4] predicted (R | t), for parity checks at matrix level


def _register_chunks(register, pcs1, pcs2, chunk):
    """register(pcs1[c0:c1], pcs2[c0:c1]) -> (R, t) per ``chunk`` pairs, concatenated"""
    Rs, ts = [], []
    for c0 in range(0, len(pcs1), max(int(chunk), 1)):
        R, t = register(pcs1[c0:c0 + chunk], pcs2[c0:c0 + chunk])
        Rs.append(R), ts.append(t)
    return torch.cat(Rs, 0), torch.cat(ts, 0)


def _eval_relocalization_batched(scenes, solver, icp, chunk):
    from . import evaluate
    dev = next(solver.model.parameters()).device
    pcs1, pcs2, gts = [], [], []
    for sc in scenes:
        ref, res = sc["ref"].to(dev), sc["rescan"].to(dev)
        pcs1 += [ref[i] for i in range(ref.shape[0])]
        pcs2 += [res[i] for i in range(ref.shape[0])]
        gts.append(concatenate(sc["rescan_T"].to(dev)[:, :3], inverse(sc["ref_T"].to(dev)[:, :3])))
    R, t = _register_chunks(lambda a, b: solver._solve_pairwise_registration_batch(a, b, icp=icp), pcs1, pcs2, chunk)
    pred = torch.cat([R, t], 2)
    m = evaluate.registration_metrics_batch(pcs1, pcs2, pred, torch.cat(gts, 0), chamfer_stride=10)
    host = torch.cat([torch.stack([m["rre"], m["rte"], m["rmse"]], 1), pred.reshape(-1, 12).double()], 1).cpu().numpy()   # the one host read
    r = host[:, 0]
    rre = np.minimum(np.minimum(r, np.abs(180 - r)), np.abs(90 - r))  # symmetry fold (:140)
    return _relocalization_summary(rre, host[:, 1], host[:, 2], host[:, 3:].reshape(-1, 3, 4).astype(np.float32))


# ------------------------------------------------------------------------------------------------ 3RScan matching evaluation
def disambiguate(pred_ids, gt_ids, ambiguity, max_hops=200):
    """/root/reference/eval_3rscan.py:189-228: 3RScan annotates symmetric / interchangeable instances of a scene as groups of
    {'instance_source', 'instance_target', 'transform'} links.  A prediction counts as the ground truth when the ground-truth id
    is reachable from the predicted id by following those links (source -> target, first matching link each hop, until the walk
    returns to its start, dead-ends, or ``max_hops``).  Returns a corrected copy of ``pred_ids``."""
    links = [(p["instance_source"], p["instance_target"]) for group in ambiguity for p in group]
    out = pred_ids.clone()
    for i in range(gt_ids.shape[0]):
        start = int(pred_ids[i])
        chain = [t for s, t in links if s == start]
        hops = 0
        while chain and hops < max_hops:
            nxt = next((t for s, t in links if s == chain[-1]), None)
            if nxt is None or nxt == start:
                break
            chain.append(nxt)
            hops += 1
        if int(gt_ids[i]) in chain:
            out[i] = gt_ids[i]
    return out


@torch.no_grad()
def eval_3rscan_matching(dataset, solver, method_list=("sequential",), batched=False):
    """Object matching between the reference scan and every rescan of each scene of a ``rscan.Dataset_3RScan``
    (eval_3rscan.py:232-335): object-level recall over the instances present in both scans (all / static / dynamic, the split
    coming from the rescan's rigid annotations), and scene-level recall = share of (scene, rescan) pairs whose hit ratio reaches
    75 / 50 / 25 %.  Codes come from ``model.encode_fps`` on the padded clouds, matches from ``solver._solve_object_matching``.
    batched=True: the codes of every (scene, rescan) are collected first, then each method matches all of them in ONE
    ``solver._solve_object_matching_batch`` call (same metrics)."""
    model = solver.model
    n_methods = len(method_list)
    n_total = 0
    n_correct = np.zeros(n_methods)
    scene_total = np.zeros(3)
    scene_count = np.zeros(3)      # hits @75, @50, @25
    tot_dyn = cor_dyn = tot_sta = cor_sta = 0

    def score(scene, ref_ids, rescan, m0s):    # m0s: the matches0 of every method for this (scene, rescan)
        nonlocal n_total, scene_total, tot_dyn, cor_dyn, tot_sta, cor_sta
        res_ids = rescan["objectId"]
        moving = set(int(v) for v in rescan["moving_ids"].tolist())
        valid = torch.tensor([int(i) in set(res_ids.tolist()) for i in ref_ids.tolist()], device=ref_ids.device)
        moving_mask = torch.tensor([int(i) in moving for i in ref_ids.tolist()], device=ref_ids.device)
        for mi, method in enumerate(method_list):
            m0 = m0s[mi].to(ref_ids.device)
            matched = res_ids[m0.clamp(min=0)]
            if len(scene.get("ambiguity", [])) != 0:
                matched = disambiguate(matched.view(-1), ref_ids, scene["ambiguity"])
            matched = torch.where(m0 != -1, matched, torch.full_like(matched, -1))
            hit = matched == ref_ids
            n_match = int(valid.sum())
            ok = int(hit[valid].sum())
            n_correct[mi] += ok
            n_total += n_match
            scene_total += 1
            ratio = ok / n_match if n_match else 0.0
            if ratio >= 0.75:
                scene_count[:] += 1
            elif ratio >= 0.5:
                scene_count[1:] += 1
            elif ratio >= 0.25:
                scene_count[2:] += 1
            tot_dyn += int((valid & moving_mask).sum()); cor_dyn += int(hit[valid & moving_mask].sum())
            tot_sta += int((valid & ~moving_mask).sum()); cor_sta += int(hit[valid & ~moving_mask].sum())

    pending = []   # batched: (scene, ref ids, rescan, ref codes, rescan codes) of every (scene, rescan)
    for i_s, scene in enumerate(dataset.scene_list):
        ref, rescans = dataset._get_scene(i_s)
        if ref is None or len(rescans) == 0:
            continue
        ref_codes = model.encode_fps(ref["pc"], ref["pc_mask"])
        ref_ids = ref["objectId"]
        for rescan in rescans:
            codes = model.encode_fps(rescan["pc"], rescan["pc_mask"])
            if batched:
                pending.append((scene, ref_ids, rescan, ref_codes, codes))
            else:
                score(scene, ref_ids, rescan, [solver._solve_object_matching(ref_codes, codes, method)["matches0"] for method in method_list])
    if pending:
        per_method = [solver._solve_object_matching_batch([r[3] for r in pending], [r[4] for r in pending], method) for method in method_list]
        for k, (scene, ref_ids, rescan, _, _) in enumerate(pending):
            score(scene, ref_ids, rescan, [res[k]["matches0"] for res in per_method])
    per_method_total = n_total / max(n_methods, 1)
    pct = lambda a, b: 100.0 * a / b if b else float("nan")
    out = {f"object_recall[{m}]": pct(n_correct[i], per_method_total) for i, m in enumerate(method_list)}
    out.update({"static_recall": pct(cor_sta, tot_sta), "dynamic_recall": pct(cor_dyn, tot_dyn)})
    out.update({f"scene_recall@{t}": pct(scene_count[i], scene_total[i]) for i, t in enumerate((75, 50, 25))})
    return out


@torch.no_grad()
def eval_3rscan_relocalization(dataset, solver, optim=True, batched=False, chunk=128):
    """Instance re-localisation over a ``rscan.Dataset_3RScan`` (eval_3rscan.py:337-456): for every annotated rigid instance that
    is present in both the reference scan and the rescan, register its reference cloud to its rescan cloud
    (``solver._solve_pairwise_registration``; the rescan is first moved back into its own frame with the inverse scene
    transform), then relative rotation error (folded by the annotation's symmetry class: 1 -> min(r, |180-r|), 2 -> also
    |90-r|), relative translation error, end-point RMSE and the chamfer distance of every tenth point.  Reported as the
    reference does: recall at RMSE < 0.1 m with the medians over RMSE < 0.2 m, recall at RRE < 10 deg with the medians over it,
    median chamfer distance.
    batched=True: every valid (scene, rescan, rigid) pair is collected first (same validity rule, same inverse scene transform, same
    order), the pairs are registered ``chunk`` at a time in lock-step (``solver._solve_pairwise_registration_optim_batch`` when
    ``optim``, else ``solver._solve_pairwise_registration_batch``), and all of them are scored by ONE
    ``evaluate.registration_metrics_batch`` call with ONE host read; the symmetry fold and the summary are the host's.  Same keys."""
    from . import evaluate
    from .evaluate import chamfer_distance_torch
    from .lib_math import torch_se3
    rre_l, rte_l, err_l, cd_l, shape_l = [], [], [], [], []
    pend1, pend2, pend_gt, pend_sym = [], [], [], []
    for i_s, scene in enumerate(dataset.scene_list):
        ref, rescans = dataset._get_scene(i_s)
        if ref is None:
            continue
        dev = ref["pc"].device
        for rescan, sg in zip(rescans, [s for s in scene["scans"]]):
            scene_tsfm = rescan["rescan2ref_tsfm"]
            pc = torch_se3.transform(torch_se3.inverse(scene_tsfm), rescan["pc"].transpose(-1, -2)).transpose(-1, -2)
            ref_ids, res_ids = ref["objectId"].tolist(), rescan["objectId"].tolist()
            for rigid in sg["rigid"]:
                if rigid["instance_reference"] not in ref_ids or rigid.get("instance_rescan", rigid["instance_reference"]) not in res_ids:
                    continue
                gt = torch.tensor(rigid["transform"], dtype=torch.float32, device=dev).reshape(1, 4, 4).transpose(-1, -2).contiguous()
                a = ref_ids.index(rigid["instance_reference"])
                b = res_ids.index(rigid.get("instance_rescan", rigid["instance_reference"]))
                inst_ref = ref["pc"][a].T[ref["pc_mask"][a, 0]].unsqueeze(0).contiguous()
                inst_res = pc[b].T[rescan["pc_mask"][b, 0]].unsqueeze(0).contiguous()
                if batched:
                    pend1.append(inst_ref[0]), pend2.append(inst_res[0]), pend_gt.append(gt[0, :3]), pend_sym.append(rigid.get("symmetry", 0))
                    shape_l.append(ref["id_label"][[l[0] for l in ref["id_label"]].index(rigid["instance_reference"])][-1])
                    continue
                with torch.enable_grad():
                    R, t = solver._solve_pairwise_registration(inst_ref, inst_res, optim=optim)
                rre = float(rotation_error(R, gt[:, :3, :3]))
                sym = rigid.get("symmetry", 0)
                if sym == 1:
                    rre = min(rre, abs(180 - rre))
                elif sym == 2:
                    rre = min(rre, abs(180 - rre), abs(90 - rre))
                pred = torch_se3.Rt_to_SE3(R, t)
                rre_l.append(rre)
                rte_l.append(float(translation_error(t, gt[:, :3, 3:4])))
                err_l.append(float(compute_transformation_error(inst_ref, inst_res, pred, gt)))
                cd_l.append(float(chamfer_distance_torch(inst_ref[:, ::10].contiguous(), inst_res[:, ::10].contiguous(), pred, gt)))
                shape_l.append(ref["id_label"][[l[0] for l in ref["id_label"]].index(rigid["instance_reference"])][-1])
    if pend1:
        register = solver._solve_pairwise_registration_optim_batch if optim else solver._solve_pairwise_registration_batch
        with torch.enable_grad():
            R, t = _register_chunks(register, pend1, pend2, chunk)
        m = evaluate.registration_metrics_batch(pend1, pend2, torch.cat([R, t], 2), torch.stack(pend_gt), chamfer_stride=10)
        host = torch.stack([m["rre"], m["rte"], m["rmse"], m["chamfer"]], 1).cpu().numpy()   # the one host read
        for (r, te, err, cd), sym in zip(host.tolist(), pend_sym):
            if sym == 1:
                r = min(r, abs(180 - r))
            elif sym == 2:
                r = min(r, abs(180 - r), abs(90 - r))
            rre_l.append(r), rte_l.append(te), err_l.append(err), cd_l.append(cd)
    rre, rte, err, cd = (np.asarray(v, dtype=np.float64) for v in (rre_l, rte_l, err_l, cd_l))
    med = lambda v, m: float(np.median(v[m])) if m.any() else float("nan")
    return {"n_pairs": int(len(rre)),
            "recall[T<0.1m]": float(100 * (err < 0.1).mean()) if len(err) else float("nan"),
            "rre_median[T<0.2m]": med(rre, err < 0.2), "rte_median[T<0.2m]": med(rte, err < 0.2),
            "recall[RRE<10deg]": float(100 * (rre < 10).mean()) if len(rre) else float("nan"),
            "rre_median[RRE<10deg]": med(rre, rre < 10), "rte_median[RRE<10deg]": med(rte, rre < 10),
            "chamfer_median": float(np.median(cd)) if len(cd) else float("nan"), "shape": shape_l}


# ------------------------------------------------------------------------------------------------ reconstruction evaluation
def _recon_summary(cd, recall, iou=None):
    cd, recall = np.asarray(cd, np.float64), np.asarray(recall, np.float64)
    out = {"chamfer_mean": float(cd.mean()) if len(cd) else float("nan"),
           "sdf_recall@0.7": float((recall > 0.7).mean() * 100) if len(recall) else float("nan")}
    if iou is not None:
        iou = np.asarray(iou, np.float64)
        out.update({"viou_recall@0.5": float((iou > 0.5).mean() * 100) if len(iou) else float("nan"),
                    "viou_mean": float(iou.mean() * 100) if len(iou) else float("nan"),
                    "viou_median": float(np.median(iou) * 100) if len(iou) else float("nan")})
    return out


def _scored(preds):
    """indices of the non-empty predicted meshes (an empty one is not scored)"""
    return [i for i, m in enumerate(preds) if m.vertices.shape[0] != 0]


@torch.no_grad()
def eval_reconstruction(scenes, solver, gt_meshes, batched=False):
    """eval_flyingshape.py:176-213: every instance of every scene is encoded (one batch per scene), meshed from its code
    (``solver._mesh_from_latent``), moved back into its canonical frame by the inverse of the instance pose, and scored against its
    ground-truth mesh ``gt_meshes[scene][instance]``: cd1 + cd2 (compute_chamfer_distance), SDF recall at 0.05 of the GT vertices
    (compute_sdf_recall), V-IoU (compute_volumetric_iou).  An empty predicted mesh scores recall 0 and V-IoU 0 and has no Chamfer entry.
    ``scenes``: dicts with 'pc' [n,N,3] and 'transform' [n,4,4] (the reference's npz keys) or synth.make_scene_pair's 'ref' / 'ref_T'.
    -> {'chamfer_mean', 'sdf_recall@0.7', 'viou_recall@0.5', 'viou_mean', 'viou_median' (percent, as logged), 'cd', 'sdf_recall', 'viou',
    'n_objects', 'n_empty'}.  batched=True: all objects of a scene are meshed together (``solver._mesh_from_latent_batch``) and scored
    with one call per metric (evaluate's *_batch functions) -- the same numbers."""
    from .evaluate import compute_chamfer_distance, compute_sdf_recall, compute_volumetric_iou
    from .mesh_extractor2 import make_mesh
    dev = next(solver.model.parameters()).device
    cd_l, rec_l, iou_l, n_obj, n_empty = [], [], [], 0, 0
    for sc, gts in zip(scenes, gt_meshes):
        pc = torch.as_tensor(sc["pc"] if "pc" in sc else sc["ref"]).to(dev).float().transpose(-1, -2).contiguous()
        pose = torch.as_tensor(sc["transform"] if "transform" in sc else sc["ref_T"]).double()
        codes = solver.model.encode(pc)
        if batched:
            preds = solver._mesh_from_latent_batch({k: codes[k].detach() for k in ("z_inv", "z_so3", "s", "t")})
            invs = [inverse(pose[i][None])[0].numpy() for i in range(len(preds))]       # [3,4] each, as the per-object leg
            preds = [make_mesh(np.asarray(p.vertices, np.float64) @ inv[:, :3].T + inv[:, 3], p.faces) for p, inv in zip(preds, invs)]
            cd, rec, iou = _score_batch(preds, gts, with_iou=True)
            n_obj += len(preds)
            n_empty += len(preds) - len(cd)
            cd_l += [a + b for a, b in cd]
            rec_l += rec
            iou_l += iou
            continue
        for i in range(pc.shape[0]):
            code = {k: codes[k][i][None].detach() for k in ("z_inv", "z_so3", "s", "t")}
            pred = solver._mesh_from_latent(code)
            inv = inverse(pose[i][None])[0].numpy()                                  # [3,4]
            pred = make_mesh(np.asarray(pred.vertices, np.float64) @ inv[:, :3].T + inv[:, 3], pred.faces)
            n_obj += 1
            if pred.vertices.shape[0] != 0:
                cd1, cd2 = compute_chamfer_distance(gts[i], pred, offset=0, scale=1)
                cd_l.append(cd1 + cd2)
                rec_l.append(compute_sdf_recall(pred, gts[i], 0.05))
                iou_l.append(compute_volumetric_iou(pred, gts[i]))
            else:
                n_empty += 1
                rec_l.append(0.0)
                iou_l.append(0.0)
    out = _recon_summary(cd_l, rec_l, iou_l)
    out.update({"cd": cd_l, "sdf_recall": rec_l, "viou": iou_l, "n_objects": n_obj, "n_empty": n_empty})
    return out


def _score_batch(preds, gts, with_iou):
    """the per-object scores of the reconstruction legs for one scene, one device call per metric: -> ([(cd1, cd2)] of the non-empty
    meshes, recall per object, V-IoU per object or None); an empty mesh scores recall 0 and V-IoU 0"""
    from .evaluate import compute_chamfer_distance_batch, compute_sdf_recall_batch, compute_volumetric_iou_batch
    live = _scored(preds)
    P, G = [preds[i] for i in live], [gts[i] for i in live]
    cd = compute_chamfer_distance_batch(G, P, offset=0, scale=1)
    rec, iou = [0.0] * len(preds), [0.0] * len(preds)
    for i, r in zip(live, compute_sdf_recall_batch(P, G, 0.05)):
        rec[i] = r
    if not with_iou:
        return cd, rec, None
    for i, v in zip(live, compute_volumetric_iou_batch(P, G)):
        iou[i] = v
    return cd, rec, iou


def eval_3rscan_reconstruction(dataset, solver, optim=True, batched=False):
    """eval_3rscan.py:466-502 over a ``rscan.Dataset_3RScan``: every kept instance of every reference scan is encoded from its padded
    cloud (``model.encode_fps``), its code refined against the cloud (``solver._optimize_code``, when ``optim``; a code whose loss never
    improved stays as encoded), meshed (``solver._mesh_from_latent``) and scored against ``<root>/val_set_recon/<ref_id>/objectId_<k>.ply``:
    one-way Chamfer cd1 = compute_chamfer_distance(gt, pred, 0, 1)[0] and SDF recall = compute_sdf_recall(pred, gt, 0.05).  An empty
    predicted mesh scores recall 0 and has no Chamfer entry.  -> {'chamfer_1way_mean', 'sdf_recall@0.7' (percent): the two numbers the
    reference logs, 'cd', 'sdf_recall' (per object), 'n_objects', 'n_empty'}.  batched=True: the instances of a scene are encoded in one
    batch, refined together (``solver._optimize_code_batch``, which agrees with the per-instance refinement to ~1e-5), meshed together
    (``solver._mesh_from_latent_batch``) and scored with one call per metric."""
    import os.path as osp
    from .evaluate import compute_chamfer_distance, compute_sdf_recall
    from .mesh_extractor2 import make_mesh
    from .rscan import load_ply_mesh
    recon_gt = osp.join(dataset.root_path, "val_set_recon")
    cd_l, rec_l, n_obj, n_empty = [], [], 0, 0
    for i_s, scene in enumerate(dataset.scene_list):
        ref_id = scene["reference"]
        ref, _ = dataset._get_scene(i_s)
        if ref is None:
            continue
        if batched:
            n = ref["pc"].shape[0]
            gts = [make_mesh(*load_ply_mesh(osp.join(recon_gt, ref_id, f"objectId_{int(ref['objectId'][i])}.ply"))) for i in range(n)]
            with torch.no_grad():
                codes = solver.model.encode_fps(ref["pc"], ref["pc_mask"])
            if optim:
                # the final values are written back into `codes` whether or not an instance improved -- as _optimize_code does for the
                # per-object leg, where `codes` is meshed when the loss never improved
                solver._optimize_code_batch(codes, [ref["pc"][i].T[ref["pc_mask"][i].reshape(-1).bool()] for i in range(n)])
            preds = solver._mesh_from_latent_batch(codes)
            cd, rec, _ = _score_batch(preds, gts, with_iou=False)
            n_obj += n
            n_empty += n - len(cd)
            cd_l += [a for a, _ in cd]
            rec_l += rec
            continue
        for i in range(ref["pc"].shape[0]):
            oid = int(ref["objectId"][i])
            gt = make_mesh(*load_ply_mesh(osp.join(recon_gt, ref_id, f"objectId_{oid}.ply")))
            with torch.no_grad():
                codes = solver.model.encode_fps(ref["pc"][i][None], ref["pc_mask"][i][None])
            if optim:
                refined = solver._optimize_code(codes, ref["pc"][i], ref["pc_mask"][i])
                codes = refined if refined is not None else codes
            pred = solver._mesh_from_latent(codes)
            n_obj += 1
            if pred.vertices.shape[0] != 0:
                cd1, _ = compute_chamfer_distance(gt, pred, offset=0, scale=1)
                cd_l.append(cd1)
                rec_l.append(compute_sdf_recall(pred, gt, 0.05))
            else:
                n_empty += 1
                rec_l.append(0.0)
    s = _recon_summary(cd_l, rec_l)
    return {"chamfer_1way_mean": s["chamfer_mean"], "sdf_recall@0.7": s["sdf_recall@0.7"], "cd": cd_l, "sdf_recall": rec_l,
            "n_objects": n_obj, "n_empty": n_empty}
