"""The reference's 3D reconstruction metrics (src/tools/eval_recon.py) without trimesh, open3d or scipy: exact nearest
neighbours on a GPU grid (ops.NNGrid, in place of cKDTree), open3d's point-to-point ICP loop with its correspondence
moments reduced on the GPU (ops.icp_moments) and the 3x3 solve on the host, trimesh's surface sampling
(ops.sample_surface), meshes read as PLY (Mesher.read_ply).

    python -m myslam_amd.src.tools.eval_recon --rec_mesh REC.ply --gt_mesh GT.ply -3d

accuracy / completion / completion_ratio take numpy arrays or torch tensors [N,3] and return a float, as the reference's
(eval_recon.py:21-39).  Deviations: the samples are drawn from a torch generator seeded with `seed` (the reconstructed
mesh's with seed, the ground truth's with seed + 1) instead of numpy's global generator; distances are float32 (the
square root of the float32 squared distance) where cKDTree's are float64.  The 2D depth-L1 metric (eval_recon.py:127+)
is not implemented: it needs a triangle rasteriser.
"""
import argparse

import numpy as np
import torch

from ... import ops
from ..utils.Mesher import read_ply

ICP_THRESHOLD = 0.1          # eval_recon.py:50
ICP_MAX_ROUNDS = 30          # open3d ICPConvergenceCriteria defaults
ICP_RELATIVE_FITNESS = 1e-6
ICP_RELATIVE_RMSE = 1e-6


def _points(p, dev=None):
    t = torch.as_tensor(p)
    if dev is None:
        dev = t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())
    return t.detach().to(dev, torch.float32).reshape(-1, 3)


def _nn_dist(ref, q):
    ref = _points(ref)
    return ops.NNGrid(ref).query(_points(q, ref.device))[0]


def completion_ratio(gt_points, rec_points, dist_th=0.05):
    """Share of ground-truth points within dist_th (strict) of a reconstructed point (eval_recon.py:21-25)."""
    d = _nn_dist(rec_points, gt_points)
    return int((d < dist_th).sum()) / d.numel()


def accuracy(gt_points, rec_points):
    """Mean distance of the reconstructed points to the ground truth (eval_recon.py:28-32)."""
    return float(_nn_dist(gt_points, rec_points).double().mean())


def completion(gt_points, rec_points):
    """Mean distance of the ground-truth points to the reconstruction (eval_recon.py:35-39)."""
    return float(_nn_dist(rec_points, gt_points).double().mean())


def umeyama_from_moments(m):
    """4x4 float64 rigid transform (no scale) taking the source to the target points, least squares over the
    correspondences whose moments m [17] = count, sum d^2, sum s, sum t, sum s t^T (ops.icp_moments) are given:
    H = sum (s - ms)(t - mt)^T = U S V^T, R = V diag(1, 1, det(V U^T)) U^T (reflection corrected), t = mt - R ms.
    Identity without correspondences (open3d's TransformationEstimationPointToPoint)."""
    m = np.asarray(m, dtype=np.float64)
    T = np.eye(4)
    n = m[0]
    if n <= 0:
        return T
    ms, mt = m[2:5] / n, m[5:8] / n
    H = m[8:17].reshape(3, 3) - n * np.outer(ms, mt)
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])
    R = Vt.T @ D @ U.T
    T[:3, :3] = R
    T[:3, 3] = mt - R @ ms
    return T


def _transform(T, v):
    T = torch.as_tensor(T, dtype=torch.float64, device=v.device)
    return v.to(torch.float64) @ T[:3, :3].T + T[:3, 3]


def icp(source, target, threshold=ICP_THRESHOLD, max_rounds=ICP_MAX_ROUNDS, init=None, target_grid=None):
    """Point-to-point ICP of source [N,3] onto target [M,3], open3d's registration_icp loop (eval_recon.py:42-56):
    correspondences = each source point's nearest target point when closer than `threshold`; fitness = |corr| / N,
    inlier_rmse = sqrt(sum d^2 / |corr|) (0 without correspondences); each round solves the rigid transform from the
    correspondences' moments (umeyama_from_moments), T <- dT T, and searches again; it stops after max_rounds rounds or
    when fitness and inlier_rmse both changed by less than 1e-6.  One host sync per round (the 17 moments).
    Returns (T float64 [4,4] numpy, info dict: rounds, fitness, inlier_rmse)."""
    tgt = _points(target)
    dev = tgt.device
    grid = target_grid if target_grid is not None else ops.NNGrid(tgt)
    src0 = torch.as_tensor(source).detach().to(dev, torch.float64).reshape(-1, 3)
    n = src0.shape[0]
    T = np.eye(4) if init is None else np.asarray(init, dtype=np.float64).copy()

    def correspond(T):
        src = _transform(T, src0).float().contiguous()
        dist, idx = grid.query(src, max_dist=threshold)
        m = ops.icp_moments(src, grid.ref, dist, idx, threshold).cpu().numpy()
        cnt = m[0]
        fitness = cnt / n if n else 0.0
        rmse = float(np.sqrt(m[1] / cnt)) if cnt > 0 else 0.0
        return m, fitness, rmse

    m, fitness, rmse = correspond(T)
    rounds = 0
    for _ in range(max_rounds):
        T = umeyama_from_moments(m) @ T
        rounds += 1
        prev_f, prev_r = fitness, rmse
        m, fitness, rmse = correspond(T)
        if abs(prev_f - fitness) < ICP_RELATIVE_FITNESS and abs(prev_r - rmse) < ICP_RELATIVE_RMSE:
            break
    return T, {"rounds": rounds, "fitness": fitness, "inlier_rmse": rmse}


def get_align_transformation(rec_meshfile, gt_meshfile):
    """eval_recon.py:42-56: the 4x4 float64 transform aligning the reconstructed mesh's vertices to the ground truth's
    (ICP from the identity, threshold 0.1)."""
    rec_v, _, _ = read_ply(rec_meshfile)
    gt_v, _, _ = read_ply(gt_meshfile)
    return icp(rec_v, gt_v)[0]


def recon_metrics(rec_v, rec_f, gt_v, gt_f, align=True, num_points=450000, seed=0, device=None):
    """In-memory calc_3d_metric: {'accuracy': cm, 'completion': cm, 'completion_ratio': %} of the two meshes (vertices
    [V,3], faces [F,3]; numpy or torch).  align: the reconstruction is first moved by the ICP transform (float64)."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    rec = torch.as_tensor(rec_v).to(dev, torch.float64).reshape(-1, 3)
    gt = torch.as_tensor(gt_v).to(dev, torch.float64).reshape(-1, 3)
    rec_f, gt_f = torch.as_tensor(rec_f).to(dev), torch.as_tensor(gt_f).to(dev)
    if align:
        rec = _transform(icp(rec, gt)[0], rec)
    rec_pc = ops.sample_surface(rec, rec_f, num_points, seed)[0].float()
    gt_pc = ops.sample_surface(gt, gt_f, num_points, seed + 1)[0].float()
    acc = ops.NNGrid(gt_pc).query(rec_pc)[0]
    comp = ops.NNGrid(rec_pc).query(gt_pc)[0]            # completion and its ratio from one query
    return {"accuracy": float(acc.double().mean()) * 100, "completion": float(comp.double().mean()) * 100,
            "completion_ratio": int((comp < 0.05).sum()) / comp.numel() * 100}


def calc_3d_metric(rec_meshfile, gt_meshfile, align=True, num_points=450000):
    """eval_recon.py:96-120: accuracy (cm), completion (cm) and completion ratio (%, 5 cm) of the reconstructed mesh
    against the ground truth, on num_points surface samples of each; printed as the reference prints them and
    returned as a dict."""
    rec_v, rec_f, _ = read_ply(rec_meshfile)
    gt_v, gt_f, _ = read_ply(gt_meshfile)
    r = recon_metrics(rec_v, rec_f, gt_v, gt_f, align=align, num_points=num_points)
    print('accuracy: ', r["accuracy"])
    print('completion: ', r["completion"])
    print('completion ratio: ', r["completion_ratio"])
    return r


def calc_2d_metric(rec_meshfile, gt_meshfile, align=True, n_imgs=1000):
    raise NotImplementedError("the 2D depth-L1 metric (reference eval_recon.py:127+) needs a mesh rasteriser, "
                              "which this project does not have")


if __name__ == '__main__':
    parser = argparse.ArgumentParser(description='Arguments to evaluate the reconstruction.')
    parser.add_argument('--rec_mesh', type=str, help='reconstructed mesh file path')
    parser.add_argument('--gt_mesh', type=str, help='ground truth mesh file path')
    parser.add_argument('-2d', '--metric_2d', action='store_true', help='enable 2D metric')
    parser.add_argument('-3d', '--metric_3d', action='store_true', help='enable 3D metric')
    args = parser.parse_args()
    if args.metric_3d:
        calc_3d_metric(args.rec_mesh, args.gt_mesh)
    if args.metric_2d:
        calc_2d_metric(args.rec_mesh, args.gt_mesh, n_imgs=1000)
