"""The reference's reconstruction metrics (src/tools/eval_recon.py) without trimesh, open3d, scipy or a GL context:
exact nearest neighbours on a GPU grid (ops.NNGrid, in place of cKDTree), open3d's point-to-point ICP loop with its
correspondence moments reduced on the GPU (ops.icp_moments) and the 3x3 solve on the host, trimesh's surface sampling
(ops.sample_surface), meshes read as PLY (Mesher.read_ply), and for the 2D metric a depth rasteriser
(ops.render_mesh_depth, in place of open3d's visualiser), the per-view |difference| sums (ops.depth_l1) and the
unseen-points test of a batch of candidate views (ops.views_see_points).

    python -m myslam_amd.src.tools.eval_recon --rec_mesh REC.ply --gt_mesh GT.ply -2d -3d
    python -m myslam_amd.src.tools.eval_recon --rec_mesh REC.ply --gt_mesh GT.ply --report --exact --error_mesh OUT

accuracy / completion / completion_ratio take numpy arrays or torch tensors [N,3] and return a float, as the reference's
(eval_recon.py:21-39).  Deviations, 3D: the samples are drawn from a torch generator seeded with `seed` (the reconstructed
mesh's with seed, the ground truth's with seed + 1) instead of numpy's global generator; distances are float32 (the
square root of the float32 squared distance) where cKDTree's are float64.  Deviations, 2D: the
views come from a seeded numpy Generator instead of `random` and numpy's global state; the camera box is the smallest
of a fixed candidate set of orientations (get_cam_position) where trimesh searches the convex hull; the near plane is
the constant Z_NEAR where open3d derives one from the scene's bounding box.
"""
import argparse

import numpy as np
import torch

from ... import ops
from ..utils.Mesher import read_ply, write_ply

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


# ----------------------------------------------------------------------------------------------
# beyond the reference: F-score, normal consistency, exact point-to-mesh distances, error maps
# ----------------------------------------------------------------------------------------------
def f_score(d_rec_to_gt, d_gt_to_rec, threshold):
    """(precision, recall, f) as fractions, from the distances of the reconstruction's points to the ground truth and of
    the ground truth's points to the reconstruction (tensors or arrays on any device): precision = the share of the
    first below `threshold` (strict, as completion_ratio), recall the share of the second, f = 2 p r / (p + r), 0 when
    both are 0.  An empty side has share 0."""
    def share(d):
        d = torch.as_tensor(d).reshape(-1)
        return int((d < threshold).sum()) / d.numel() if d.numel() else 0.0
    p, r = share(d_rec_to_gt), share(d_gt_to_rec)
    return p, r, (2.0 * p * r / (p + r) if p + r > 0 else 0.0)


def normal_consistency(n_a, n_b):
    """(mean |n_a . n_b| over the rows where both normals have a non-zero, finite length, each normalised in float64;
    the number of rows used).  Rows left out are those with a zero or non-finite normal on either side: total - used.
    No row used: (nan, 0).  Tensors or arrays [N,3] on any device."""
    a = torch.as_tensor(n_a).to(torch.float64).reshape(-1, 3)
    b = torch.as_tensor(n_b).to(a.device, torch.float64).reshape(-1, 3)
    la, lb = a.norm(dim=1), b.norm(dim=1)
    use = (la > 0) & (lb > 0) & torch.isfinite(la) & torch.isfinite(lb)
    used = int(use.sum())
    if used == 0:
        return float("nan"), 0
    dots = ((a[use] / la[use, None]) * (b[use] / lb[use, None])).sum(dim=1).abs()
    return float(dots.mean()), used


def face_normals(verts, faces):
    """float64 [F,3] on verts' device: the unit normal (b - a) x (c - a) / |.| of every face, a zero row for a face of
    zero (or non-finite) area."""
    v = torch.as_tensor(verts).to(torch.float64).reshape(-1, 3)
    f = torch.as_tensor(faces).to(v.device, torch.int64).reshape(-1, 3)
    n = torch.linalg.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    ln = n.norm(dim=1, keepdim=True)
    ok = (ln > 0) & torch.isfinite(ln)
    return torch.where(ok, n / torch.where(ok, ln, torch.ones_like(ln)), torch.zeros_like(n))


def error_colors(dist, max_err, lut=None):
    """uint8 [N,3] on dist's device: lut[floor(min(d / max_err, 1) * 255 + 0.5)] in float64, index 255 for an infinite
    or NaN distance; lut = the committed plasma table (ops.load_plasma_lut) unless given."""
    d = torch.as_tensor(dist).to(torch.float64).reshape(-1)
    if lut is None:
        lut = torch.from_numpy(ops.load_plasma_lut())
    lut = torch.as_tensor(lut).to(d.device)
    idx = torch.floor(torch.clamp(d / float(max_err), max=1.0) * 255.0 + 0.5)
    idx = torch.where(torch.isfinite(d), idx, torch.full_like(idx, 255.0)).to(torch.int64)
    return lut[idx]


def _report_inputs(rec_v, rec_f, gt_v, gt_f, align, device):
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    rec = torch.as_tensor(rec_v).to(dev, torch.float64).reshape(-1, 3)
    gt = torch.as_tensor(gt_v).to(dev, torch.float64).reshape(-1, 3)
    rec_f, gt_f = torch.as_tensor(rec_f).to(dev), torch.as_tensor(gt_f).to(dev)
    if align:
        rec = _transform(icp(rec, gt)[0], rec)
    return rec, rec_f, gt, gt_f


def recon_report(rec_v, rec_f, gt_v, gt_f, align=True, num_points=450000, seed=0, exact=False, f_threshold=0.05, device=None):
    """recon_metrics' three numbers and the metrics the reference lacks, from the same samples: {'accuracy',
    'completion' (cm), 'completion_ratio' (%, 5 cm), 'chamfer' (cm, their mean), 'precision', 'recall', 'f_score' (%, at
    f_threshold), 'normal_consistency' (mean |n . n'| of a sample's face normal and the other side's, both directions
    averaged), 'normals_skipped' (rows without a normal on either side, both directions), 'exact'}.
    exact=False: every sample is measured to the nearest SAMPLE of the other mesh (ops.NNGrid), as recon_metrics does -
    the first three keys are recon_metrics' floats - and the other side's normal is that sample's face's.
    exact=True: every sample is measured to the other MESH (ops.MeshDistance, float32 vertices) and the normal is the
    returned face's: no sampling bias on the far side."""
    rec, rec_f, gt, gt_f = _report_inputs(rec_v, rec_f, gt_v, gt_f, align, device)
    rec_s, rec_fi = ops.sample_surface(rec, rec_f, num_points, seed)
    gt_s, gt_fi = ops.sample_surface(gt, gt_f, num_points, seed + 1)
    rec_pc, gt_pc = rec_s.float(), gt_s.float()
    rec_n, gt_n = face_normals(rec, rec_f), face_normals(gt, gt_f)
    if exact:
        acc, acc_face = ops.MeshDistance(gt.float(), gt_f).query(rec_pc)
        comp, comp_face = ops.MeshDistance(rec.float(), rec_f).query(gt_pc)
    else:
        acc, idx = ops.NNGrid(gt_pc).query(rec_pc)
        acc_face = torch.where(idx >= 0, gt_fi[idx.long().clamp(min=0)], torch.full_like(gt_fi[:1], -1))
        comp, idx = ops.NNGrid(rec_pc).query(gt_pc)
        comp_face = torch.where(idx >= 0, rec_fi[idx.long().clamp(min=0)], torch.full_like(rec_fi[:1], -1))

    def other(normals, face):          # the other side's normal, a zero row where no face was found
        face = face.long()
        return torch.where((face >= 0)[:, None], normals[face.clamp(min=0)], torch.zeros_like(normals[:1]))

    nc_a, used_a = normal_consistency(rec_n[rec_fi], other(gt_n, acc_face))
    nc_c, used_c = normal_consistency(gt_n[gt_fi], other(rec_n, comp_face))
    p, r, f = f_score(acc, comp, f_threshold)
    accuracy_cm, completion_cm = float(acc.double().mean()) * 100, float(comp.double().mean()) * 100
    return {"accuracy": accuracy_cm, "completion": completion_cm,
            "completion_ratio": int((comp < 0.05).sum()) / comp.numel() * 100,
            "chamfer": 0.5 * (accuracy_cm + completion_cm), "precision": p * 100, "recall": r * 100, "f_score": f * 100,
            "normal_consistency": 0.5 * (nc_a + nc_c), "normals_skipped": (acc.numel() - used_a) + (comp.numel() - used_c),
            "exact": bool(exact)}


def error_meshes(rec_v, rec_f, gt_v, gt_f, max_err=0.05, align=True, device=None):
    """Per-vertex error maps: the exact distance (ops.MeshDistance) of every vertex of the (aligned) reconstruction to
    the ground-truth mesh and of every ground-truth vertex to the reconstruction, coloured by error_colors(d, max_err).
    Returns {'rec_colors', 'gt_colors' (uint8 [V,3]), 'rec_dist', 'gt_dist' (float32 [V], metres), 'rec_vertices'
    (float64 [V,3], after the alignment)}, tensors on the GPU."""
    rec, rec_f, gt, gt_f = _report_inputs(rec_v, rec_f, gt_v, gt_f, align, device)
    rec_d = ops.MeshDistance(gt.float(), gt_f).query(rec.float())[0]
    gt_d = ops.MeshDistance(rec.float(), rec_f).query(gt.float())[0]
    return {"rec_colors": error_colors(rec_d, max_err), "gt_colors": error_colors(gt_d, max_err), "rec_dist": rec_d,
            "gt_dist": gt_d, "rec_vertices": rec}


def write_error_meshes(rec_meshfile, gt_meshfile, prefix, max_err=0.05, align=True):
    """PREFIX_accuracy.ply: the (aligned) reconstruction coloured by its distance to the ground truth; PREFIX_completion.ply:
    the ground truth coloured by its distance to the reconstruction (plasma, 0 .. max_err metres).  Returns the paths."""
    rec_v, rec_f, _ = read_ply(rec_meshfile)
    gt_v, gt_f, _ = read_ply(gt_meshfile)
    e = error_meshes(rec_v, rec_f, gt_v, gt_f, max_err=max_err, align=align)
    paths = (prefix + "_accuracy.ply", prefix + "_completion.ply")
    write_ply(paths[0], e["rec_vertices"].cpu().numpy(), rec_f, colors=e["rec_colors"].cpu().numpy() / 255.0)
    write_ply(paths[1], gt_v, gt_f, colors=e["gt_colors"].cpu().numpy() / 255.0)
    return paths


def print_report(rec_meshfile, gt_meshfile, exact=False, f_threshold=0.05, align=True, num_points=450000):
    """recon_report of two mesh files, one `name: value` line per key."""
    rec_v, rec_f, _ = read_ply(rec_meshfile)
    gt_v, gt_f, _ = read_ply(gt_meshfile)
    r = recon_report(rec_v, rec_f, gt_v, gt_f, align=align, num_points=num_points, exact=exact, f_threshold=f_threshold)
    for k, v in r.items():
        print(f"{k}: {v}")
    return r


# ----------------------------------------------------------------------------------------------
# the 2D metric: depth L1 over random views inside the room (eval_recon.py:59-85, 116-207)
# ----------------------------------------------------------------------------------------------
IMG_H = IMG_W = 500          # eval_recon.py:132-138
FOCAL = 300.0
IMG_CX = IMG_H / 2.0 - 0.5
IMG_CY = IMG_W / 2.0 - 0.5
Z_NEAR = ops._hip.RASTER_Z_NEAR      # ours (open3d derives its near plane from the bounding box)
Z_FAR = ops._hip.RASTER_Z_FAR        # ctr.set_constant_z_far(20)
BOX_ANGLES = 90              # get_cam_position: candidate rotations of 1 degree about each axis of each base frame
VIEW_BATCH = 64              # sample_views: candidates drawn and tested per call


def viewmatrix(z, up, pos):
    """eval_recon.py:13-19: the 3x4 camera-to-world matrix [right | down | forward | pos] of a camera at pos looking
    along z: forward = z / |z|, right = up x forward normalised, down = forward x right normalised."""
    forward = np.asarray(z, dtype=np.float64) / np.linalg.norm(z)
    right = np.cross(np.asarray(up, dtype=np.float64), forward)
    right = right / np.linalg.norm(right)
    down = np.cross(forward, right)
    down = down / np.linalg.norm(down)
    return np.stack([right, down, forward, np.asarray(pos, dtype=np.float64)], axis=1)


def check_proj(points, W, H, fx, fy, cx, cy, c2w):
    """eval_recon.py:59-85 on the host, step by step in the reference's precisions: True when a point of points [N,3]
    projects into the view.  The float64 c2w has its columns 1 and 2 negated and is inverted; then in float32
    c = w2c [p, 1], c.x *= -1, (a, b, zz) = K c, z = zz + 1e-5, (u, v) = (a, b) / z; in view when 0 <= -z, 0 < u < W,
    0 < v < H.  ops.views_see_points is the same test for a batch of views on the GPU."""
    c2w = np.array(c2w, dtype=np.float64)
    c2w[:3, 1] *= -1.0
    c2w[:3, 2] *= -1.0
    w2c = np.linalg.inv(c2w).astype(np.float32)
    pts = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    homo = np.concatenate([pts, np.ones_like(pts[:, :1])], axis=1).reshape(-1, 4, 1)
    cam = (w2c @ homo)[:, :3]
    cam[:, 0] *= -1
    Km = np.array([[fx, .0, cx], [.0, fy, cy], [.0, .0, 1.0]], dtype=np.float32)
    uv = Km @ cam
    z = uv[:, -1:] + np.float32(1e-5)
    uv = (uv[:, :2] / z)[:, :, 0]
    mask = (0 <= -z[:, 0, 0]) & (uv[:, 0] < W) & (uv[:, 0] > 0) & (uv[:, 1] < H) & (uv[:, 1] > 0)
    return bool(mask.sum() > 0)


def _rot_about(axis, deg):
    a = np.radians(deg)
    k = np.asarray(axis, dtype=np.float64)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx


def box_candidates(cov):
    """The candidate orientations of get_cam_position, float64 [2 * 3 * BOX_ANGLES, 3, 3] (rows = box axes): for each
    of the two base frames - the world axes, and the eigenvectors of the vertices' 3x3 covariance `cov` (numpy eigh,
    ascending eigenvalues) - and each of its three axes, the frame turned about that axis by 0, 1, ..., BOX_ANGLES - 1
    degrees."""
    frames = [np.eye(3), np.linalg.eigh(np.asarray(cov, dtype=np.float64))[1].T]
    out = []
    for B in frames:
        for a in range(3):
            for deg in range(BOX_ANGLES):
                out.append(B @ _rot_about(B[a], deg).T)
    return np.stack(out)


def get_cam_position(gt_meshfile_or_vertices):
    """eval_recon.py:116-124: (extents [3], transform [4,4]) of the box views are sampled in: an oriented bounding box of
    the ground-truth vertices with its axes ordered by ascending extent (trimesh.bounds.oriented_bounds, ordered=True),
    extents scaled by (0.3, 0.7, 0.7), transform = box-to-world (rotation | centre) with 0.4 added to transform[2, 3].
    Deviation: trimesh searches the convex hull for the minimum-volume box; here the box is the smallest-volume one of
    box_candidates(), each evaluated in float64 on the vertices' device (the GPU when there is one) as the min / max of
    the vertices' projections on its axes; the first of equal volumes wins.  One host sync."""
    if isinstance(gt_meshfile_or_vertices, str):
        v = torch.from_numpy(np.ascontiguousarray(read_ply(gt_meshfile_or_vertices)[0]))
    else:
        v = torch.as_tensor(gt_meshfile_or_vertices)
    if not v.is_cuda and torch.cuda.is_available():
        v = v.to(torch.device("cuda", torch.cuda.current_device()))
    v = v.detach().to(torch.float64).reshape(-1, 3)
    if v.shape[0] < 1:
        raise RuntimeError("get_cam_position: no vertices")
    mean = v.mean(0)
    cov = ((v - mean).T @ (v - mean) / v.shape[0]).cpu().numpy()
    cand = box_candidates(cov)
    R = torch.from_numpy(cand).to(v.device)
    lo = torch.empty(len(cand), 3, dtype=torch.float64, device=v.device)
    hi = torch.empty_like(lo)
    for k in range(len(cand)):
        lo[k], hi[k] = (v @ R[k].T).aminmax(dim=0)
    ext = hi - lo
    best = int(torch.argmin(ext.prod(dim=1)))            # (argmin returns the first minimum)
    ext, lo_b = ext[best].cpu().numpy(), lo[best].cpu().numpy()
    order = np.argsort(ext, kind="stable")
    axes = cand[best][order]
    if np.linalg.det(axes) < 0:
        axes[2] *= -1.0
    centre = (lo_b + 0.5 * ext) @ cand[best]
    extents = ext[order].copy()
    transform = np.eye(4)
    transform[:3, :3] = axes.T
    transform[:3, 3] = centre
    extents[2] *= 0.7
    extents[1] *= 0.7
    extents[0] *= 0.3
    transform[2, 3] += 0.4
    return extents, transform


def sample_views(extents, transform, n, pc_unseen=None, seed=0, K=(FOCAL, FOCAL, IMG_CX, IMG_CY), H=IMG_H, W=IMG_W):
    """eval_recon.py:156-175: n camera-to-world matrices, float64 [n,4,4]; per candidate the origin uniform in the box
    (trimesh.sample.volume_rectangular: transform [(u - 0.5) extents, 1]), the target uniform in +-10000 rounded to 2
    decimals, up = [0, 0, -1], c2w = viewmatrix(target - origin, up, origin); a candidate is dropped when it sees a point
    of pc_unseen (check_proj).  Candidates are drawn VIEW_BATCH at a time - six uniforms each, row by row, so the sequence
    does not depend on the batch size - and tested by one ops.views_see_points call per batch; the first n accepted are
    kept in draw order.  pc_unseen=None accepts every candidate.  Deviation: a numpy Generator seeded with `seed` instead
    of `random` and numpy's global state.  Returns (c2ws, {'drawn': candidates tested, 'rejected': dropped among them})."""
    rng = np.random.default_rng(int(seed))
    extents, transform = np.asarray(extents, dtype=np.float64), np.asarray(transform, dtype=np.float64)
    up = np.array([0.0, 0.0, -1.0])
    pts = None
    if pc_unseen is not None:
        pts = _points(pc_unseen)
        if pts.shape[0] == 0:
            pts = None
    kept, drawn, rejected = [], 0, 0
    while len(kept) < n:
        u = rng.uniform(size=(VIEW_BATCH, 6))
        c2ws = np.tile(np.eye(4), (VIEW_BATCH, 1, 1))
        for k in range(VIEW_BATCH):
            origin = transform[:3, :3] @ ((u[k, :3] - 0.5) * extents) + transform[:3, 3]
            target = np.round(-10000.0 + 20000.0 * u[k, 3:], 2)
            c2ws[k, :3, :] = viewmatrix(target - origin, up, origin)
        ok = np.ones(VIEW_BATCH, dtype=bool)
        if pts is not None:
            ok = ~ops.views_see_points(pts, c2ws, K, H, W).cpu().numpy()
        for k in range(VIEW_BATCH):
            if len(kept) == n:
                break
            drawn += 1
            if ok[k]:
                kept.append(c2ws[k])
            else:
                rejected += 1
        if drawn >= 1000 * max(n, 1) and not kept:
            raise RuntimeError("sample_views: every one of %d candidate views sees an unseen point" % drawn)
    return np.stack(kept) if kept else np.zeros((0, 4, 4)), {"drawn": drawn, "rejected": rejected}


def depth_l1_metric(rec_v, rec_f, gt_v, gt_f, pc_unseen=None, align=True, n_imgs=1000, seed=0, views=None, chunk=32,
                    device=None):
    """In-memory calc_2d_metric: both meshes (vertices [V,3], faces [F,3]; numpy or torch) rendered from n_imgs views
    of 500 x 500 pixels, focal 300, principal point 249.5 (eval_recon.py:132-138), `chunk` views at a time; only the
    per-view sums of |gt depth - rec depth| come to the host.  views: an explicit [n,4,4] stack of c2w that bypasses
    the sampling (get_cam_position on the ground truth, sample_views with pc_unseen and seed).  align: the reconstruction
    is first moved by the ICP transform.  Returns {'depth_l1': the mean over views and pixels in cm, 'per_view': float64
    [n] in cm, 'views': the c2w used, 'drawn', 'rejected': sample_views' counters}."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    rec = torch.as_tensor(rec_v).to(dev, torch.float64).reshape(-1, 3)
    gt = torch.as_tensor(gt_v).to(dev, torch.float64).reshape(-1, 3)
    rec_f = torch.as_tensor(rec_f).to(dev, torch.int32).reshape(-1, 3)
    gt_f = torch.as_tensor(gt_f).to(dev, torch.int32).reshape(-1, 3)
    if align:
        rec = _transform(icp(rec, gt)[0], rec)
    info = {"drawn": 0, "rejected": 0}
    if views is None:
        extents, transform = get_cam_position(gt)
        views, info = sample_views(extents, transform, n_imgs, pc_unseen, seed)
    views = np.asarray(torch.as_tensor(views).detach().cpu().numpy(), dtype=np.float64).reshape(-1, 4, 4)
    rec32, gt32 = rec.float().contiguous(), gt.float().contiguous()
    K = (FOCAL, FOCAL, IMG_CX, IMG_CY)
    sums = []
    for lo in range(0, len(views), chunk):
        c = views[lo:lo + chunk]
        gt_depth = ops.render_mesh_depth(gt32, gt_f, c, K, IMG_H, IMG_W, Z_NEAR, Z_FAR, chunk)
        rec_depth = ops.render_mesh_depth(rec32, rec_f, c, K, IMG_H, IMG_W, Z_NEAR, Z_FAR, chunk)
        sums.append(ops.depth_l1(gt_depth, rec_depth))
    per_view = (torch.cat(sums).cpu().numpy() if sums else np.zeros(0)) / (IMG_H * IMG_W) * 100     # from m to cm
    return {"depth_l1": float(per_view.mean()) if len(per_view) else float("nan"), "per_view": per_view, "views": views,
            "drawn": info["drawn"], "rejected": info["rejected"]}


def calc_2d_metric(rec_meshfile, gt_meshfile, align=True, n_imgs=1000):
    """eval_recon.py:127-207: the depth L1 (cm) between renders of the ground-truth mesh and of the reconstruction from
    n_imgs random views inside the room that see none of the points of GT_pc_unseen.npy (the file beside the
    ground-truth mesh, '_culled.ply' replaced by '_pc_unseen.npy'; missing = the error of np.load, as in the reference);
    printed as the reference prints it and returned as depth_l1_metric's dict."""
    rec_v, rec_f, _ = read_ply(rec_meshfile)
    gt_v, gt_f, _ = read_ply(gt_meshfile)
    unseen_gt_pointcloud_file = gt_meshfile.replace('_culled.ply', '_pc_unseen.npy')
    pc_unseen = np.load(unseen_gt_pointcloud_file)
    rec_v = torch.as_tensor(rec_v).to(torch.float64)
    if align:
        T = get_align_transformation(rec_meshfile, gt_meshfile)
        rec_v = rec_v @ torch.from_numpy(T[:3, :3].T.copy()) + torch.from_numpy(T[:3, 3].copy())
    r = depth_l1_metric(rec_v, rec_f, gt_v, gt_f, pc_unseen=pc_unseen, align=False, n_imgs=n_imgs)
    print('Depth L1: ', r["depth_l1"])
    return r


if __name__ == '__main__':
    parser = argparse.ArgumentParser(description='Arguments to evaluate the reconstruction.')
    parser.add_argument('--rec_mesh', type=str, help='reconstructed mesh file path')
    parser.add_argument('--gt_mesh', type=str, help='ground truth mesh file path')
    parser.add_argument('-2d', '--metric_2d', action='store_true', help='enable 2D metric')
    parser.add_argument('-3d', '--metric_3d', action='store_true', help='enable 3D metric')
    parser.add_argument('--report', action='store_true', help='accuracy, completion, F-score, normal consistency: one '
                        '"name: value" line per key')
    parser.add_argument('--exact', action='store_true', help='--report measures to the other mesh, not to its samples')
    parser.add_argument('--f_threshold', type=float, default=0.05, help='distance threshold (m) of precision / recall / F-score')
    parser.add_argument('--error_mesh', type=str, default=None, metavar='PREFIX',
                        help='write PREFIX_accuracy.ply and PREFIX_completion.ply, vertices coloured by exact distance')
    parser.add_argument('--error_max', type=float, default=0.05, help='distance (m) at the top of the colour scale')
    args = parser.parse_args()
    if args.report:
        print_report(args.rec_mesh, args.gt_mesh, exact=args.exact, f_threshold=args.f_threshold)
    if args.error_mesh:
        write_error_meshes(args.rec_mesh, args.gt_mesh, args.error_mesh, max_err=args.error_max)
    if args.metric_3d:
        calc_3d_metric(args.rec_mesh, args.gt_mesh)
    if args.metric_2d:
        calc_2d_metric(args.rec_mesh, args.gt_mesh, n_imgs=1000)
