"""numpy model of ops.prepare_frame (csrc/eslam_frame.hip; include/eslam_hip.h eslam_frame_*): the same stages with the
same arithmetic - tap positions and weights in float64 rounded to float32, blends in float32 one operation at a time, the
undistortion in float32 with its three fused multiply-adds, the depth as two float32 operations.  tests/test_frame_ref.py
pins it against BaseDataset.__getitem__ without a GPU; tests/test_gpu_frames.py holds the kernels to the same criteria.

Also the three tiny sequences both test files read (write_replica / write_scannet / write_tum) and the criteria
themselves (check_against_host)."""
import os

import numpy as np

f32 = np.float32


# ---- the model ---------------------------------------------------------------------------------------------------------
def bilinear_taps(n_in, n_out, align):
    """(i0, i1 int64 [n_out], w0, w1 float32 [n_out]) of F.interpolate(mode='bilinear') along one axis, float64."""
    dst = np.arange(n_out, dtype=np.float64)
    if n_in == n_out:
        i = np.arange(n_out)
        return i, i, np.ones(n_out, f32), np.zeros(n_out, f32)
    if align:
        s = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
        src = s * dst
    else:
        src = np.maximum((n_in / n_out) * (dst + 0.5) - 0.5, 0.0)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    l1 = src - i0
    return i0, i0 + (i0 < n_in - 1), (1.0 - l1).astype(f32), l1.astype(f32)


def nearest_index(n_in, n_out):
    """F.interpolate(mode='nearest') of a float32 image: float32 scale, floor, clamp."""
    if n_in == n_out:
        return np.arange(n_out)
    s = f32(n_in) / f32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=f32) * s).astype(np.int64), n_in - 1)


def _resize(img, size, align):
    """float32 [h,w,3] -> [H,W,3]: wy0 (wx0 a + wx1 b) + wy1 (wx0 c + wx1 d), every operation float32."""
    y0, y1, wy0, wy1 = bilinear_taps(img.shape[0], size[0], align)
    x0, x1, wx0, wx1 = bilinear_taps(img.shape[1], size[1], align)
    wx0, wx1 = wx0[None, :, None], wx1[None, :, None]
    top = wx0 * img[y0][:, x0] + wx1 * img[y0][:, x1]
    bot = wx0 * img[y1][:, x0] + wx1 * img[y1][:, x1]
    out = wy0[:, None, None] * top + wy1[:, None, None] * bot
    # a pixel both of whose second weights are 0 is its single tap, untouched (1 v + 0 v' is v anyway)
    assert out.dtype == f32
    return out


def undistort_ref(rgb, grid):
    """uint8 [H,W,3] sampled at grid float32 [H,W,2], float32 in the order of torch's CPU grid_sample kernel, rounded half
    to even.  A fused multiply-add of a byte value is exact in float64 before its single rounding."""
    H, W = rgb.shape[:2]
    x = (grid[..., 0] + f32(1)) * (f32(W - 1) / f32(2))
    y = (grid[..., 1] + f32(1)) * (f32(H - 1) / f32(2))
    xf, yf = np.floor(x), np.floor(y)
    w, n = x - xf, y - yf
    e, s = f32(1) - w, f32(1) - n
    weights = (e * s, w * s, e * n, w * n)
    fin = (xf >= -2) & (xf <= W) & (yf >= -2) & (yf <= H)
    x0 = np.where(fin, xf, -2).astype(np.int64)
    y0 = np.where(fin, yf, -2).astype(np.int64)
    acc = None
    for k, wt in enumerate(weights):
        xx, yy = x0 + (k & 1), y0 + (k >> 1)
        ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        v = np.where(ok[..., None], rgb[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], 0).astype(f32)
        if acc is None:
            acc = v * wt[..., None]
        else:
            acc = (v.astype(np.float64) * wt[..., None].astype(np.float64) + acc.astype(np.float64)).astype(f32)
    return np.clip(np.rint(acc), 0, 255).astype(np.uint8)


def prepare_frame_ref(rgb, depth, spec):
    """(colour float32 [H',W',3], depth float32 [H',W']) from uint8 [Hc,Wc,3] and uint16 [Hd,Wd]; spec: a FrameSpec."""
    if spec.grid is not None:
        rgb = undistort_ref(rgb, spec.grid.numpy())
    size2 = spec.crop_size if spec.crop_size is not None else depth.shape
    c = _resize(_resize(rgb.astype(f32), depth.shape, align=False), size2, align=True)
    d = (depth.astype(f32) / f32(spec.png_depth_scale)) * f32(spec.scale)
    d = d[nearest_index(depth.shape[0], size2[0])][:, nearest_index(depth.shape[1], size2[1])]
    e = spec.crop_edge
    if e > 0:
        c, d = c[e:-e, e:-e], d[e:-e, e:-e]
    return np.ascontiguousarray(c / f32(255)), np.ascontiguousarray(d)


# ---- the criteria ------------------------------------------------------------------------------------------------------
COLOR_TOL = 1e-6            # a handful of float32 roundings at magnitude <= 1, each <= 6e-8, given exact weights
UNDISTORT_CAP = 0.002       # share of PIXELS (any channel) whose uint8 intermediate may round the other way
UNDISTORT_STEP = 1.0 / 255 + 1e-6


def check_against_host(color, depth, host_color, host_depth, undistorted, what=""):
    """color, depth: float32 arrays of the path under test; host_color float64, host_depth float32: the reader's item."""
    assert color.dtype == np.float32 and depth.dtype == np.float32
    assert color.shape == host_color.shape and depth.shape == host_depth.shape, (what, color.shape, host_color.shape)
    assert np.array_equal(depth.view(np.uint32), np.asarray(host_depth, dtype=f32).view(np.uint32)), f"{what}: depth bits differ"
    err = np.abs(color.astype(np.float64) - np.asarray(host_color, dtype=np.float64))
    beyond = err > COLOR_TOL
    pixels = beyond.any(-1)                             # a pixel is beyond when any of its channels is
    print(f"{what}: max colour error {err.max():.3e}, pixels beyond {COLOR_TOL:g}: {int(pixels.sum())} of {pixels.size}")
    if not undistorted:
        assert not beyond.any(), f"{what}: colour off by {err.max():.3e}"
    else:
        assert pixels.mean() <= UNDISTORT_CAP, f"{what}: {pixels.mean():.4%} of the pixels beyond {COLOR_TOL:g}"
        assert err.max() <= UNDISTORT_STEP, f"{what}: colour off by {err.max():.3e}"


# ---- the sequences -----------------------------------------------------------------------------------------------------
def smooth_image(rng, H, W):
    """uint8 [H,W,3]: a low-resolution random image resized up (smooth), plus a vertical step edge."""
    from PIL import Image
    small = rng.integers(30, 226, (max(2, H // 6), max(2, W // 6), 3)).astype(np.uint8)
    img = np.asarray(Image.fromarray(small).resize((W, H), Image.BICUBIC)).astype(np.int64)
    img[:, W // 2 + 1:] = np.clip(img[:, W // 2 + 1:] + 60, 0, 255)
    return img.astype(np.uint8)


def depth_image(rng, H, W):
    """uint16 [H,W]: a ramp with noise, holes (0) and saturated samples (65535)."""
    d = (2000 + 40 * np.arange(W)[None] + 25 * np.arange(H)[:, None] + rng.integers(0, 30, (H, W))).astype(np.uint16)
    d[rng.random((H, W)) < 0.08] = 0
    d[rng.random((H, W)) < 0.03] = 65535
    d[0, 0], d[-1, -1] = 0, 65535
    return d


def _pose(k):
    m = np.eye(4)
    c, s = np.cos(0.05 * k), np.sin(0.05 * k)
    m[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    m[:3, 3] = [0.1 * k, -0.02 * k, 0.3 + 0.05 * k]
    return m


N_FRAMES = 3


def write_replica(root, seed=1):
    """Replica layout, 23 x 37, nothing to resample."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    H, W = 23, 37
    os.makedirs(os.path.join(root, "results"))
    with open(os.path.join(root, "traj.txt"), "w") as f:
        for k in range(N_FRAMES):
            Image.fromarray(smooth_image(rng, H, W)).save(os.path.join(root, "results", f"frame{k:06d}.jpg"), quality=95)
            Image.fromarray(depth_image(rng, H, W)).save(os.path.join(root, "results", f"depth{k:06d}.png"))
            f.write(" ".join(f"{x:.9e}" for x in _pose(k).reshape(-1)) + "\n")
    return dict(dataset="replica", data=dict(input_folder=str(root)),
                cam=dict(H=H, W=W, fx=20.0, fy=20.0, cx=18.0, cy=11.0, png_depth_scale=6553.5, crop_edge=0))


def write_scannet(root, seed=2):
    """ScanNet layout: colour 49 x 65 beside depth 24 x 32, crop_edge 2."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    for sub in ("color", "depth", "pose"):
        os.makedirs(os.path.join(root, sub))
    for k in range(N_FRAMES):
        Image.fromarray(smooth_image(rng, 49, 65)).save(os.path.join(root, "color", f"{k}.jpg"), quality=95)
        Image.fromarray(depth_image(rng, 24, 32)).save(os.path.join(root, "depth", f"{k}.png"))
        np.savetxt(os.path.join(root, "pose", f"{k}.txt"), _pose(k))
    return dict(dataset="scannet", data=dict(input_folder=str(root)),
                cam=dict(H=24, W=32, fx=28.0, fy=28.0, cx=15.5, cy=11.5, png_depth_scale=1000.0, crop_edge=2))


def write_tum(root, seed=3):
    """TUM layout, 24 x 32: the freiburg1 distortion coefficients with its intrinsics scaled from 480 x 640 to the image,
    crop_size [18, 26], crop_edge 2."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    H, W = 24, 32
    os.makedirs(os.path.join(root, "rgb"))
    os.makedirs(os.path.join(root, "depth"))
    lines = {"rgb": ["# colour"], "depth": ["# depth"], "groundtruth": ["# timestamp tx ty tz qx qy qz qw"]}
    for k in range(N_FRAMES):
        t = 100.0 + 0.1 * k
        Image.fromarray(smooth_image(rng, H, W)).save(os.path.join(root, "rgb", f"{t:.6f}.png"))
        Image.fromarray(depth_image(rng, H, W)).save(os.path.join(root, "depth", f"{t:.6f}.png"))
        lines["rgb"].append(f"{t:.6f} rgb/{t:.6f}.png")
        lines["depth"].append(f"{t:.6f} depth/{t:.6f}.png")
        h = 0.025 * k
        lines["groundtruth"].append(f"{t:.6f} {0.1 * k:.6f} {-0.02 * k:.6f} {0.05 * k:.6f} 0 {np.sin(h):.9f} 0 {np.cos(h):.9f}")
    for name, rows in lines.items():
        with open(os.path.join(root, name + ".txt"), "w") as f:
            # (rgb.txt and depth.txt are read without skipping a header: rows only)
            f.write("\n".join(rows if name == "groundtruth" else rows[1:]) + "\n")
    s = W / 640.0
    return dict(dataset="tumrgbd", data=dict(input_folder=str(root)),
                cam=dict(H=H, W=W, fx=517.3 * s, fy=516.5 * s, cx=318.6 * s, cy=255.3 * s, png_depth_scale=5000.0,
                         crop_edge=2, crop_size=[18, 26], distortion=[0.2624, -0.9531, -0.0054, 0.0026, 1.1633]))


# name -> (writer, reader scale, undistorted)
CASES = {"replica": (write_replica, 1.0, False), "scannet": (write_scannet, 1.0, False), "tum": (write_tum, 1.0, True),
         "tum_scale2": (write_tum, 2.0, True)}


def open_case(name, root):
    """(reader, undistorted) of case `name`, its files written under root."""
    from types import SimpleNamespace
    from myslam_amd.src.utils import datasets as ds
    writer, scale, undistorted = CASES[name]
    cfg = writer(str(root))
    return ds.get_dataset(cfg, SimpleNamespace(input_folder=None), scale=scale, device="cpu"), undistorted


def raw_images(reader, k):
    """The decoded images of frame k: uint8 [Hc,Wc,3], uint16 [Hd,Wd]."""
    from myslam_amd.src.utils import datasets as ds
    return ds._imread_color(reader.color_paths[k]), ds._imread_depth(reader.depth_paths[k])
