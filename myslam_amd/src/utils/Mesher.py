"""The reference's Mesher (src/utils/Mesher.py) on the HIP path: the field query, the frame hull and mesh extraction.

The `Mesher` class below has the reference's constructor and these functions as its methods.  The functions keep the
reference's signatures and can also be bound onto the reference's own Mesher class one line each:

    from myslam_amd.src.utils import Mesher as hip_mesher
    Mesher.eval_points = hip_mesher.eval_points                        # Mesher.py:130-157
    Mesher.get_bound_from_frames = hip_mesher.get_bound_from_frames    # Mesher.py:63-128
    Mesher.get_mesh = hip_mesher.get_mesh                              # Mesher.py:188-262

and, for the reference's own hull construction (a TSDF fusion of the keyframes, ops.TSDFVolume) instead of the default:

    Mesher.get_bound_from_frames = hip_mesher.get_bound_from_frames_tsdf

eval_points: same arguments, same [N,4] result (rgb, sdf with -1 outside the bound).  The bound test is folded into the
decode kernel (ESLAM_DECODE_MASK_OUTSIDE), so a batch is one launch instead of a decode plus 8 mask / index ops, and all
batches write into one output tensor (no torch.cat).

get_bound_from_frames: the keyframes' valid depth back-projected (ops.image_rays) plus the camera centres, bounded by
support half-spaces along a fixed set of 1024 directions and scaled by mesh_bound_scale - an outer approximation of the
reference's convex hull of an open3d TSDF mesh.

get_mesh: the grid of get_grid_uniform, the field on it with the bound and hull masks (ops.sdf_grid: the points are
never materialised), marching cubes (ops.marching_cubes), vertex colours through eval_points, a binary PLY.  Needs none
of skimage, open3d or trimesh.
"""
import ctypes
import math

import numpy as np
import torch

from ... import _hip, ops


def eval_points(self, p, all_planes, decoders):
    _hip.require_gpu_f32("p", p)
    p = ops._c(p.detach().reshape(-1, 3))
    N = p.shape[0]
    dev = p.device
    bound6 = ops.bound_to_host(decoders.bound)
    same_bound = bound6 == ops.bound_to_host(self.bound)
    # (inside ops.mixed_precision(half, points=True): on the half copies, the field that was trained and rendered)
    arr, _ = _hip.make_planes(tuple([t.detach() for t in grp] for grp in all_planes), half=ops.points_half())
    dec, keep = _hip.make_decoders([t.detach() for t in ops.decoder_params(decoders)], ops.beta_tensor(10, dev))
    out = torch.empty(N, 4, device=dev)
    lib = _hip.lib()
    step = int(self.points_batch_size)
    flags = 2 if same_bound else 0                       # ESLAM_DECODE_MASK_OUTSIDE
    with _hip.on_device(dev):
        for lo in range(0, N, step):                     # Mesher.py:141: torch.split(p, points_batch_size)
            n = min(step, N - lo)
            _hip.check(lib.eslam_decode_fwd(arr, ctypes.byref(dec), _hip.make_bound(bound6),
                                            ctypes.c_void_p(p.data_ptr() + lo * 12), n, flags,
                                            ctypes.c_void_p(out.data_ptr() + lo * 16), None, _hip.stream_handle(dev)),
                       "eslam_decode_fwd")
    if not same_bound:      # a mesher bound that differs from the decoders' normalisation bound: mask with its own
        b = self.bound.to(dev)
        inside = ((p < b[:, 1]) & (p > b[:, 0])).all(dim=1)
        out[~inside, -1] = -1
    return out


# ----------------------------------------------------------------------------------------------
# frame hull (Mesher.py:63-128)
# ----------------------------------------------------------------------------------------------
N_DIRECTIONS = 1024
_dirs_cache = {}


def support_directions():
    """float64 [1024,3] unit vectors: the 26 directions of the 3x3x3 lattice (exact for box-shaped rooms) and a
    Fibonacci sphere of 998 points.  A constant of the method, not an option."""
    d = _dirs_cache.get("d")
    if d is None:
        lat = torch.tensor([(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if (i, j, k) != (0, 0, 0)],
                           dtype=torch.float64)
        n = N_DIRECTIONS - lat.shape[0]
        k = torch.arange(n, dtype=torch.float64) + 0.5
        z = 1.0 - 2.0 * k / n
        r = torch.sqrt(1.0 - z * z)
        phi = k * math.pi * (3.0 - math.sqrt(5.0))
        fib = torch.stack([r * torch.cos(phi), r * torch.sin(phi), z], 1)
        d = torch.cat([lat / lat.norm(dim=1, keepdim=True), fib], 0)
        _dirs_cache["d"] = d
    return d


class FrameHull:
    """The convex region {p : n.p + d <= 0 for every row (n, d) of halfspaces [K,4]} (float64)."""

    def __init__(self, halfspaces):
        self.halfspaces = halfspaces

    def contains(self, points):
        """bool [N] (trimesh.Trimesh.contains of the reference's hull, Mesher.py:211), on the points' device."""
        p = torch.as_tensor(points)
        hs = self.halfspaces.to(p.device, torch.float64)
        out = torch.ones(p.shape[0], dtype=torch.bool, device=p.device)
        for lo in range(0, p.shape[0], 1 << 16):
            q = p[lo:lo + (1 << 16)].to(torch.float64)
            out[lo:lo + q.shape[0]] = (q @ hs[:, :3].T + hs[:, 3]).le(0).all(dim=1)
        return out


def halfspaces_from_points(points, mesh_bound_scale=1.02, chunk=1 << 15):
    """float64 [K,4] half-spaces (d, -h') bounding the point set [P,3] (any device): h(d) = max_p d.p over the fixed
    directions, scaled about c, the mean of the distinct support points: h' = s h + (1 - s) d.c.  Contains every input
    point (h' >= h >= d.c for s >= 1)."""
    p = torch.as_tensor(points)
    dev = p.device
    dirs = support_directions().to(dev)
    best = torch.full((dirs.shape[0],), -math.inf, dtype=torch.float64, device=dev)
    arg = torch.zeros(dirs.shape[0], dtype=torch.int64, device=dev)
    for lo in range(0, p.shape[0], chunk):
        proj = p[lo:lo + chunk].to(torch.float64) @ dirs.T                 # [chunk, K]
        v, i = proj.max(dim=0)
        better = v > best
        best = torch.where(better, v, best)
        arg = torch.where(better, i + lo, arg)
    support = torch.unique(arg)
    c = p[support].to(torch.float64).mean(dim=0)
    s = float(mesh_bound_scale)
    h = s * best + (1.0 - s) * (dirs @ c)
    return torch.cat([dirs, -h[:, None]], 1)


def keyframe_points(self, keyframe_dict):
    """float32 [P,3] on the keyframes' device: every valid depth pixel (> 0) back-projected with its est_c2w through
    ops.image_rays (reference camera convention, src/common.py:183-201), then the camera centres."""
    pts, cams = [], []
    for kf in keyframe_dict:
        c2w = kf["est_c2w"]
        depth = kf["depth"]
        ro, rd = ops.image_rays(int(self.H), int(self.W), float(self.fx), float(self.fy), float(self.cx), float(self.cy),
                                c2w.to(depth.device, torch.float32))
        d = depth.reshape(-1)
        ok = d > 0
        pts.append(ro[ok] + rd[ok] * d[ok, None])
        cams.append(c2w[:3, 3].to(depth.device, torch.float32)[None])
    return torch.cat(pts + cams, 0)


def get_bound_from_frames(self, keyframe_dict, scale=1):
    """Mesher.py:63-128 without open3d: a FrameHull around the keyframes' back-projected depth and camera centres.
    (`scale` only set the reference's TSDF voxel size.)"""
    return FrameHull(halfspaces_from_points(keyframe_points(self, keyframe_dict), self.mesh_bound_scale))


def get_bound_from_frames_tsdf(self, keyframe_dict, scale=1, voxel=None):
    """Mesher.py:63-128 by the reference's own construction, to be bound in place of get_bound_from_frames by whoever wants
    it: the keyframes' depth fused with est_c2w into a TSDF volume over marching_cubes_bound (ops.TSDFVolume: voxel
    4 scale / 512 unless given, truncation 0.04 scale, no colour), its mesh's vertices plus the camera centres bounded by
    the FrameHull's support half-spaces and scaled by mesh_bound_scale.  Deviations from open3d: DESIGN.md section 17."""
    voxel = 4.0 * scale / 512.0 if voxel is None else voxel
    dev = keyframe_dict[0]["depth"].device
    vol = ops.TSDFVolume(self.marching_cubes_bound, voxel, 0.04 * scale, color=False, device=dev)
    K = (float(self.fx), float(self.fy), float(self.cx), float(self.cy))
    vol.integrate(((i, None, kf["depth"], kf["est_c2w"]) for i, kf in enumerate(keyframe_dict)), K)
    verts, _, _ = vol.extract_mesh()
    cams = torch.stack([kf["est_c2w"][:3, 3].to(verts.device, torch.float32) for kf in keyframe_dict])
    return FrameHull(halfspaces_from_points(torch.cat([verts, cams], 0), self.mesh_bound_scale))


# ----------------------------------------------------------------------------------------------
# mesh (Mesher.py:158-262)
# ----------------------------------------------------------------------------------------------
def grid_axes(marching_cubes_bound, resolution):
    """(x, y, z) float64 numpy axes of get_grid_uniform (Mesher.py:158-186): padding 0.05, nsteps rounded from the
    float64 bound."""
    b = torch.as_tensor(marching_cubes_bound, dtype=torch.float64)
    padding = 0.05
    out = []
    for k in range(3):
        n = ((b[k][1] - b[k][0] + 2 * padding) / resolution).round().int().item()
        out.append(np.linspace(float(b[k][0]) - padding, float(b[k][1]) + padding, n))
    return out


NO_SURFACE = 'marching_cubes error. Possibly no surface extracted from the level set.'


def vertex_normals(self, vertices, all_planes, decoders):
    """float32 numpy [V,3]: the unit surface normals of a mesh at its own vertices (scene units, as extract_mesh and the
    files give them): +grad sdf of the field at vertices * self.scale, one fused launch (Decoders.sdf_normals).  The
    direction is towards free space, the side marching cubes' face winding faces.  Zero where the gradient vanishes."""
    dev = ops.decoder_params(decoders)[0].device
    v = torch.as_tensor(np.ascontiguousarray(vertices, dtype=np.float32)).reshape(-1, 3).to(dev)
    return decoders.sdf_normals(v * self.scale, all_planes).cpu().numpy()


def extract_mesh(self, all_planes, decoders, keyframe_dict, device='cuda:0', color=True, normals=False):
    """get_mesh without the file: (vertices float32 [V,3] in scene units / self.scale, faces int32 [F,3],
    colours float32 [V,3] or None) as numpy arrays, or None when the level set has no surface.  normals=True: a fourth
    element, the unit normals float32 [V,3] of vertex_normals."""
    with torch.no_grad():
        dev = torch.device(device)
        x, y, z = grid_axes(self.marching_cubes_bound, self.resolution)
        axes = [torch.from_numpy(a).float().to(dev) for a in (x, y, z)]
        hull = get_bound_from_frames(self, keyframe_dict, self.scale)
        vol = ops.sdf_grid(all_planes, decoders, axes, self.bound, hull.halfspaces)
        origin = (x[0], y[0], z[0])
        spacing = (x[2] - x[1], y[2] - y[1], z[2] - z[1])
        verts, faces = ops.marching_cubes(vol, self.level_set, origin, spacing)
        del vol
        if faces.shape[0] == 0:
            return None
        colours = None
        if color:
            colours = eval_points(self, verts, all_planes, decoders)[:, :3].cpu().numpy()
        vertices = verts.cpu().numpy()
        vertices /= self.scale
        if normals:
            return vertices, faces.cpu().numpy(), colours, vertex_normals(self, vertices, all_planes, decoders)
        return vertices, faces.cpu().numpy(), colours


def get_mesh(self, mesh_out_file, all_planes, decoders, keyframe_dict, device='cuda:0', color=True, normals=False):
    """Mesher.py:188-262: extract the mesh and write it as a binary PLY (write_ply).  No surface: the reference's message,
    no file.  normals=True: the file carries the vertex normals of vertex_normals (nx, ny, nz)."""
    m = extract_mesh(self, all_planes, decoders, keyframe_dict, device, color, normals)
    if m is None:
        print(NO_SURFACE)
        return
    write_ply(mesh_out_file, *m)


class Mesher:
    """The reference's class (src/utils/Mesher.py:42-61) over the functions above: same constructor, the attributes those
    functions read, the functions as its methods.  `eslam` provides bound, H, W, fx, fy, cx, cy (after update_cam) and,
    optionally, renderer and verbose.  The reference's constructor also opens a second dataset reader that none of its
    methods uses; that is left out."""

    def __init__(self, cfg, args, eslam, points_batch_size=500000, ray_batch_size=100000):
        self.points_batch_size = points_batch_size
        self.ray_batch_size = ray_batch_size
        self.renderer = getattr(eslam, 'renderer', None)
        self.scale = cfg['scale']
        self.resolution = cfg['meshing']['resolution']
        self.level_set = cfg['meshing']['level_set']
        self.mesh_bound_scale = cfg['meshing']['mesh_bound_scale']
        self.bound = eslam.bound
        self.verbose = getattr(eslam, 'verbose', False)
        self.marching_cubes_bound = torch.from_numpy(np.array(cfg['mapping']['marching_cubes_bound']) * self.scale)
        self.H, self.W, self.fx, self.fy, self.cx, self.cy = eslam.H, eslam.W, eslam.fx, eslam.fy, eslam.cx, eslam.cy

    eval_points = eval_points
    keyframe_points = keyframe_points
    get_bound_from_frames = get_bound_from_frames
    get_bound_from_frames_tsdf = get_bound_from_frames_tsdf
    vertex_normals = vertex_normals
    extract_mesh = extract_mesh
    get_mesh = get_mesh


def write_ply(path, vertices, faces, colors=None, normals=None):
    """Binary little-endian PLY: vertex x y z float (+ nx ny nz float directly after z, the order open3d, MeshLab and
    trimesh write) (+ red green blue alpha uchar, colour round(255 c) clipped, alpha 255), face
    `list uchar int vertex_indices`."""
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}",
            "property float x", "property float y", "property float z"]
    vfields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals is not None:
        nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        if nrm.shape[0] != v.shape[0]:
            raise ValueError(f"write_ply: {nrm.shape[0]} normals for {v.shape[0]} vertices")
        head += ["property float nx", "property float ny", "property float nz"]
        vfields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if colors is not None:
        head += ["property uchar red", "property uchar green", "property uchar blue", "property uchar alpha"]
        vfields += [("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")]
    head += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    vrec = np.empty(v.shape[0], dtype=vfields)
    vrec["x"], vrec["y"], vrec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if normals is not None:
        vrec["nx"], vrec["ny"], vrec["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    if colors is not None:
        c = np.clip(np.round(255.0 * np.asarray(colors, dtype=np.float64)), 0, 255).astype(np.uint8).reshape(-1, 3)
        vrec["red"], vrec["green"], vrec["blue"] = c[:, 0], c[:, 1], c[:, 2]
        vrec["alpha"] = 255
    frec = np.empty(f.shape[0], dtype=[("n", "u1"), ("v", "<i4", (3,))])
    frec["n"] = 3
    frec["v"] = f
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def _ply_header(data):
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError("not a PLY file")
    end = data.index(b"\n", end) + 1
    fmt, elements = None, []
    for line in data[:end].decode("ascii", "replace").splitlines():
        tok = line.split()
        if not tok or tok[0] in ("comment", "obj_info", "ply", "end_header"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            if tok[1] == "list":             # (name, count type, item type)
                elements[-1][2].append((tok[4], _PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]]))
            else:
                elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]], None))
    if fmt not in ("ascii", "binary_little_endian", "binary_big_endian"):
        raise ValueError(f"unsupported PLY format {fmt!r}")
    return fmt, elements, end


def _ply_read_binary(data, off, n, props, bo):
    """One element of a binary PLY: ({scalar name: array [n]}, {list name: list of arrays}), offset after it."""
    if all(lt is None for _, _, lt in props):
        dt = np.dtype([(name, bo + t) for name, t, _ in props])
        rec = np.frombuffer(data, dtype=dt, count=n, offset=off)
        return {name: rec[name] for name, _, _ in props}, {}, off + n * dt.itemsize
    # lists: try one uniform count per list (the common case: triangles), else walk the records
    if n > 0:
        fields, o, uniform = [], off, True
        for name, t, lt in props:
            if lt is None:
                fields.append((name, bo + t))
                o += np.dtype(t).itemsize
            else:
                k = int(np.frombuffer(data, dtype=bo + t, count=1, offset=o)[0])
                fields += [(name + "#n", bo + t), (name, bo + lt, (k,))]
                o += np.dtype(t).itemsize + k * np.dtype(lt).itemsize
        dt = np.dtype(fields)
        if off + n * dt.itemsize <= len(data):
            rec = np.frombuffer(data, dtype=dt, count=n, offset=off)
            uniform = all((rec[name + "#n"] == rec[name].shape[1]).all() for name, _, lt in props if lt is not None)
            if uniform:
                return ({name: rec[name] for name, _, lt in props if lt is None},
                        {name: rec[name] for name, _, lt in props if lt is not None}, off + n * dt.itemsize)
    scal = {name: np.empty(n, dtype=t) for name, t, lt in props if lt is None}
    lists = {name: [] for name, _, lt in props if lt is not None}
    for i in range(n):
        for name, t, lt in props:
            v = np.frombuffer(data, dtype=bo + t, count=1, offset=off)[0]
            off += np.dtype(t).itemsize
            if lt is None:
                scal[name][i] = v
            else:
                lists[name].append(np.frombuffer(data, dtype=bo + lt, count=int(v), offset=off))
                off += int(v) * np.dtype(lt).itemsize
    return scal, lists, off


def _ply_read_ascii(lines, pos, n, props):
    scal = {name: np.empty(n, dtype=t) for name, t, lt in props if lt is None}
    lists = {name: [] for name, _, lt in props if lt is not None}
    for i in range(n):
        tok = lines[pos + i].split()
        j = 0
        for name, t, lt in props:
            if lt is None:
                scal[name][i] = float(tok[j]) if t[0] == "f" else int(tok[j])
                j += 1
            else:
                k = int(tok[j])
                lists[name].append(np.array([float(x) if lt[0] == "f" else int(x) for x in tok[j + 1:j + 1 + k]]))
                j += 1 + k
    return scal, lists, pos + n


def _fan(polys):
    """Triangles [F,3] of polygons ([P,k] array or list of index arrays), each fanned from its first vertex."""
    if isinstance(polys, np.ndarray):
        k = polys.shape[1]
        if k < 3:
            return np.zeros((0, 3), dtype=np.int64)
        return np.stack([np.stack([polys[:, 0], polys[:, j], polys[:, j + 1]], 1) for j in range(1, k - 1)], 1).reshape(-1, 3)
    tris = [(p[0], p[j], p[j + 1]) for p in polys for j in range(1, len(p) - 1)]
    return np.array(tris, dtype=np.int64).reshape(-1, 3)


def _ply_elements(path):
    """[(element name, {scalar property: array}, {list property: arrays})] of a PLY file, in file order."""
    with open(path, "rb") as fh:
        data = fh.read()
    fmt, elements, off = _ply_header(data)
    lines, pos = None, 0
    if fmt == "ascii":
        lines = [ln for ln in data[off:].decode("ascii").splitlines() if ln.strip()]
    bo = ">" if fmt == "binary_big_endian" else "<"
    out = []
    for name, n, props in elements:
        if fmt == "ascii":
            scal, lists, pos = _ply_read_ascii(lines, pos, n, props)
        else:
            scal, lists, off = _ply_read_binary(data, off, n, props, bo)
        out.append((name, scal, lists))
    return out


def _mesh_of(elements, path):
    verts, faces, colors, normals = None, np.zeros((0, 3), dtype=np.int64), None, None
    for name, scal, lists in elements:
        if name == "vertex":
            verts = np.stack([scal["x"], scal["y"], scal["z"]], 1).astype(np.float32)
            if all(c in scal for c in ("red", "green", "blue")):
                c = np.stack([scal["red"], scal["green"], scal["blue"]], 1)
                colors = (c.astype(np.float32) / 255.0).astype(np.float32) if c.dtype.kind in "iu" else c.astype(np.float32)
            if all(c in scal for c in ("nx", "ny", "nz")):
                normals = np.stack([scal["nx"], scal["ny"], scal["nz"]], 1).astype(np.float32)
        elif name == "face":
            key = "vertex_indices" if "vertex_indices" in lists else "vertex_index"
            faces = _fan(lists[key]).astype(np.int64)
    if verts is None:
        raise ValueError(f"{path}: no vertex element")
    return verts, faces, colors, normals


def read_ply(path):
    """(vertices float32 [V,3], faces int64 [F,3], colours float32 [V,3] in [0, 1] or None) of a PLY file: ASCII or
    binary (either byte order), any scalar vertex properties (x, y, z and red, green, blue are used; normals and other
    properties are skipped), faces as a `vertex_indices` (or `vertex_index`) list of any count and index type, polygons
    fan-triangulated from their first vertex, other elements skipped.  Reads what write_ply writes, bit for bit."""
    return _mesh_of(_ply_elements(path), path)[:3]


def read_ply_with_normals(path):
    """read_ply's three arrays and the vertex normals (nx, ny, nz) float32 [V,3], or None when the vertices carry none, from
    one pass over the file."""
    return _mesh_of(_ply_elements(path), path)


def read_ply_normals(path):
    """float32 [V,3]: the vertex normals (nx, ny, nz) of a PLY file, or None when its vertices carry none.  Reads what
    write_ply(normals=...) writes, bit for bit."""
    return _mesh_of(_ply_elements(path), path)[3]
