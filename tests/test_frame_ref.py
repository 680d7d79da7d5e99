"""tests/frame_ref.py (the numpy float32 model of ops.prepare_frame) against BaseDataset.__getitem__, on the three tiny
sequences the GPU test uses and by the same criteria - no GPU needed.  This is where the float32 arithmetic is shown to
stay inside the undistortion cap on these very images before a kernel runs."""
import numpy as np
import pytest
import torch

from tests import frame_ref as fr


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """name -> (reader, undistorted, host items): every sequence written and read on the host once."""
    out = {}
    for name in fr.CASES:
        reader, undistorted = fr.open_case(name, tmp_path_factory.mktemp(name))
        assert len(reader) == fr.N_FRAMES
        poses = [p.clone() for p in reader.poses]
        items = [reader[k] for k in range(len(reader))]
        out[name] = (reader, undistorted, items, poses)
    return out


@pytest.mark.parametrize("name", list(fr.CASES))
def test_model_matches_the_host_reader(cases, name):
    from myslam_amd.src.utils import datasets as ds
    reader, undistorted, items, _ = cases[name]
    spec = ds.FrameSpec.from_reader(reader)
    for k, (idx, hc, hd, _) in enumerate(items):
        rgb, dep = fr.raw_images(reader, k)
        assert rgb.dtype == np.uint8 and dep.dtype == np.uint16 and (dep == 0).any() and (dep == 65535).any()
        color, depth = fr.prepare_frame_ref(rgb, dep, spec)
        assert hc.dtype == torch.float64 and hd.dtype == torch.float32
        fr.check_against_host(color, depth, hc.numpy(), hd.numpy(), undistorted, f"{name}[{k}]")


def test_sequences_take_every_stage(cases):
    """The shapes say which stages ran: nothing for Replica; colour resize and trim for ScanNet; undistortion, crop_size
    and trim for TUM."""
    from myslam_amd import ops
    from myslam_amd.src.utils import datasets as ds
    shapes = {name: tuple(c[2][0][1].shape) for name, c in cases.items()}
    assert shapes == {"replica": (23, 37, 3), "scannet": (20, 28, 3), "tum": (14, 22, 3), "tum_scale2": (14, 22, 3)}
    stages = {}
    for name, (reader, undistorted, _, _) in cases.items():
        spec = ds.FrameSpec.from_reader(reader)
        rgb, dep = fr.raw_images(reader, 0)
        assert ops.frame_out_shape(rgb.shape[:2], dep.shape, spec.crop_size, spec.crop_edge) == shapes[name][:2]
        assert (spec.grid is not None) == undistorted
        stages[name] = (spec.grid is not None, rgb.shape[:2] != dep.shape, spec.crop_size is not None, spec.crop_edge > 0)
    # (undistort, colour resize, crop_size, trim)
    assert stages == {"replica": (False, False, False, False), "scannet": (False, True, False, True),
                      "tum": (True, False, True, True), "tum_scale2": (True, False, True, True)}
    d1, d2 = cases["tum"][2][1][2], cases["tum_scale2"][2][1][2]
    assert torch.equal(d2, d1 * 2.0)


def test_undistort_map_split_keeps_undistort(cases):
    """datasets.undistort = undistort_map + resampling: the map is the grid the function always built, and the model's
    undistortion reproduces torch's CPU grid_sample byte for byte or within the cap."""
    from myslam_amd.src.utils import datasets as ds
    reader = cases["tum"][0]
    K, dist = reader._K_dist()
    grid = ds.undistort_map(K, dist, 24, 32)
    assert grid.dtype == torch.float32 and tuple(grid.shape) == (24, 32, 2)
    rgb, _ = fr.raw_images(reader, 0)
    host = ds.undistort(rgb, K, dist)
    assert host.dtype == np.uint8 and (host != rgb).any()                                # the map moves pixels
    model = fr.undistort_ref(rgb, grid.numpy())
    diff = np.abs(model.astype(int) - host.astype(int))
    assert diff.max() <= 1 and (diff != 0).any(-1).mean() <= fr.UNDISTORT_CAP          # share of pixels


def test_frame_spec_and_out_shape(cases):
    from myslam_amd import ops
    from myslam_amd.src.utils import datasets as ds
    spec = ds.FrameSpec.from_reader(cases["tum_scale2"][0])
    assert (spec.png_depth_scale, spec.scale, spec.crop_size, spec.crop_edge) == (5000.0, 2.0, (18, 26), 2)
    assert ds.FrameSpec.from_reader(cases["replica"][0]).grid is None
    assert ops.frame_out_shape((24, 32), (24, 32), (18, 26), 2) == (14, 22)
    assert ops.frame_out_shape((49, 65), (24, 32), None, 2) == (20, 28)
    for bad in (((24, 32), (24, 32), (18, 26), 9), ((0, 32), (24, 32), None, 0), ((24, 32), (24, 40000), None, 0)):
        with pytest.raises(RuntimeError):
            ops.frame_out_shape(*bad)


def test_frame_stream_host_path_and_poses(cases):
    """FrameStream(native=False) on the CPU: the reader's items (colour cast to float32), poses scaled once on a copy."""
    from myslam_amd.src.utils import datasets as ds
    reader, _, items, poses0 = cases["tum_scale2"]
    # a fresh reader: the fixture's was read once, which scaled its stored poses in place
    fresh, _ = fr.open_case("tum_scale2", reader.input_folder + "_again")
    stream = ds.FrameStream(fresh, "cpu", native=False)
    for _ in range(2):                                   # iterating twice does not scale twice
        got = list(stream)
        assert [g[0] for g in got] == list(range(fr.N_FRAMES))
        for (idx, c, d, p), (_, hc, hd, hp) in zip(got, items):
            assert c.dtype == torch.float32 and torch.equal(c, hc.float()) and torch.equal(d, hd)
            assert torch.equal(p, hp)                    # the host item's pose after its one scaling
    for p, p0 in zip(fresh.poses, poses0):
        assert torch.equal(p, p0)                        # the reader's own poses were left alone
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        next(iter(ds.FrameStream(fresh, "cpu")))
