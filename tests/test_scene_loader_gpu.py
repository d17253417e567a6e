"""The one path of scene_loader.launch that no other test takes, for each of the three loaders: a build
with out=None ON A SIDE STREAM with explicit draws.  The kept tensors are then the fresh outputs (and
scratch) plus the uploaded draws, all allocated on the current stream, and stream != current: the side
stream has to wait for the current one, and every one of them has to be recorded on the side stream.

After current.wait_stream(side) every output must be BIT-equal to the same build on the current stream
and to host_batch with the same draws.

Shapes: B = 2, one scene of 50 and one of 3000 points from the modules' own synthetic writers; N = 64
(the 50-point scene is sampled with replacement) and N = 2049 (one slot past a 2048-slot chunk of the
points kernels); kinds semi (1 labeled + 1 unlabeled row) and eval for the labeled loaders.
"""
import importlib
import os

import numpy as np
import pytest
import torch

from conftest import load_pkg

load_pkg()
V = importlib.import_module("3dioumatch_amd.votenet")
SN = importlib.import_module("3dioumatch_amd.votenet.scannet_data")
SU = importlib.import_module("3dioumatch_amd.votenet.sunrgbd_data")
SC = importlib.import_module("3dioumatch_amd.votenet.scan_data")
DEV = torch.device("cuda", 0)
SIZES = (50, 3000)
COUNTER = 5
pytestmark = pytest.mark.gpu


def host(batch):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in batch.items()}


def assert_same_bits(got, want, what):
    assert set(got) == set(want), what
    report = {}
    for k, w in want.items():
        g = got[k]
        if isinstance(w, tuple):
            assert g == w, (what, k)
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k)
        report[k] = int((np.ascontiguousarray(g).view(np.uint8) != np.ascontiguousarray(w).view(np.uint8)).sum())
    print(what, "bytes that differ per key:", {k: v for k, v in report.items() if v} or "none")
    assert not any(report.values()), (what, report)


def labeled_loader(which, tmp_path, num_points):
    d = str(tmp_path)
    if which == "scannet":
        names = ["scene0000_00", "scene0001_00"]
        for i, (name, n) in enumerate(zip(names, SIZES)):
            SN.write_synthetic_scans(d, [name], num_points=n, instances=9, boxes=7, seed=20 + i)
        scenes = SN.ScanNetScenes(d, names, DEV, use_color=True, use_height=True)
        return SN.ScanNetLoader(scenes, V.scannet_config(), num_points, seed=3)
    names = ["000001", "000002"]
    for i, (name, n) in enumerate(zip(names, SIZES)):
        SU.write_synthetic_scans(d, [name], num_points=n, boxes=6, seed=30 + i)
    scenes = SU.SunRgbdScenes(d, names, DEV, use_color=True, use_height=True, votes=which.split("-")[1])
    return SU.SunRgbdLoader(scenes, V.sunrgbd_config(), num_points, seed=3)


@pytest.mark.parametrize("kind", ["semi", "eval"])
@pytest.mark.parametrize("num_points", [64, 2049])
@pytest.mark.parametrize("which", ["scannet", "sunrgbd-file", "sunrgbd-boxes"])
def test_fresh_build_on_a_side_stream_with_explicit_draws(tmp_path, which, num_points, kind):
    loader = labeled_loader(which, tmp_path, num_points)
    lab, unl = ([0], [1]) if kind == "semi" else ([0, 1], None)
    draws = loader.host_draws(kind, lab, unl, COUNTER)
    assert set(draws) == ({"idx", "ema_idx", "u"} if kind == "semi" else {"idx"})
    current, side = torch.cuda.current_stream(DEV), torch.cuda.Stream(DEV)
    on_side = loader.build(kind, lab, unl, COUNTER, draws=draws, stream=side)
    current.wait_stream(side)
    on_side = host(on_side)
    assert on_side["point_clouds"].shape == (2, num_points, 7)
    assert_same_bits(on_side, host(loader.build(kind, lab, unl, COUNTER, draws=draws)), "side vs current stream")
    want = loader.host_batch(kind, lab, unl, COUNTER, draws=draws)
    want["supervised_mask_host"] = (1, 0) if kind == "semi" else (1, 1)
    assert_same_bits(on_side, want, "side stream vs host_batch")


@pytest.mark.parametrize("num_points", [64, 2049])
def test_fresh_scan_batch_on_a_side_stream_with_explicit_draws(tmp_path, num_points):
    paths = []
    for i, n in enumerate(SIZES):
        paths.append(os.path.join(str(tmp_path), "scan%d.npy" % i))
        np.save(paths[-1], SC.synthetic_clouds(1, n, seed=40 + i)[0])
    loader = SC.ScanLoader(SC.ScanStore.from_files(paths, DEV), num_points, use_color=True, seed=3)
    draws = loader.host_draws([0, 1], COUNTER)
    current, side = torch.cuda.current_stream(DEV), torch.cuda.Stream(DEV)
    on_side = loader.batch([0, 1], COUNTER, draws=draws, stream=side)
    current.wait_stream(side)
    on_side = host(on_side)
    assert on_side["point_clouds"].shape == (2, num_points, 7)
    assert_same_bits(on_side, host(loader.batch([0, 1], COUNTER, draws=draws)), "side vs current stream")
    assert_same_bits(on_side, loader.host_batch([0, 1], COUNTER, draws=draws), "side stream vs host_batch")
