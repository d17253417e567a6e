"""GPU tests of the SUN RGB-D vote rule on the device (csrc/sunrgbd_batch.hip: sun_vote_row in
sun_votes_kernel and in the votes-from-boxes instantiation of sun_points_kernel) against the
reference's own extraction (tests/golden/sunrgbd_votes_ref.npz) and against the stored-votes path,
with the bounds of test_sunrgbd_votes.py.

Shapes: the five fixture scenes (about 400 points each; 9, 0, 64, 12 and 5 boxes) in one batch of
N = 2113 points per row: two 2048-slot workgroups per row, the second with a 65-slot tail, sampled
with replacement.
"""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

from conftest import load_pkg
from test_sunrgbd_votes import BATCHES, F32, GOLD, SCENES, check_rows, compare_batches, loaders, write_scenes

load_pkg()
SD = importlib.import_module("3dioumatch_amd.votenet.sunrgbd_data")
V = importlib.import_module("3dioumatch_amd.votenet")
DEV = torch.device("cuda", 0)
N = 2113
INVALID = 1  # hipErrorInvalidValue
pytestmark = pytest.mark.gpu


def host(batch):
    return {k: v.cpu().numpy() for k, v in batch.items() if torch.is_tensor(v)}


def test_vote_rows_of_a_boxes_store_reproduce_the_reference(tmp_path):
    from_file, from_boxes = loaders(tmp_path, DEV, N)
    st = from_boxes.scenes
    assert "votes" not in st.dev and "votes" in from_file.scenes.dev
    rows = st.vote_rows()
    assert rows.is_cuda and rows.dtype == torch.float32 and tuple(rows.shape) == (int(st.count.sum()), 10)
    rows = rows.cpu().numpy()
    for s, off, n in zip(SCENES, st.offset, st.count):
        check_rows(rows[off:off + n], s, "vote_rows")
    stored = from_file.scenes.vote_rows()
    assert stored.data_ptr() == from_file.scenes.dev["votes"].data_ptr()
    for s, off, n in zip(SCENES, st.offset, st.count):
        if s in F32:  # the device's rows are the stored float32(reference) rows, bit for bit
            assert torch.equal(stored[off:off + n].cpu(), torch.from_numpy(rows[off:off + n])), s


@pytest.mark.parametrize("explicit", [True, False], ids=["explicit_draws", "device_draws"])
@pytest.mark.parametrize("kind,lab,unl", BATCHES)
def test_batches_of_a_boxes_store_equal_the_file_store(tmp_path, kind, lab, unl, explicit):
    from_file, from_boxes = loaders(tmp_path, DEV, N)
    counter = 6
    draws = from_file.host_draws(kind, lab, unl, counter) if explicit else None
    want = host(from_file._build(kind, lab, unl, counter, draws=draws))
    got = host(from_boxes._build(kind, lab, unl, counter, draws=draws))
    if kind == "semi":
        assert "ema_point_clouds" in want and want["vote_label"].shape[0] == 4
    assert want["vote_label"].shape[1:] == (N, 9)
    assert want["vote_label_mask"].any() and (want["vote_label"] != 0).any()
    compare_batches(got, want, lab, "%s %s" % (kind, "explicit" if explicit else "device"))


@pytest.mark.parametrize("kind,lab,unl", BATCHES)
def test_every_vote_output_is_written_over_poisoned_memory(tmp_path, kind, lab, unl):
    _, from_boxes = loaders(tmp_path, DEV, N)
    out = from_boxes.allocate(kind, len(lab), len(unl or []))
    for t in out[0].values():
        t.fill_(float("nan") if t.dtype.is_floating_point else -123456789)
    b = host(from_boxes._build(kind, lab, unl, 2, out=out))
    assert np.isfinite(b["vote_label"]).all() and np.isfinite(b["point_clouds"]).all()
    assert np.isin(b["vote_label_mask"], (0, 1)).all()
    want = from_boxes.host_batch(kind, lab, unl, 2)
    assert np.array_equal(b["vote_label_mask"], want["vote_label_mask"])
    np.testing.assert_allclose(b["vote_label"], want["vote_label"], rtol=0, atol=2e-6)
    for r, s in enumerate(lab):
        if GOLD[SCENES[s] + "_bbox"].shape[0] == 0:
            assert (b["vote_label"][r] == 0).all() and (b["vote_label_mask"][r] == 0).all()
    if kind != "semi":
        assert any(GOLD[SCENES[s] + "_bbox"].shape[0] == 0 for s in lab)


def test_missing_boxes_and_null_pointers_are_refused_before_any_launch(tmp_path):
    _L = importlib.import_module("3dioumatch_amd._lib")
    _, from_boxes = loaders(tmp_path, DEV, N)
    d = from_boxes.scenes.dev
    stream = torch.cuda.current_stream(DEV).cuda_stream
    pc = torch.full((1, 64, 4), -7.0, device=DEV)
    vl = torch.full((1, 64, 9), -7.0, device=DEV)
    vm = torch.full((1, 64), -7, dtype=torch.int64, device=DEV)

    def args(boxes, nbox):
        a = importlib.import_module("3dioumatch_amd.records").SunBatchArgs()
        a.B, a.N, a.C, a.has_height, a.vote_rows, a.div256_from, a.num_heading_bin = 1, 64, 4, 1, 1, 1, 12
        a.cloud, a.offset, a.count = d["cloud"].data_ptr(), d["offset"].data_ptr(), d["count"].data_ptr()
        a.votes, a.boxes, a.nbox = None, boxes, nbox
        a.point_clouds, a.vote_label, a.vote_label_mask = pc.data_ptr(), vl.data_ptr(), vm.data_ptr()
        return a

    build = _L.lib.scene_sunrgbd_batch_build
    assert build(ctypes.byref(args(None, None)), stream) == INVALID
    assert build(ctypes.byref(args(d["boxes"].data_ptr(), None)), stream) == INVALID
    assert build(ctypes.byref(args(None, d["nbox"].data_ptr())), stream) == INVALID

    P = d["cloud"].shape[0]
    rows = torch.full((P, 10), -7.0, device=DEV)
    good = [d["cloud"].data_ptr(), 4, d["offset"].data_ptr(), d["count"].data_ptr(), d["boxes"].data_ptr(),
            d["nbox"].data_ptr(), len(SCENES), rows.data_ptr(), stream]
    for i in (0, 2, 3, 4, 5, 7):
        bad = list(good)
        bad[i] = None
        assert _L.lib.scene_sunrgbd_votes(*bad) == INVALID, i
    for i, v in ((1, 2), (6, 0), (6, -1)):
        bad = list(good)
        bad[i] = v
        assert _L.lib.scene_sunrgbd_votes(*bad) == INVALID, (i, v)
    torch.cuda.synchronize()
    for t in (pc, vl, vm, rows):  # nothing was launched: no output was touched
        assert bool((t == -7).all())
    # the same arguments with the boxes in place are accepted and write every element
    assert build(ctypes.byref(args(d["boxes"].data_ptr(), d["nbox"].data_ptr())), stream) == 0
    assert _L.lib.scene_sunrgbd_votes(*good) == 0
    torch.cuda.synchronize()
    assert not bool((pc == -7).any()) and not bool((vl == -7).any()) and not bool((vm == -7).any())
    assert not bool((rows == -7).any())
    assert torch.equal(rows, from_boxes.scenes.vote_rows())


def test_exported_votes_reload_as_a_file_store_with_the_same_batch(tmp_path):
    _, from_boxes = loaders(tmp_path, DEV, N)
    folder = str(tmp_path / "boxes")
    from_boxes.scenes.export_votes(folder)
    for s in SCENES:
        with np.load(os.path.join(folder, s + "_votes.npz")) as f:
            assert f["point_votes"].dtype == np.float64 and f["point_votes"].shape == GOLD[s + "_votes"].shape
    again = SD.SunRgbdScenes(folder, SCENES, DEV, use_color=False, use_height=True)  # votes="file"
    assert torch.equal(again.dev["votes"], from_boxes.scenes.vote_rows())
    reloaded = SD.SunRgbdLoader(again, from_boxes.config, N, seed=5)
    want = reloaded.pretrain_batch([0, 1, 2, 3, 4], 9)
    got = from_boxes.pretrain_batch([0, 1, 2, 3, 4], 9)
    assert set(got) == set(want)
    for k, w in want.items():
        if torch.is_tensor(w):
            assert torch.equal(got[k], w), k


def test_a_folder_without_vote_files_trains_through_feed(tmp_path):
    """Two supervised steps fed on the side stream from a folder that holds only `_pc.npz` and
    `_bbox.npy`: the yielded batches equal the host restatement and the losses are finite."""
    write_scenes(tmp_path, votes=False)
    scenes = SD.SunRgbdScenes(str(tmp_path), SCENES, DEV, use_color=False, use_height=True, votes="boxes")
    loader = SD.SunRgbdLoader(scenes, V.sunrgbd_config(), N, seed=5)
    plan = list(SD.epoch_plan(len(SCENES), 2, 0, seed=1))[:2]
    runner = V.SupervisedStep(loader.config, DEV, world_size=1, num_proposal=64, seed=3, graphs=False, lr=1e-3)
    seen, losses = [], []
    for b in SD.feed(runner, loader, plan, kind="pretrain"):
        seen.append({k: v.clone() for k, v in b.items() if torch.is_tensor(v)})
        losses.append(runner(b)[0].detach().clone())
    torch.cuda.synchronize()
    assert len(seen) == 2 and bool(torch.isfinite(torch.stack(losses)).all())
    for (counter, lab, unl), got in zip(plan, seen):
        want = loader.host_batch("pretrain", lab, unl, counter)
        got = host(got)
        assert np.array_equal(got["vote_label_mask"], want["vote_label_mask"])
        np.testing.assert_allclose(got["vote_label"], want["vote_label"], rtol=0, atol=2e-6)
