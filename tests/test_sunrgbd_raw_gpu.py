"""Raw SUN RGB-D trainval scenes -> kept rows, floors and store rows on the MI355X:
scene_sunrgbd_raw_export (csrc/sunrgbd_raw.hip) against the numpy restatement at the golden's shapes --
floors with ==, every other array bit for bit -- with the scenes of a dtype in one chunk (workgroups
straddle scene boundaries), one scene per call, a chunk bound that splits the list, both kept counts,
the device's own draw and the recorded choice; twice; on poisoned allocations; the from_raw store's
batches against those of the store read back from its exported folder; its vote rows; a .mat cloud in
the label-free scan store; and tools/train.py --dataset sunrgbd for one epoch of each stage."""
import importlib
import inspect
import os
import runpy

import numpy as np
import pytest
import torch

import dirty_memory
from sunrgbd_raw_cases import (FLOAT32, KEPT, R, SCENES, assert_same_bits, assert_same_export, extra_record,
                               materialise, num_point, records, ref)
from test_dirty_memory import ALLOWED, uninitialised_sites

SUN = importlib.import_module("3dioumatch_amd.votenet.sunrgbd_data")
SC = importlib.import_module("3dioumatch_amd.votenet.scan_data")
V = importlib.import_module("3dioumatch_amd.votenet")

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOAT64 = tuple(s for s in SCENES if s not in FLOAT32)
# the scenes of one dtype side by side, so that a chunk holds several; behind them two clouds of distinct
# values with more points than either kept count (in float64 the golden has none)
ORDER = FLOAT32 + FLOAT64


def same(got, want, names, what):
    assert len(got) == len(want) == len(names)
    for s, g, w in zip(names, got, want):
        assert_same_export(g, w, "scene_sunrgbd_raw_export %s, scene %s (%s, %d raw points)"
                           % (what, s, g["pc"].dtype, 0 if s not in SCENES else ref()[s + "_raw"].shape[0]))


@pytest.fixture(scope="module")
def raw(tmp_path_factory):
    folder = materialise(tmp_path_factory.mktemp("sunrgbd_raw_gpu"))
    recs = records(folder, ORDER) + [extra_record("000098", 2300, np.float64, 3), extra_record("000099", 2500, np.float32, 4)]
    names = [r["name"] for r in recs]
    # the restatement, computed once per kept count: the project's draw, and the recorded choice where
    # the golden's scene was kept at that count
    host, choices = {}, {}
    for n in KEPT:
        choices[n] = {s: ref()[s + "_choice"] for s in SCENES if num_point(s) == n}
        host[n, "drawn"] = R.export_trainval(recs, None, n, seed=11)
        host[n, "given"] = R.export_trainval(recs, None, n, seed=11, choices=choices[n])
    return {"folder": folder, "records": recs, "names": names, "host": host, "choices": choices}


@pytest.mark.parametrize("n", KEPT)
def test_chunks_of_a_dtype_equal_the_restatement(raw, n):
    for kind, choices in (("drawn", None), ("given", raw["choices"][n])):
        got = R.export_trainval(raw["records"], DEV, n, seed=11, choices=choices)
        assert [g["pc"].shape for g in got] == [(n, 6)] * 8 and [g["rows"].shape for g in got] == [(n, 7)] * 8
        assert [g["bbox"].shape[0] for g in got] == [9, 64, 5, 0, 2, 4, 0, 0]
        same(got, raw["host"][n, kind], raw["names"], "in chunks of a dtype, %d kept, %s" % (n, kind))
    for s, g in zip(raw["names"], got):  # the recorded choice gives the reference's rows
        if s in raw["choices"][n]:
            assert_same_bits(g["pc"], ref()[s + "_pc"], s)


@pytest.mark.parametrize("n", KEPT)
def test_one_scene_per_call_and_a_split_list_equal_the_restatement(raw, n):
    choices = raw["choices"][n]
    for index, (rec, w) in enumerate(zip(raw["records"], raw["host"][n, "given"])):
        [g] = R.export_trainval([rec], DEV, n, seed=11, choices=choices, first_index=index)
        same([g], [w], [rec["name"]], "one scene per call, %d kept" % n)
    # chunks of two scenes at most: the bound splits each dtype's run, the draws keep their rows
    got = R.export_trainval(raw["records"], DEV, n, seed=11, choices=choices, chunk_points=3000)
    same(got, raw["host"][n, "given"], raw["names"], "chunk_points 3000, %d kept" % n)
    got = R.export_trainval(raw["records"], DEV, n, seed=11, chunk_points=1)
    same(got, raw["host"][n, "drawn"], raw["names"], "chunk_points 1, %d kept" % n)


def test_twice_is_bit_equal(raw):
    a = R.export_trainval(raw["records"], DEV, 1977, seed=5)
    b = R.export_trainval(raw["records"], DEV, 1977, seed=5)
    for s, x, y in zip(raw["names"], a, b):
        assert_same_export(x, y, s)
        assert_same_bits(np.asarray(x["floor"]), np.asarray(y["floor"]), s + " floor")


@pytest.mark.parametrize("fill", dirty_memory.FILLS, ids=dirty_memory.FILL_IDS)
def test_poisoned_allocations_change_nothing(raw, fill):
    n = 2048
    clean = R.export_trainval(raw["records"], DEV, n, seed=11, choices=raw["choices"][n])
    with dirty_memory.poisoned(fill) as p:
        dirty = R.export_trainval(raw["records"], DEV, n, seed=11, choices=raw["choices"][n])
    assert p.count >= 1 and p.bytes >= sum(g["pc"].nbytes + g["rows"].nbytes for g in clean)  # every output's block
    same(dirty, clean, raw["names"], "on poisoned memory against fresh memory")
    same(dirty, raw["host"][n, "given"], raw["names"], "on poisoned memory")


def test_binding_allocates_only_through_the_replaced_names():
    used, bad = uninitialised_sites(inspect.getsource(R), inspect.getsourcefile(R))
    assert not bad, "\n".join(bad)
    assert used and used <= ALLOWED


def test_a_cloud_with_nan_is_refused_after_the_copy_back(raw):
    rec = dict(raw["records"][1])
    rec["points"] = rec["points"].copy()
    rec["points"][599, 5] = np.nan  # the last value of the scene: every raw row is looked at, kept or not
    rec["points"][0, 0] = -np.inf
    with pytest.raises(R.SceneError, match=r"NaN or Inf .*: 000003 \(2\)$"):
        R.export_trainval([raw["records"][0], rec, raw["records"][2]], DEV, 64)


def words(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def assert_same_batch(a, b, what):
    tensors = [k for k in a if torch.is_tensor(a[k])]
    assert sorted(tensors) == sorted(k for k in b if torch.is_tensor(b[k])) and len(tensors) >= 3, what
    for k in tensors:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert torch.equal(words(a[k]), words(b[k])), (what, k)


@pytest.mark.parametrize("color", [False, True])
def test_batches_from_raw_are_the_exported_folders(raw, tmp_path, color):
    names = list(SCENES)
    store = SUN.SunRgbdScenes.from_raw(raw["folder"], names, DEV, use_color=color, use_height=True, num_point=2048, seed=2)
    out = str(tmp_path / "exported")
    store.export(out)
    store.export_votes(out)
    cfg = V.sunrgbd_config()
    mine = SUN.SunRgbdLoader(store, cfg, 512, seed=7)
    for votes in ("boxes", "file"):
        back = SUN.SunRgbdLoader(SUN.SunRgbdScenes(out, names, DEV, use_color=color, use_height=True, votes=votes),
                                 cfg, 512, seed=7)
        what = "the %r store of the exported folder, colour %s" % (votes, color)
        a, b = mine.pretrain_batch([0, 1, 2, 3, 4, 5], counter=6), back.pretrain_batch([0, 1, 2, 3, 4, 5], counter=6)
        assert len([k for k in a if torch.is_tensor(a[k])]) >= 10 and a["point_clouds"].shape == (6, 512, 4 + 3 * color)
        assert_same_batch(a, b, "pretrain batch, " + what)
        assert_same_batch(mine.semi_batch([0, 2, 3], [1, 4, 5], counter=3), back.semi_batch([0, 2, 3], [1, 4, 5], counter=3),
                          "semi batch, " + what)
        assert_same_batch(mine.eval_batch([5, 4, 3, 2, 1, 0], counter=1), back.eval_batch([5, 4, 3, 2, 1, 0], counter=1),
                          "eval batch, " + what)
        assert np.array_equal(store.floor, back.scenes.floor) and store.floor.dtype == np.float64
    # and the store is the host path's, its vote rows included
    host = SUN.SunRgbdScenes.from_raw(raw["folder"], names, None, use_color=color, use_height=True, num_point=2048, seed=2)
    rows = store.vote_rows().cpu().numpy()
    assert rows.shape == (6 * 2048, 10) and rows[:, 0].sum() > 1000
    for s, x, y, off in zip(names, store.scenes, host.scenes, store.offset):
        assert_same_bits(x["cloud"], y["cloud"], s + " cloud")
        assert x["floor"] == y["floor"], s
        assert_same_bits(store.raw_export[s]["pc"], host.raw_export[s]["pc"], s + " pc")
        assert_same_bits(rows[off:off + 2048], SUN.compute_votes(y["cloud"], y["boxes"]), s + " vote_rows")


def test_scan_store_reads_a_mat_cloud(raw, tmp_path):
    points = raw["records"][0]["points"]
    R.write_mat(str(tmp_path / "cloud.mat"), points)
    np.savez(str(tmp_path / "cloud.npz"), pc=points)
    a = SC.ScanStore.from_files([str(tmp_path / "cloud.mat")], DEV, "sunrgbd")
    b = SC.ScanStore.from_files([str(tmp_path / "cloud.npz")], DEV, "sunrgbd")
    assert a.names == b.names == ["cloud"] and a.dataset == "sunrgbd"
    assert torch.equal(words(a.dev["cloud"]), words(b.dev["cloud"])) and np.array_equal(a.floor, b.floor)
    x = SC.ScanLoader(a, 1024, use_color=True, seed=1).batch([0], 3)
    y = SC.ScanLoader(b, 1024, use_color=True, seed=1).batch([0], 3)
    assert torch.equal(words(x["point_clouds"]), words(y["point_clouds"]))


@pytest.mark.parametrize("stage,scans,batch,steps", [("pretrain", "6", "2", 2), ("semi", "8", "2,2", 1)])
def test_train_front_end_runs_an_epoch_on_sunrgbd(tmp_path, stage, scans, batch, steps):
    tool = runpy.run_path(os.path.join(ROOT, "tools", "train.py"))
    log_dir = str(tmp_path / "log")
    trainer = tool["main"](["--dataset", "sunrgbd", "--stage", stage, "--synthetic", scans, "--num_point", "3000",
                            "--num_target", "64", "--batch_size", batch, "--max_epoch", "1", "--print_interval", "1",
                            "--log_dir", log_dir, "--seed", "3"])
    torch.cuda.synchronize()
    assert trainer.runner.global_step == steps
    with open(os.path.join(log_dir, "log_train.txt")) as f:
        lines = f.read().splitlines()
    assert any("dataset='sunrgbd'" in l for l in lines)
    losses = [float(l.split(": ")[1]) for l in lines if l.startswith("mean loss: ")]
    assert len(losses) == steps and all(np.isfinite(x) and x > 0 for x in losses), losses
    assert not any(l.startswith("skipped steps") for l in lines)
    ckpt = torch.load(os.path.join(log_dir, "checkpoint.tar"), weights_only=False)
    keys = ["epoch", "loss", "model_state_dict", "optimizer_state_dict"] + (["ema_model_state_dict"] if stage == "semi" else [])
    assert sorted(ckpt) == sorted(keys) and ckpt["epoch"] == 1
    assert all(bool(torch.isfinite(v).all()) for v in ckpt["model_state_dict"].values() if v.is_floating_point())
