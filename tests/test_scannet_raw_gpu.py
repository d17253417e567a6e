"""Raw ScanNet scans -> the preprocessed layout on the MI355X: scannet_raw_export (csrc/scannet_raw.hip)
against the numpy restatement bit for bit at the golden's shapes, in one chunk (workgroups straddle scan
boundaries) and one scan per call; twice; on poisoned allocations; the from_raw store's batch against the
batch of the store read back from the exported folder; a .ply cloud in the label-free scan store."""
import importlib
import inspect

import numpy as np
import pytest
import torch

import dirty_memory
from scannet_raw_cases import R, SCANS, assert_same_export, materialise, max_points, ref
from test_dirty_memory import ALLOWED, uninitialised_sites

SD = importlib.import_module("3dioumatch_amd.votenet.scannet_data")
SC = importlib.import_module("3dioumatch_amd.votenet.scan_data")
V = importlib.import_module("3dioumatch_amd.votenet")

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N = 2048  # sceneE's MAX_NUM_POINT; sceneB (3001) is subsampled by it too


@pytest.fixture(scope="module")
def raw(tmp_path_factory):
    scans, tsv = materialise(tmp_path_factory.mktemp("scannet_raw_gpu"))
    label_map = R.read_label_map(tsv)
    records = [R.read_raw_scan(scans, s, label_map) for s in SCANS]
    choices = {"sceneE": ref()["sceneE_choice"]}
    # the restatement, computed once: B by the project's draw (row 1), E by the recorded choice
    host = R.export_raw_scans(records, None, N, seed=11, choices=choices)
    return {"scans": scans, "tsv": tsv, "records": records, "choices": choices, "host": host}


def test_one_chunk_equals_the_restatement(raw):
    assert max_points("sceneE") == N
    got = R.export_raw_scans(raw["records"], DEV, N, seed=11, choices=raw["choices"])
    assert [g["vert"].shape[0] for g in got] == [1000, N, 1400, 1, N]
    assert [g["bbox"].shape[0] for g in got] == [10, 8, 64, 0, 8]
    for s, g, w in zip(SCANS, got, raw["host"]):
        assert_same_export(g, w, s)
    # no subsampling, and both subsampled scans by the device's own draw
    for n, choices in ((50000, None), (N, None)):
        got = R.export_raw_scans(raw["records"], DEV, n, seed=3, choices=choices)
        want = R.export_raw_scans(raw["records"], None, n, seed=3, choices=choices)
        for s, g, w in zip(SCANS, got, want):
            assert_same_export(g, w, "%s at max_points %d" % (s, n))


def test_one_scan_per_call_equals_the_restatement(raw):
    for index, (s, rec, w) in enumerate(zip(SCANS, raw["records"], raw["host"])):
        [g] = R.export_raw_scans([rec], DEV, N, seed=11, choices=raw["choices"], first_index=index)
        assert_same_export(g, w, s)
    # chunks of two scans at most: the chunk bound splits the list, the draws keep their rows
    got = R.export_raw_scans(raw["records"], DEV, N, seed=11, choices=raw["choices"], chunk_points=4500)
    for s, g, w in zip(SCANS, got, raw["host"]):
        assert_same_export(g, w, s)


def test_twice_is_bit_equal(raw):
    a = R.export_raw_scans(raw["records"], DEV, N, seed=5)
    b = R.export_raw_scans(raw["records"], DEV, N, seed=5)
    for s, x, y in zip(SCANS, a, b):
        assert_same_export(x, y, s)


@pytest.mark.parametrize("fill", dirty_memory.FILLS, ids=dirty_memory.FILL_IDS)
def test_poisoned_allocations_change_nothing(raw, fill):
    clean = R.export_raw_scans(raw["records"], DEV, N, seed=11, choices=raw["choices"])
    with dirty_memory.poisoned(fill) as p:
        dirty = R.export_raw_scans(raw["records"], DEV, N, seed=11, choices=raw["choices"])
    assert p.count >= 1 and p.bytes >= sum(g["vert"].nbytes for g in clean)  # the block of every output
    for s, x, y, w in zip(SCANS, dirty, clean, raw["host"]):
        assert_same_export(x, y, s)
        assert_same_export(x, w, s)


def test_binding_allocates_only_through_the_replaced_names():
    used, bad = uninitialised_sites(inspect.getsource(R), inspect.getsourcefile(R))
    assert not bad, "\n".join(bad)
    assert used and used <= ALLOWED


def test_an_overfull_scan_is_refused_after_the_copy_back(raw):
    rec = dict(raw["records"][2])
    groups = [(o, "chair" if o == 5 else label, s) for o, label, s in rec["groups"]]
    rec["seg_label"], rec["seg_object"], rec["object_label"] = R.seg_tables(
        "sceneC", rec["seg"], groups, R.read_label_map(raw["tsv"]))
    with pytest.raises(R.SceneError, match="sceneC: 65 boxes, at most MAX_NUM_OBJ = 64"):
        R.export_raw_scans([raw["records"][0], rec], DEV)


def words(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("color,height", [(False, True), (True, True)])
def test_pretrain_batch_from_raw_is_the_exported_folders(raw, tmp_path, color, height):
    names = list(SCANS)
    store = SD.ScanNetScenes.from_raw(raw["scans"], names, raw["tsv"], DEV, use_color=color, use_height=height,
                                      max_points=N, seed=2)
    out = str(tmp_path / "exported")
    store.export(out)
    back = SD.ScanNetScenes(out, names, DEV, use_color=color, use_height=height)
    cfg = V.scannet_config()
    a = SD.ScanNetLoader(store, cfg, 512, seed=7).pretrain_batch([0, 1, 2, 3, 4], counter=6)
    b = SD.ScanNetLoader(back, cfg, 512, seed=7).pretrain_batch([0, 1, 2, 3, 4], counter=6)
    tensors = [k for k in a if torch.is_tensor(a[k])]
    assert sorted(tensors) == sorted(k for k in b if torch.is_tensor(b[k])) and len(tensors) >= 10
    for k in tensors:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert torch.equal(words(a[k]), words(b[k])), k
    assert a["point_clouds"].shape == (5, 512, 3 + 3 * color + height)
    # and the store is the host path's
    host = SD.ScanNetScenes.from_raw(raw["scans"], names, raw["tsv"], None, use_color=color, use_height=height,
                                     max_points=N, seed=2)
    for s in names:
        assert_same_export(store.raw_export[s], host.raw_export[s], s)


def test_scan_store_reads_a_ply_cloud(raw, tmp_path):
    vert = raw["records"][1]["vert"]
    R.write_ply(str(tmp_path / "cloud.ply"), vert, binary=True)
    np.save(str(tmp_path / "cloud.npy"), vert)
    a = SC.ScanStore.from_files([str(tmp_path / "cloud.ply")], DEV)
    b = SC.ScanStore.from_files([str(tmp_path / "cloud.npy")], DEV)
    assert torch.equal(words(a.dev["cloud"]), words(b.dev["cloud"])) and np.array_equal(a.floor, b.floor)
    x = SC.ScanLoader(a, 1024, use_color=True, seed=1).batch([0], 3)
    y = SC.ScanLoader(b, 1024, use_color=True, seed=1).batch([0], 3)
    assert torch.equal(words(x["point_clouds"]), words(y["point_clouds"]))
