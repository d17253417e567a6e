"""CPU tests of semi-supervised batches whose unlabeled rows come from a label-free ScanStore
(SceneLoader(unlabeled_scans=...)): the host batch against the labeled loader that holds the same scans
with their labels, bit for bit; the labeled rows' independence of the store; what is refused, by the
loader and by scene_scan_semi_build; epoch planning over the store; the flag of tools/train.py."""
import ctypes
import importlib
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT, load_pkg

load_pkg()
L = importlib.import_module("3dioumatch_amd._lib")
R = importlib.import_module("3dioumatch_amd.records")
SL = importlib.import_module("3dioumatch_amd.votenet.scene_loader")
SC = importlib.import_module("3dioumatch_amd.votenet.scan_data")
SD = importlib.import_module("3dioumatch_amd.votenet.scannet_data")
SU = importlib.import_module("3dioumatch_amd.votenet.sunrgbd_data")
T = importlib.import_module("3dioumatch_amd.votenet.trainer")
V = importlib.import_module("3dioumatch_amd.votenet")

N = 2500                      # two chunks of 2048 slots, the second partial
COUNTS = (1500, 2500, 5000)   # the unlabeled scans: n < N (with replacement), n == N, n > N
LAB_COUNTS = (2000, 3000)     # the labeled scans
COMBOS = [(False, True), (True, True), (True, False)]  # (use_color, use_height)
SPLITS = [(1, 1), (2, 3), (1, 63)]
INVALID = 1  # hipErrorInvalidValue


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def same(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(bits(g), bits(w)), k


class Data(object):
    """float32 scans on disk: LAB_COUNTS labeled, COUNTS unlabeled (written WITH labels, so that the
    labeled store can hold them too; ScanStore.from_files reads their clouds alone)."""

    def __init__(self, dataset, d):
        self.dataset, self.dir = dataset, d
        self.M = SD if dataset == "scannet" else SU
        fmt = "scene%04d_00" if dataset == "scannet" else "%06d"
        self.lab = [fmt % (i + 1) for i in range(len(LAB_COUNTS))]
        self.unl = [fmt % (i + 11) for i in range(len(COUNTS))]
        for i, (name, n) in enumerate(zip(self.lab + self.unl, LAB_COUNTS + COUNTS)):
            if dataset == "scannet":
                SD.write_synthetic_scans(d, [name], num_points=n, instances=5, boxes=3, seed=40 + i)
            else:
                SU.write_synthetic_scans(d, [name], num_points=n, boxes=3, seed=60 + i, dtype=np.float32)
        self.config = V.scannet_config() if dataset == "scannet" else V.sunrgbd_config()

    def files(self):
        return [os.path.join(self.dir, s + ("_vert.npy" if self.dataset == "scannet" else "_pc.npz"))
                for s in self.unl]

    def scenes(self, names, color, height, device=None):
        cls = SD.ScanNetScenes if self.dataset == "scannet" else SU.SunRgbdScenes
        return cls(self.dir, names, device, use_color=color, use_height=height)

    def loader(self, scenes, seed, **kw):
        cls = SD.ScanNetLoader if self.dataset == "scannet" else SU.SunRgbdLoader
        return cls(scenes, self.config, N, seed=seed, **kw)

    def pair(self, color, height, seed=5, device=None):
        """(the labeled loader over all five scans, the mixed loader: two labeled scans + the store)"""
        both = self.loader(self.scenes(self.lab + self.unl, color, height, device), seed,
                           labeled=self.lab, unlabeled=self.unl)
        store = SC.ScanStore.from_files(self.files(), device, self.dataset)
        mixed = self.loader(self.scenes(self.lab, color, height, device), seed, unlabeled_scans=store)
        return both, mixed


@pytest.fixture(scope="module", params=["scannet", "sunrgbd"])
def data(request, tmp_path_factory):
    return Data(request.param, str(tmp_path_factory.mktemp(request.param + "_semi_scans")))


def split_ids(nl, nu):
    return np.arange(nl) % len(LAB_COUNTS), (np.arange(nu) + 1) % len(COUNTS)


def explicit_draws(dataset, lab, unl, seed):
    g = np.random.default_rng(seed)
    counts = [LAB_COUNTS[i] for i in lab] + [COUNTS[i] for i in unl]
    return {"idx": np.stack([g.integers(0, n, N) for n in counts]),
            "ema_idx": np.stack([g.integers(0, n, N) for n in counts]),
            "u": g.random((len(counts), SC.UNIFORMS[dataset]))}


# ------------------------------------------------------------------ host parity
@pytest.mark.parametrize("color,height", COMBOS)
def test_host_batch_is_the_labeled_loaders(data, color, height):
    both, mixed = data.pair(color, height)
    assert mixed.unlabeled.tolist() == [0, 1, 2] and mixed.unlabeled_scans.names == data.unl
    for (nl, nu), counter in zip(SPLITS, (0, 3, 70000)):
        lab, unl = split_ids(nl, nu)
        want = both.host_batch("semi", lab, unl, counter)
        got = mixed.host_batch("semi", lab, unl, counter)
        same(got, want)
        C = 3 + 3 * color + height
        assert got["point_clouds"].shape == (nl + nu, N, C) and got["vote_label"].shape == (nl, N, 9)
        assert got["supervised_mask"].tolist() == [1] * nl + [0] * nu
        assert got["scan_idx"][nl:].tolist() == unl.tolist()
        same(mixed.host_draws("semi", lab, unl, counter), both.host_draws("semi", lab, unl, counter))
    flips = mixed.host_batch("semi", [0], np.arange(63) % 3, 70000)
    assert 0 < flips["flip_x_axis"].sum() < 64  # the augmentation is at work
    if data.dataset == "sunrgbd":
        assert not flips["flip_y_axis"].any()


@pytest.mark.parametrize("color,height", COMBOS)
def test_host_batch_with_explicit_draws(data, color, height):
    both, mixed = data.pair(color, height)
    for nl, nu in SPLITS[:2]:
        lab, unl = split_ids(nl, nu)
        draws = explicit_draws(data.dataset, lab, unl, 100 + nu)
        got = mixed.host_batch("semi", lab, unl, 9, draws=draws)
        same(got, both.host_batch("semi", lab, unl, 9, draws=draws))
        # the teacher's sample is the raw row: x, y, z of the drawn points
        store = mixed.unlabeled_scans
        for r, s in enumerate(unl):
            assert np.array_equal(got["ema_point_clouds"][nl + r, :, 0:3], store.clouds[s][draws["ema_idx"][nl + r], 0:3])
    lab, unl = split_ids(1, 2)
    bad = explicit_draws(data.dataset, lab, unl, 1)
    bad["idx"][2, 7] = COUNTS[unl[1]]
    with pytest.raises(ValueError, match="out of range"):
        mixed.host_batch("semi", lab, unl, 0, draws=bad)


def test_host_semi_rows_alone(data):
    both, mixed = data.pair(True, True, seed=8)
    rows = mixed._scan_rows
    assert isinstance(rows, SC.ScanLoader)
    for row0 in (1, 2, 61):
        lab, unl = split_ids(row0, 3)
        want = both.host_batch("semi", lab, unl, 4)
        got = rows.host_semi_rows(unl, counter=4, row0=row0)
        assert sorted(got) == sorted(rows._SEMI_KEYS)
        same(got, {k: want[k][row0:] for k in got})
    with pytest.raises(ValueError, match="row0"):
        rows.host_semi_rows([0, 1], row0=63)
    with pytest.raises(ValueError, match="row0"):
        rows.host_semi_rows([0], row0=-1)


# ------------------------------------------------------------------ the labeled rows and the store
def test_labeled_rows_never_reach_the_store(data):
    _, mixed = data.pair(True, True)
    other = SC.ScanStore(SC.synthetic_clouds(4, 3000, seed=3, dataset=data.dataset), None, data.dataset)
    mixed2 = data.loader(mixed.scenes, 5, unlabeled_scans=other)
    assert mixed2.unlabeled.tolist() == [0, 1, 2, 3]
    a = mixed.host_batch("semi", [0, 1], [0, 1, 2], 6)
    b = mixed2.host_batch("semi", [0, 1], [0, 1, 2], 6)
    for k in a:
        rows = 2 if a[k].shape[0] == 5 else a[k].shape[0]
        assert np.array_equal(bits(a[k][:rows]), bits(b[k][:rows])), k
    assert not np.array_equal(a["point_clouds"][2:], b["point_clouds"][2:])
    # pretrain and eval batches do not know the store
    plain = data.loader(mixed.scenes, 5)
    same(mixed.host_batch("pretrain", [0, 1], counter=2), plain.host_batch("pretrain", [0, 1], counter=2))
    same(mixed.host_batch("eval", [1], counter=2), plain.host_batch("eval", [1], counter=2))


# ------------------------------------------------------------------ refusals
def test_the_loader_refuses_what_a_store_cannot_give(data):
    _, mixed = data.pair(True, True)
    with pytest.raises(ValueError, match="no labels"):
        mixed.host_batch("semi", [0], [1], unlabeled_labels=True)
    with pytest.raises(ValueError, match="no labels"):
        mixed._layout("semi", 1, 1, True)
    with pytest.raises(ValueError, match="labeled row"):
        mixed.host_batch("semi", [], [1, 2])
    with pytest.raises(ValueError, match="labeled row"):
        mixed._layout("semi", 0, 2)
    with pytest.raises(ValueError, match="1..64"):
        mixed.host_batch("semi", [0, 1], np.arange(63) % 3)
    wrong = "sunrgbd" if data.dataset == "scannet" else "scannet"
    clouds = SC.synthetic_clouds(2, 100, seed=1, dataset=data.dataset)
    with pytest.raises(ValueError, match="loader"):
        data.loader(mixed.scenes, 0, unlabeled_scans=SC.ScanStore(clouds, None, wrong))
    with pytest.raises(ValueError, match="3-column"):
        data.loader(mixed.scenes, 0, unlabeled_scans=SC.ScanStore([c[:, :3] for c in clouds], None, data.dataset))
    with pytest.raises(ValueError, match="not both"):
        data.loader(mixed.scenes, 0, unlabeled=data.lab, unlabeled_scans=mixed.unlabeled_scans)
    # a 3-column store serves scenes without colour
    xyz = data.loader(data.scenes(data.lab, False, True), 0,
                      unlabeled_scans=SC.ScanStore([c[:, :3] for c in clouds], None, data.dataset))
    assert xyz.host_batch("semi", [0], [1, 0])["point_clouds"].shape == (3, N, 4)
    with pytest.raises(RuntimeError, match="no device copy"):
        mixed.build("semi", [0], [1])


def _valid_args():
    a = R.ScanSemiArgs()
    a.B, a.N, a.C, a.use_color, a.use_height, a.dataset, a.row0 = 2, 16, 6, 1, 1, 0, 1
    for name, kind in R.ScanSemiArgs._fields_:
        if kind is ctypes.c_void_p and name not in ("idx_in", "ema_idx_in", "u_in"):
            setattr(a, name, 0x1000)  # never dereferenced: every call below is refused before a launch
    return a


REQUIRED = ("cloud", "offset", "count", "floor", "point_clouds", "ema_point_clouds", "flip_x_axis",
            "flip_y_axis", "rot_angle", "rot_mat", "scale", "supervised_mask", "scan_idx_out")


@pytest.mark.parametrize("field,value", [
    ("B", 0), ("B", -1), ("B", 65), ("row0", -1), ("row0", 63), ("N", 0), ("C", 4), ("C", 7), ("C", 0),
    ("C", 3),  # use_color with 3 columns
    ("dataset", 2), ("dataset", -1)] + [(k, None) for k in REQUIRED])
def test_the_entry_refuses_bad_arguments_without_a_launch(field, value):
    a = _valid_args()
    setattr(a, field, value)
    assert L.lib.scene_scan_semi_build(ctypes.byref(a), None) == INVALID


def test_the_entry_refuses_a_null_record_and_is_no_drop_in_export():
    assert L.lib.scene_scan_semi_build(None, None) == INVALID
    assert "scene_scan_semi_build" in L._LOADER_SIGNATURES and "scene_scan_semi_build" not in L.EXPORTS
    assert ctypes.sizeof(R.ScanSemiArgs) == 4 * 9 + 2 * 4 * 64 + 4 + 8 * 16  # scan_hip.h ScanSemiArgs, padded


# ------------------------------------------------------------------ planning
def test_loader_epochs_plans_over_the_store(data, monkeypatch):
    _, mixed = data.pair(False, True)
    assert len(mixed.labeled) == 2 and len(mixed.unlabeled) == 3
    monkeypatch.setattr(SL, "feed", lambda runner, loader, plan, kind, unlabeled_labels: list(plan))
    epoch_batches = T.loader_epochs(None, mixed, "semi", 1, 3, seed=2)
    for epoch in range(3):
        plan = epoch_batches(epoch)
        assert len(plan) == 2
        for counter, lab, unl in plan:
            assert sorted(unl.tolist()) == [0, 1, 2] and len(lab) == 1
    with pytest.raises(ValueError, match="fewer unlabeled"):
        T.loader_epochs(None, mixed, "semi", 1, 4)(0)


# ------------------------------------------------------------------ tools/train.py
def _tool():
    spec = importlib.util.spec_from_file_location("tools_train", os.path.join(ROOT, "tools", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_tool_lists_the_flag_and_refuses_its_misuse(capsys):
    tool = _tool()
    with pytest.raises(SystemExit) as e:
        tool.main(["--help"])
    assert e.value.code == 0
    assert "--unlabeled_scans" in capsys.readouterr().out
    with pytest.raises(SystemExit) as e:
        tool.main(["--stage", "semi", "--unlabeled_scans", "captures", "--view_stats"])
    assert "--view_stats" in str(e.value) and "labels" in str(e.value)
    with pytest.raises(SystemExit) as e:
        tool.main(["--stage", "pretrain", "--unlabeled_scans", "captures"])
    assert "pretrain" in str(e.value)
    with pytest.raises(SystemExit) as e:
        tool.main(["--stage", "semi", "--unlabeled_scans", "synthetic"])
    assert "--synthetic N" in str(e.value)
