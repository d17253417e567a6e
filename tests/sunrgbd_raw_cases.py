"""What the raw SUN RGB-D tests share (test_sunrgbd_raw.py on the CPU, test_sunrgbd_raw_gpu.py on the
MI355X): the golden of tests/golden/make_sunrgbd_raw_golden.py written back to disk as the
`sunrgbd_trainval/` folder it was made from, and comparisons bit for bit.  A plain module, no fixture."""
import importlib
import os

import numpy as np

from conftest import golden, load_pkg

load_pkg()
R = importlib.import_module("3dioumatch_amd.votenet.sunrgbd_raw")

SCENES = ("000001", "000002", "000003", "000004", "000005", "000006")
FLOAT32 = ("000001", "000003", "000005")
KEPT = (2048, 1977)  # the virtual index 0.0099 (n - 1) has the fraction .27 and .56: one lerp branch each
KEYS = ("pc", "bbox", "floor", "rows")
_GOLDEN = None


def ref():
    global _GOLDEN
    if _GOLDEN is None:
        with golden("sunrgbd_raw_ref.npz") as f:
            _GOLDEN = {k: f[k] for k in f.files}
    return _GOLDEN


def num_point(name):
    return int(ref()["%s_num_point" % name])


def materialise(root, compress=True):
    """The golden's scenes as root/sunrgbd_trainval (depth/ by write_mat, label_v1/, the two index
    lists: the odd scenes train, the even ones val) -> the folder."""
    g = ref()
    folder = os.path.join(str(root), "sunrgbd_trainval")
    for sub in ("depth", "label_v1"):
        os.makedirs(os.path.join(folder, sub))
    for name in SCENES:
        R.write_mat(os.path.join(folder, "depth", name + ".mat"), g[name + "_raw"], compress=compress)
        g[name + "_label"].tofile(os.path.join(folder, "label_v1", name + ".txt"))
    for split, part in (("train", SCENES[0::2]), ("val", SCENES[1::2])):
        with open(os.path.join(folder, split + "_data_idx.txt"), "w") as f:
            f.write("".join("%d\n" % int(s) for s in part))
    return folder


def records(folder, names=SCENES):
    return [R.read_trainval_scene(folder, s) for s in names]


def extra_record(name="000099", n=2500, dtype=np.float64, seed=3):
    """A cloud of distinct, full-mantissa values with more points than either kept count: the distinct
    draw and, in float64, two different order statistics."""
    g = np.random.default_rng(seed)
    points = np.concatenate([g.normal(size=(n, 3)), g.random((n, 3))], 1).astype(dtype)
    return {"name": name, "points": points, "boxes": np.zeros((0, 8))}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def assert_same_bits(got, want, what=""):
    g, w = np.asarray(got), np.asarray(want)
    assert g.dtype == w.dtype, (what, g.dtype, w.dtype)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    differ = int((bits(g) != bits(w)).sum())
    assert differ == 0, "%s: %d of %d words differ" % (what, differ, g.size)


def assert_same_export(got, want, what=""):
    """Two exports of one scene: floors with == (a zero's sign is np.percentile's to choose), every
    other array bit for bit."""
    assert sorted(got) == sorted(KEYS) and sorted(want) == sorted(KEYS), what
    for k in ("pc", "bbox", "rows"):
        assert_same_bits(got[k], want[k], "%s %s" % (what, k))
    assert np.asarray(got["floor"]).dtype == np.asarray(want["floor"]).dtype == got["pc"].dtype, what
    assert got["floor"] == want["floor"], "%s floor: %r != %r" % (what, got["floor"], want["floor"])
