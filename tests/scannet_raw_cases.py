"""What the raw-ScanNet tests share (test_scannet_raw.py on the CPU, test_scannet_raw_gpu.py on the
MI355X): the golden of tests/golden/make_scannet_raw_golden.py written back to disk as the raw scan
folders it was made from, and comparisons bit for bit.  A plain module, no fixture."""
import importlib
import os

import numpy as np

from conftest import golden, load_pkg

load_pkg()
R = importlib.import_module("3dioumatch_amd.votenet.scannet_raw")

SCANS = ("sceneA", "sceneB", "sceneC", "sceneD", "sceneE")
KEYS = ("vert", "ins_label", "sem_label", "bbox")
DTYPES = {"vert": np.float32, "ins_label": np.uint32, "sem_label": np.uint32, "bbox": np.float64}
_GOLDEN = None


def ref():
    global _GOLDEN
    if _GOLDEN is None:
        with golden("scannet_raw_ref.npz") as f:
            _GOLDEN = {k: f[k] for k in f.files}
    return _GOLDEN


def materialise(root):
    """The golden's raw files under root/scans/<scan>/ and its label tsv -> (scans dir, tsv path)."""
    g = ref()
    scans = os.path.join(str(root), "scans")
    for name in SCANS:
        os.makedirs(os.path.join(scans, name))
        for k, suffix in R.SUFFIXES.items():
            g["%s_file_%s" % (name, k)].tofile(os.path.join(scans, name, name + suffix))
    tsv = os.path.join(str(root), "labels.tsv")
    g["label_map_tsv"].tofile(tsv)
    return scans, tsv


def max_points(name):
    return int(ref()["%s_max_points" % name])


def reference_export(name):
    """load_scannet_data.export's vertices and labels with export_one_scan's (filtered) boxes: what
    export_one_scan saves for a scan it does not subsample."""
    g = ref()
    out = {k: g["%s_export_%s" % (name, k)] for k in KEYS[:3]}
    out["bbox"] = g["%s_one_bbox" % name]
    return out


def reference_one_scan(name):
    """export_one_scan's own output (sceneE: subsampled by the recorded choice)."""
    g = ref()
    if "%s_choice" % name not in g:
        return reference_export(name)
    return {k: g["%s_one_%s" % (name, k)] for k in KEYS}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def assert_same_export(got, want, what=""):
    assert sorted(got) == sorted(KEYS), what
    for k in KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == DTYPES[k] and w.dtype == DTYPES[k], (what, k, g.dtype, w.dtype)
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        differ = int((bits(g) != bits(w)).sum())
        assert differ == 0, "%s %s: %d of %d words differ" % (what, k, differ, g.size)
