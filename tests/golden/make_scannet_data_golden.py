"""Regenerate tests/golden/scannet_data_ref.npz with the REFERENCE's own ScanNet datasets (build
container only):

    python tests/golden/make_scannet_data_golden.py

A few small seeded scenes are written in the reference's on-disk layout (`<scan>_vert.npy` float32
xyz+rgb, `_ins_label.npy` / `_sem_label.npy` uint32, `_bbox.npy` (nb, 7) float64 with the nyu40 id
last) and run through scannet/scannet_ssl_dataset.py's ScannetSSLLabeledDataset and
ScannetSSLUnlabeledDataset (load_labels on and off) and scannet/scannet_detection_dataset.py's
ScannetDetectionDataset (train with augment, val without).  The datasets are built with __new__
(their __init__ reads fixed paths of the reference tree); every np.random.choice / np.random.random
they make is recorded by wrapping it in numpy.random; the imports the reference's utilities pull in
but the loader path never calls (plyfile, trimesh, matplotlib) are stubbed and torch.Tensor.cuda is
the identity.  ScannetDetectionDataset with use_color=True raises NameError in the reference
(pcl_color), so colour is covered through the SSL classes.

The scenes cover: n < N (sampling with replacement), an instance with mixed semantic labels,
instance 0 carrying a nyu40 id, a scene without a box and one with exactly 64.
Only data is stored: the scenes, the reference's mean sizes, the draws and the outputs.
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
NUM_POINTS = 256
NYU = [3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39]
SCENES = ["scene0000_00", "scene0001_00", "scene0002_00", "scene0003_00"]
# variant -> (dataset, use_color, extra)
VARIANTS = {
    "lab": ("ssl_labeled", True, {}),
    "unl": ("ssl_unlabeled", False, {"load_labels": True}),
    "unl_nolab": ("ssl_unlabeled", True, {"load_labels": False}),
    "det_train": ("detection", False, {"augment": True}),
    "det_val": ("detection", False, {"augment": False}),
}
OUT_KEYS = ["point_clouds", "ema_point_clouds", "center_label", "heading_class_label",
            "heading_residual_label", "size_class_label", "size_residual_label", "sem_cls_label",
            "box_label_mask", "vote_label", "vote_label_mask", "flip_x_axis", "flip_y_axis", "rot_mat",
            "rot_angle", "scale"]


def make_scene(g, n, n_inst, n_box, mixed=True):
    xyz = (g.random((n, 3)) * [6.0, 5.0, 3.0] - [3.0, 2.5, 0.2]).astype(np.float32)
    rgb = g.integers(0, 256, (n, 3)).astype(np.float32)
    inst = g.integers(0, n_inst, n).astype(np.uint32) * 3  # sparse ids: the store remaps them densely
    sem = np.zeros(n, np.uint32)
    pool = NYU + [1, 2, 13, 40]  # some non-nyu40 semantic labels too
    for k, iid in enumerate(np.unique(inst)):
        sem[inst == iid] = pool[int(g.integers(0, len(pool)))]
    sem[inst == 0] = 3  # instance 0 carries a nyu40 id
    if mixed:  # an instance with mixed semantic labels
        iid = np.unique(inst)[1]
        where = np.where(inst == iid)[0]
        sem[where[::2]] = 1
        sem[where[1::2]] = 7
    box = np.zeros((n_box, 7))
    box[:, 0:3] = g.random((n_box, 3)) * [6.0, 5.0, 2.0] - [3.0, 2.5, 0.0]
    box[:, 3:6] = g.random((n_box, 3)) * 1.5 + 0.1
    box[:, 6] = np.array(NYU)[g.integers(0, 18, n_box)]
    return np.concatenate([xyz, rgb], 1), inst, sem, box


def main():
    for name in ("plyfile", "trimesh", "matplotlib", "matplotlib.pyplot"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["plyfile"].PlyData = sys.modules["plyfile"].PlyElement = object
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    sys.modules["matplotlib.pyplot"].cm = types.SimpleNamespace(jet=None)  # a default argument
    torch.Tensor.cuda = lambda self, *a, **k: self
    for p in (REF, os.path.join(REF, "utils"), os.path.join(REF, "scannet")):
        sys.path.insert(0, p)
    import scannet.scannet_ssl_dataset as ssl  # noqa: E402
    import scannet_detection_dataset as det  # noqa: E402

    record = []
    real_choice, real_random = np.random.choice, np.random.random

    def choice(*a, **k):
        r = real_choice(*a, **k)
        record.append(("choice", np.asarray(r)))
        return r

    def random(*a, **k):
        r = real_random(*a, **k)
        record.append(("random", r))
        return r

    np.random.choice, np.random.random = choice, random

    g = np.random.default_rng(2024)
    specs = [(400, 7, 10), (180, 4, 0), (300, 5, 64), (520, 20, 25)]  # (n, instances, boxes)
    out = {"num_points": np.int64(NUM_POINTS), "scan_names": np.array(SCENES),
           "mean_size": ssl.DC.mean_size_arr.astype(np.float64)}
    with tempfile.TemporaryDirectory() as tmp:
        for s, (n, ni, nb) in zip(SCENES, specs):
            vert, inst, sem, box = make_scene(g, n, ni, nb)
            for k, v in (("vert", vert), ("ins_label", inst), ("sem_label", sem), ("bbox", box)):
                np.save(os.path.join(tmp, "%s_%s.npy" % (s, k)), v)
                out["%s_%s" % (s, k)] = v
        for vname, (kind, use_color, extra) in VARIANTS.items():
            if kind == "ssl_labeled":
                ds = ssl.ScannetSSLLabeledDataset.__new__(ssl.ScannetSSLLabeledDataset)
                ds.augment = True
            elif kind == "ssl_unlabeled":
                ds = ssl.ScannetSSLUnlabeledDataset.__new__(ssl.ScannetSSLUnlabeledDataset)
                ds.augment, ds.load_labels = True, extra["load_labels"]
            else:
                ds = det.ScannetDetectionDataset.__new__(det.ScannetDetectionDataset)
                ds.augment, ds.remove_obj = extra["augment"], False
            ds.data_path, ds.scan_names, ds.num_points = tmp, list(SCENES), NUM_POINTS
            ds.use_color, ds.use_height = use_color, True
            for i, s in enumerate(SCENES):
                np.random.seed(1000 + 17 * i + len(vname))
                del record[:]
                r = ds[i]
                choices = [v for k, v in record if k == "choice"]
                unis = np.array([v for k, v in record if k == "random"], np.float64)
                if kind == "ssl_labeled":
                    idx, ema = choices
                elif kind == "ssl_unlabeled":
                    ema, idx = choices
                else:
                    idx, ema = choices[0], None
                pre = "%s_%s_" % (vname, s)
                out[pre + "draw_idx"] = idx.astype(np.int32)
                if ema is not None:
                    out[pre + "draw_ema"] = ema.astype(np.int32)
                if unis.size:
                    out[pre + "draw_u"] = unis
                for k in OUT_KEYS:
                    if k in r:
                        v = np.asarray(r[k])
                        if k == "vote_label":
                            v = v[:, 0:3]  # tiled x3: one copy is enough
                        if k == "vote_label_mask":
                            v = v.astype(np.int8)
                        out[pre + k] = v
    np.random.choice, np.random.random = real_choice, real_random
    path = os.path.join(HERE, "scannet_data_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
