"""Regenerate tests/golden/sunrgbd_votes_ref.npz with the REFERENCE's own vote extraction (build
container only; needs scipy, whose Delaunay hull the reference calls):

    python tests/golden/make_sunrgbd_votes_golden.py <path of the reference tree>

Five small seeded scenes are served to sunrgbd/sunrgbd_data.py:extract_sunrgbd_data(save_votes=True)
by a stand-in for its `sunrgbd_object` (get_label_objects: objects with classname, centroid, l, w,
h, heading_angle; get_depth: the cloud), pc_util.random_sampling is the identity, and the imports
the path never calls (cv2, mayavi, plyfile, trimesh, matplotlib) are stubbed.  What the reference
writes into its output folder -- `<id>_pc.npz`, `<id>_bbox.npy`, `<id>_votes.npz` -- is the fixture.

The scenes: 9 boxes / float32, 0 boxes / float64 (so skip_empty_scene is off), 64 boxes / float32,
12 boxes / float64, 5 boxes / float32 one of which has zero height, with points placed exactly in
its plane.  In the 9- and the 12-box scene four boxes share nearly one centre, so that some points
lie in four or more boxes (asserted below, from the analytic membership in float64; the count is
stored as `<id>_hits`).  No point lies within 1e-5 of a face of a box with a volume (asserted
below: move SEED0 if it fails), so the reference's hull test and the analytic test cannot differ
on any point and no point is left out of any comparison.  Only data is stored.
"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEED0 = 5100
SCENES = ["000001", "000002", "000003", "000004", "000005"]
# (points, boxes, cloud dtype, four boxes around one centre, box 2 has zero height)
SPECS = [(410, 9, np.float32, True, False), (380, 0, np.float64, False, False),
         (400, 64, np.float32, False, False), (390, 12, np.float64, True, False),
         (400, 5, np.float32, False, True)]
CLASSES = ['bed', 'table', 'sofa', 'chair', 'toilet', 'desk', 'dresser', 'night_stand', 'bookshelf', 'bathtub']
FLAT_Z = 0.25  # exact in float32: the plane of the zero-height box


def make_scene(g, n, nb, dtype, cluster, flat):
    box = np.zeros((nb, 8))
    box[:, 0:3] = g.random((nb, 3)) * [5.0, 4.0, 1.5] + [-2.5, 1.0, -1.0]
    box[:, 3:6] = g.random((nb, 3)) * 0.6 + 0.15
    box[:, 6] = g.random(nb) * 2 * np.pi - np.pi
    box[:, 7] = g.integers(0, len(CLASSES), nb)
    if cluster:  # boxes 0, 1, 5, 7 around one centre: the 4th containing box comes late in the table
        for k, d in ((1, [0.06, -0.05, 0.03]), (5, [-0.05, 0.04, 0.0]), (7, [0.02, 0.07, -0.04])):
            box[k, 0:3] = box[0, 0:3] + d
        box[[0, 1, 5, 7], 3:6] = g.random((4, 3)) * 0.3 + 0.45
    if flat:
        box[2, 2], box[2, 5] = FLAT_Z, 0.0
    xyz = g.random((n, 3)) * [6.0, 5.0, 2.5] + [-3.0, 0.5, -1.3]
    if nb:
        inside = np.where(g.random(n) < 2.0 / 3.0)[0]
        b = g.integers(0, nb, inside.size)
        local = (g.random((inside.size, 3)) * 2 - 1) * box[b, 3:6]
        if cluster:  # a fifth of them close to the shared centre
            near = g.random(inside.size) < 0.2
            b[near] = 0
            local[near] = (g.random((int(near.sum()), 3)) * 2 - 1) * 0.12
        c, s = np.cos(box[b, 6]), np.sin(box[b, 6])
        xyz[inside, 0] = box[b, 0] + local[:, 0] * c + local[:, 1] * s
        xyz[inside, 1] = box[b, 1] - local[:, 0] * s + local[:, 1] * c
        xyz[inside, 2] = box[b, 2] + local[:, 2]
    rgb = np.round(g.random((n, 3)) * 255) / 256
    return np.concatenate([xyz, rgb], 1).astype(dtype), box


def membership(pc, box):
    """(n, K) analytic membership in float64 and the smallest distance of any point to a face of a
    box with a volume."""
    p = pc[:, 0:3].astype(np.float64)
    inside = np.zeros((p.shape[0], box.shape[0]), bool)
    closest = np.inf
    for k in range(box.shape[0]):
        d = p - box[k, 0:3]
        c, s = np.cos(box[k, 6]), np.sin(box[k, 6])
        loc = np.abs(np.stack([d[:, 0] * c - d[:, 1] * s, d[:, 0] * s + d[:, 1] * c, d[:, 2]], 1))
        half = np.abs(box[k, 3:6])
        if (half == 0).any():
            continue
        inside[:, k] = (loc <= half).all(1)
        for a in range(3):
            others = [x for x in range(3) if x != a]
            on_face = (loc[:, others] <= half[others] + 1e-5).all(1)
            if on_face.any():
                closest = min(closest, np.abs(loc[on_face, a] - half[a]).min())
    return inside, closest


def main(ref):
    for name in ("cv2", "mayavi", "mayavi.mlab", "plyfile", "trimesh", "matplotlib", "matplotlib.pyplot"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["mayavi"].mlab = sys.modules["mayavi.mlab"]
    sys.modules["plyfile"].PlyData = sys.modules["plyfile"].PlyElement = object
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    sys.modules["matplotlib.pyplot"].cm = types.SimpleNamespace(jet=None)  # a default argument
    for p in (os.path.join(ref, "utils"), os.path.join(ref, "sunrgbd")):
        sys.path.insert(0, p)
    import pc_util  # noqa: E402
    import sunrgbd_data as ref_data  # noqa: E402  (the reference's sunrgbd/sunrgbd_data.py)

    scenes = {}
    for i, (s, (n, nb, dtype, cluster, flat)) in enumerate(zip(SCENES, SPECS)):
        pc, box = make_scene(np.random.default_rng(SEED0 + i), n, nb, dtype, cluster, flat)
        if flat:  # points exactly in the plane of the zero-height box, inside its footprint
            g = np.random.default_rng(SEED0 + 100)
            local = (g.random((24, 2)) * 2 - 1) * box[2, 3:5]
            c, sn = np.cos(box[2, 6]), np.sin(box[2, 6])
            pc[:24, 0] = box[2, 0] + local[:, 0] * c + local[:, 1] * sn
            pc[:24, 1] = box[2, 1] - local[:, 0] * sn + local[:, 1] * c
            pc[:24, 2] = FLAT_Z
            assert (pc[:24, 2].astype(np.float64) == box[2, 2]).all()
        scenes[int(s)] = (pc, box)

    class Obj(object):
        def __init__(self, row):
            self.classname = CLASSES[int(row[7])]
            self.centroid = np.array(row[0:3])
            self.l, self.w, self.h = float(row[3]), float(row[4]), float(row[5])
            self.heading_angle = float(row[6])

    class StandIn(object):
        def __init__(self, root_dir, split="training", use_v1=False):
            pass

        def get_label_objects(self, idx):
            return [Obj(r) for r in scenes[idx][1]]

        def get_depth(self, idx):
            return scenes[idx][0]

    ref_data.sunrgbd_object = StandIn
    pc_util.random_sampling = lambda pc, num_sample, replace=None, return_choices=False: pc

    out = {"scan_names": np.array(SCENES)}
    with tempfile.TemporaryDirectory() as tmp:
        idx_file = os.path.join(tmp, "idx.txt")
        with open(idx_file, "w") as f:
            f.write("".join("%d\n" % int(s) for s in SCENES))
        folder = os.path.join(tmp, "out")
        ref_data.extract_sunrgbd_data(idx_file, "training", folder, num_point=1 << 20, save_votes=True,
                                      use_v1=True, skip_empty_scene=False)
        for s, (n, nb, dtype, cluster, flat) in zip(SCENES, SPECS):
            pc = np.load(os.path.join(folder, s + "_pc.npz"))["pc"]
            box = np.load(os.path.join(folder, s + "_bbox.npy"))
            votes = np.load(os.path.join(folder, s + "_votes.npz"))["point_votes"]
            assert pc.dtype == dtype and pc.shape == (n, 6) and np.array_equal(pc, scenes[int(s)][0])
            assert box.shape == (nb, 8) and np.array_equal(box, scenes[int(s)][1])
            assert votes.dtype == np.float64 and votes.shape == (n, 10)
            inside, closest = membership(pc, box)
            assert closest > 1e-5, (s, "a point within 1e-5 of a face", closest)
            hits = inside.sum(1)
            assert np.array_equal(votes[:, 0] > 0, hits > 0), (s, "hull and analytic membership differ")
            if cluster:
                assert (hits >= 4).sum() >= 10, (s, "no points in four or more boxes")
            if flat:
                assert (inside[:24, [0, 1, 3, 4]].sum(1) == 0).any(), "no in-plane point outside the other boxes"
            print(s, "points", n, "boxes", nb, pc.dtype, "in a box", int((hits > 0).sum()),
                  "in >= 4", int((hits >= 4).sum()), "most", int(hits.max()), "closest face %.3g" % closest)
            out[s + "_pc"], out[s + "_bbox"], out[s + "_votes"] = pc, box, votes
            out[s + "_hits"] = hits.astype(np.int8)
    path = os.path.join(HERE, "sunrgbd_votes_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 200 * 1024


if __name__ == "__main__":
    main(sys.argv[1])
