"""Regenerate tests/golden/sunrgbd_raw_ref.npz with the REFERENCE's own SUN RGB-D extraction (build
container only; needs scipy, whose loadmat and Delaunay hull the reference calls):

    python tests/golden/make_sunrgbd_raw_golden.py <path of the reference tree>

A small `sunrgbd_trainval/` is written to a temporary folder -- `depth/%06d.mat` by scipy's savemat
with compression, `label_v1/%06d.txt` as text -- and served, one scene per call so that each scene has
its own kept count, to sunrgbd/sunrgbd_data.py:extract_sunrgbd_data(save_votes=True, use_v1=True,
skip_empty_scene=False).  The reference's sunrgbd_object, read_sunrgbd_label and
load_depth_points_mat run unpatched; only the imports the path never calls (cv2, mayavi, plyfile,
trimesh, matplotlib) are stubbed, and pc_util.random_sampling is replaced by a seeded draw of the
same kind (np.random's choice, replace = n < num_point) whose indices are recorded as `<id>_choice`.
What the reference writes -- `<id>_pc.npz`, `<id>_bbox.npy`, `<id>_votes.npz` -- is the fixture, with
each scene's raw cloud, its label file's text and its kept count, and the bytes of one float32 and one
float64 `.mat` written by scipy (a second, short-named variable in front of `instance`).  Only data
is stored.

The scenes (id: raw points -> kept, cloud dtype, kept boxes / other label lines):

  000001  2300 -> 2048  float32   9 / 4   n > num_point: distinct indices; the two order statistics differ
  000002   150 -> 1977  float64   0 / 2   n < num_point: with replacement; no kept box
  000003   600 ->  600  float32  64 / 6   n == num_point; exactly MAX_NUM_OBJ kept boxes
  000004     1 -> 1977  float64   2 / 0   one point
  000005   500 -> 1977  float32   5 / 1   a run of 60 raw points with one z around the 0.99th percentile
  000006   200 -> 2048  float64   4 / 1   a run of 20 raw points with z = -0.0 there: the floor is a zero

2048 kept points put the virtual index 0.0099 * 2047 at 20.27 (numpy's lerp takes a + (b - a) t), 1977
at 19.56 (b - (b - a)(1 - t)).  To keep the fixture small, x and y of the float32 clouds are multiples
of 1/1024, their z -- but for the 64 lowest points, which decide the floor -- of 1/4096, every colour
is a multiple of 1/256 and the boxes' centres and half sizes of 1/64; a float64 cloud's coordinates
have every mantissa bit.  No point lies within 1e-5 of a face of a box (asserted below: move SEED0
if it fails), so the reference's hull test and the analytic test cannot differ on any point.
"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEED0 = 7313
CLASSES = ['bed', 'table', 'sofa', 'chair', 'toilet', 'desk', 'dresser', 'night_stand', 'bookshelf', 'bathtub']
OTHERS = ['lamp', 'pillow', 'garbage_bin', 'monitor']
# (id, raw points, kept, dtype, kept boxes, other lines, special)
SPECS = [("000001", 2300, 2048, np.float32, 9, 4, None), ("000002", 150, 1977, np.float64, 0, 2, None),
         ("000003", 600, 600, np.float32, 64, 6, None), ("000004", 1, 1977, np.float64, 2, 0, None),
         ("000005", 500, 1977, np.float32, 5, 1, "tie"), ("000006", 200, 2048, np.float64, 4, 1, "zero")]
TIE_Z = -1.2578125  # exact in float32


def make_scene(g, n, dtype, nb, other, special):
    box = np.zeros((nb, 7))
    box[:, 0:3] = g.random((nb, 3)) * [5.0, 4.0, 1.2] + [-2.5, 1.0, -0.6]
    box[:, 3:6] = g.random((nb, 3)) * 0.5 + 0.15
    box[:, 0:6] = np.round(box[:, 0:6] * 64) / 64
    box[:, 6] = g.random(nb) * 2 * np.pi - np.pi
    xyz = g.random((n, 3)) * [6.0, 5.0, 2.5] + [-3.0, 0.5, -1.3]
    if nb:
        inside = np.where(g.random(n) < 0.3)[0]
        b = g.integers(0, nb, inside.size)
        local = (g.random((inside.size, 3)) * 2 - 1) * box[b, 3:6]
        c, s = np.cos(box[b, 6]), np.sin(box[b, 6])
        xyz[inside, 0] = box[b, 0] + local[:, 0] * c + local[:, 1] * s
        xyz[inside, 1] = box[b, 1] - local[:, 0] * s + local[:, 1] * c
        xyz[inside, 2] = box[b, 2] + local[:, 2]
    if dtype == np.float32:
        xyz[:, 0:2] = np.round(xyz[:, 0:2] * 1024) / 1024
        high = np.argsort(xyz[:, 2])[64:]
        xyz[high, 2] = np.round(xyz[high, 2] * 4096) / 4096
    if special == "tie":    # two points below the run, 60 in it
        low = np.argsort(xyz[:, 2])
        xyz[low[:2], 2] = [-1.29, -1.28]
        xyz[low[2:62], 2] = TIE_Z
        xyz[low[62:], 2] = np.maximum(xyz[low[62:], 2], -1.25)
    if special == "zero":   # one point below the run of -0.0, everything else above it
        low = np.argsort(xyz[:, 2])
        xyz[:, 2] = np.abs(xyz[:, 2]) + 0.01
        xyz[low[0], 2] = -0.5
        xyz[low[1:21], 2] = -0.0
    rgb = np.round(g.random((n, 3)) * 255) / 256
    cloud = np.concatenate([xyz, rgb], 1).astype(dtype)
    # the label file: kept classes in table order with the other classes' lines spread between them
    lines = []
    for r in box:  # class, 2-D box, centroid, w l h, orientation
        v = list(g.random(4) * 100) + [r[0], r[1], r[2], r[4], r[3], r[5], np.cos(-r[6]), np.sin(-r[6])]
        lines.append(" ".join([CLASSES[int(g.integers(0, len(CLASSES)))]] + [repr(float(x)) for x in v]))
    for e, at in enumerate(sorted(np.linspace(0, nb, other, endpoint=False).astype(int).tolist(), reverse=True)):
        lines.insert(at, " ".join([OTHERS[e % len(OTHERS)]] + [repr(float(x)) for x in g.random(12) * 3]))
    return cloud, "".join(x + "\n" for x in lines)


def closest_face(pc, box):
    """The smallest distance of any point to a face of a box, analytic in float64."""
    p = pc[:, 0:3].astype(np.float64)
    closest = np.inf
    for k in range(box.shape[0]):
        d = p - box[k, 0:3]
        c, s = np.cos(box[k, 6]), np.sin(box[k, 6])
        loc = np.abs(np.stack([d[:, 0] * c - d[:, 1] * s, d[:, 0] * s + d[:, 1] * c, d[:, 2]], 1))
        half = np.abs(box[k, 3:6])
        for a in range(3):
            others = [x for x in range(3) if x != a]
            on_face = (loc[:, others] <= half[others] + 1e-5).all(1)
            if on_face.any():
                closest = min(closest, np.abs(loc[on_face, a] - half[a]).min())
    return closest


def main(ref):
    import scipy.io as sio
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

    draw = np.random.RandomState(SEED0)
    recorded = []

    def random_sampling(pc, num_sample, replace=None, return_choices=False):
        if replace is None:
            replace = pc.shape[0] < num_sample
        choices = draw.choice(pc.shape[0], num_sample, replace=replace)
        recorded.append(choices)
        return (pc[choices], choices) if return_choices else pc[choices]

    pc_util.random_sampling = random_sampling

    out = {"scan_names": np.array([s[0] for s in SPECS])}
    here = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, "sunrgbd_trainval")  # extract_sunrgbd_data opens './sunrgbd_trainval'
        for sub in ("depth", "label_v1"):
            os.makedirs(os.path.join(root, sub))
        os.chdir(tmp)
        try:
            for i, (s, n, kept, dtype, nb, other, special) in enumerate(SPECS):
                cloud, text = make_scene(np.random.default_rng(SEED0 + i), n, dtype, nb, other, special)
                sio.savemat(os.path.join(root, "depth", s + ".mat"), {"instance": cloud}, do_compression=True)
                with open(os.path.join(root, "label_v1", s + ".txt"), "w") as f:
                    f.write(text)
                idx_file = os.path.join(tmp, "idx_%s.txt" % s)
                with open(idx_file, "w") as f:
                    f.write("%d\n" % int(s))
                del recorded[:]
                ref_data.extract_sunrgbd_data(idx_file, "training", os.path.join(tmp, "out"), num_point=kept,
                                              save_votes=True, use_v1=True, skip_empty_scene=False)
                assert len(recorded) == 1
                choice = recorded[0]
                pc = np.load(os.path.join(tmp, "out", s + "_pc.npz"))["pc"]
                box = np.load(os.path.join(tmp, "out", s + "_bbox.npy"))
                votes = np.load(os.path.join(tmp, "out", s + "_votes.npz"))["point_votes"]
                assert pc.dtype == dtype and pc.shape == (kept, 6) and np.array_equal(pc, cloud[choice])
                assert box.shape == (nb, 8) and box.dtype == np.float64
                assert votes.dtype == np.float64 and votes.shape == (kept, 10)
                assert len(text.splitlines()) == nb + other
                assert (np.unique(choice).size == kept) == (n >= kept)
                closest = closest_face(pc, box)
                assert closest > 1e-5, (s, "a point within 1e-5 of a face", closest)
                z = np.sort(pc[:, 2])
                lo = int(np.floor(0.0099 * (kept - 1)))
                floor = np.percentile(pc[:, 2], 0.99)
                if special == "tie":
                    assert z[lo] == z[lo + 1] == np.float32(TIE_Z) and z[lo - 4] == z[lo + 8] and z[0] < z[lo]
                elif special == "zero":
                    assert floor == 0 and z[lo] == 0 and z[lo + 1] == 0 and z[0] < 0
                    assert not (np.signbit(pc[:, 2]) == 0)[pc[:, 2] == 0].any()  # every zero is -0.0
                elif n >= kept:
                    assert z[lo] != z[lo + 1]
                print(s, "raw", n, "kept", kept, pc.dtype, "boxes", nb, "in a box", int((votes[:, 0] > 0).sum()),
                      "floor %r" % floor, "closest face %.3g" % closest)
                out[s + "_raw"], out[s + "_label"] = cloud, np.frombuffer(text.encode("ascii"), np.uint8)
                out[s + "_num_point"], out[s + "_choice"] = np.int64(kept), choice.astype(np.int32)
                out[s + "_pc"], out[s + "_bbox"], out[s + "_votes"] = pc, box, votes
            # one small file of each class by a foreign writer, a short-named variable in front
            g = np.random.default_rng(SEED0 + 100)
            for tag, dtype in (("f32", np.float32), ("f64", np.float64)):
                array = np.concatenate([g.normal(size=(37, 3)), g.random((37, 3))], 1).astype(dtype)
                path = os.path.join(tmp, tag + ".mat")
                sio.savemat(path, {"a": np.arange(3.0), "instance": array}, do_compression=True)
                out["mat_%s_bytes" % tag] = np.fromfile(path, np.uint8)
                out["mat_%s_array" % tag] = array
        finally:
            os.chdir(here)
    path = os.path.join(HERE, "sunrgbd_raw_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 200 * 1024


if __name__ == "__main__":
    main(sys.argv[1])
