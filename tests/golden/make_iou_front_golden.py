"""Regenerate tests/golden/iou_front_ref.npz -- BUILD container only (imports the reference's Python
from /root/reference; only arrays are stored).

The REFERENCE VoteNet (models/votenet_iou_branch.py) runs forward_with_pred_jitter on the CPU for
ScanNet and SUN RGB-D, with ITS dataset configuration's class2angle_gpu, on the planted head outputs
of tests/test_iou_front.py (head_inputs: negative / zero / -0.0 sizes, headings at float32(pi) and
around it, the winning class first and last):
  * forward_backbone returns the planted head outputs and a small seed cloud;
  * the two torch.randn draws of the reference are made under torch.manual_seed, in its order; the planted
    draws (plant_noise: the 1e-8 clamp, a centre draw of 0) are written into what was drawn;
  * grid_conv.mlp_before_iou is a recorder; `pointnet2._ext` is the oracle stand-in, whose three_nn
    keeps the grid points it is asked about; `.cuda()` is the identity.
Stored: the inputs, the noise as used, size, heading, jitter_center, jitter_size, jitter_heading, and --
for the boxes listed in `grid_boxes` (every planted proposal, predicted and jittered copy, and every
17th box; all 64 grid points of each) -- the reference's whole_grid and relative_grid.  All boxes of
both tensors would be 1.3 MB.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, ROOT)
sys.path.insert(0, TESTS)
sys.path.insert(0, HERE)
from oracle.oracle import Oracle  # noqa: E402
from oracle import standin as oracle_ext  # noqa: E402
from test_iou_front import (GOLDEN_CHANNELS, GOLDEN_SEEDS, GOLDEN_SHAPE, NUM_CLASS, head_inputs,  # noqa: E402
                            plant_noise, seed_cloud)

REF = "/root/reference"
INPUT_KEYS = ("center", "size_scores", "size_residuals", "heading_scores", "heading_residuals")


class Recorder(nn.Module):
    def forward(self, x):
        self.seen = x.detach().clone()
        return x.new_zeros((x.shape[0], 128, x.shape[2], x.shape[3]))


def grid_box_list(plants, b, k):
    """flat indices into the (b, 2k) boxes the IoU branch sees: [predicted | jittered] per cloud"""
    picked = set(range(0, b * 2 * k, 17)) | {b * 2 * k - 1}
    for t in plants.values():
        cloud, prop = divmod(t, k)
        picked |= {cloud * 2 * k + prop, cloud * 2 * k + k + prop}
    return np.array(sorted(picked), dtype=np.int32)


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps: regenerating gives a byte-identical file"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    o = Oracle(omp=False)
    ext = oracle_ext.make(o)
    asked = []
    real_three_nn = ext.three_nn

    def three_nn(unknown, known):
        asked.append(unknown.detach().clone())
        return real_three_nn(unknown, known)

    ext.three_nn = three_nn
    sys.modules["pointnet2._ext"] = ext
    # utils/box_util.py wants pcdet's IoU at import; nothing here calls it
    iou_stub = types.ModuleType("pcdet.ops.iou3d_nms.iou3d_nms_utils")
    iou_stub.boxes_iou3d_gpu = None
    for name in ("pcdet", "pcdet.ops", "pcdet.ops.iou3d_nms"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["pcdet.ops.iou3d_nms.iou3d_nms_utils"] = iou_stub
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.cuda.FloatTensor = torch.FloatTensor
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "pointnet2"))
    from models.votenet_iou_branch import VoteNet  # noqa: E402
    from scannet.model_util_scannet import ScannetDatasetConfig  # noqa: E402
    from sunrgbd.model_util_sunrgbd import SunrgbdDatasetConfig  # noqa: E402

    b, k = GOLDEN_SHAPE
    out = {}
    for tag, cfg in (("scannet", ScannetDatasetConfig()), ("sunrgbd", SunrgbdDatasetConfig())):
        inp = head_inputs(tag, b, k)
        assert (cfg.num_size_cluster, cfg.num_heading_bin) == (inp["size_scores"].shape[-1],
                                                                inp["heading_scores"].shape[-1])
        net = VoteNet(NUM_CLASS[tag], cfg.num_heading_bin, cfg.num_size_cluster, inp["mean_size"], cfg,
                      input_feature_dim=1, num_proposal=k, sampling="seed_fps")
        torch.manual_seed(7)  # (the weights of the IoU head: its output is not stored)
        net.eval()
        net.grid_conv.mlp_before_iou = Recorder()
        seed_xyz, seed_features = seed_cloud(b, GOLDEN_SEEDS, GOLDEN_CHANNELS)

        def forward_backbone(inputs):
            ep = {key: torch.from_numpy(inp[key].copy()) for key in INPUT_KEYS}
            ep["seed_xyz"], ep["seed_features"] = torch.from_numpy(seed_xyz), torch.from_numpy(seed_features)
            return ep

        net.forward_backbone = forward_backbone
        real_randn = torch.randn
        # the reference's two draws (votenet_iou_branch.py:166-167), made ahead under the same seed and in
        # the same order, planted, and handed out where it calls torch.randn
        torch.manual_seed(5)
        ahead = [real_randn(b, k, 3), real_randn(b, k, 3)]
        plant_noise(ahead[0].numpy(), ahead[1].numpy(), inp["plants"])
        queue = list(ahead)
        torch.randn = lambda *a, **kw: queue.pop(0)
        del asked[:]
        try:
            with torch.no_grad():
                ep = net.forward_with_pred_jitter({"point_clouds": None})
        finally:
            torch.randn = real_randn
        assert not queue and len(asked) == 1
        for key in INPUT_KEYS + ("mean_size",):
            out["%s_in::%s" % (tag, key)] = inp[key]
        out[tag + "_in::noise_c"], out[tag + "_in::noise_s"] = ahead[0].numpy(), ahead[1].numpy()
        out[tag + "_in::seed_xyz"], out[tag + "_in::seed_features"] = seed_xyz, seed_features
        for key in ("size", "heading", "jitter_center", "jitter_size", "jitter_heading"):
            assert ep[key].dtype == torch.float32, key
            out["%s_%s" % (tag, key)] = ep[key].detach().numpy()
        boxes = grid_box_list(inp["plants"], b, k)
        whole = asked[0].numpy().reshape(b * 2 * k, 64, 3)
        rel = net.grid_conv.mlp_before_iou.seen[:, :3].numpy()           # (b, 3, 2k, 64)
        rel = rel.transpose(0, 2, 3, 1).reshape(b * 2 * k, 64, 3)
        out[tag + "_grid_boxes"] = boxes
        out[tag + "_whole"] = np.ascontiguousarray(whole[boxes])
        out[tag + "_relative"] = np.ascontiguousarray(rel[boxes])
        print(tag, "boxes stored", len(boxes), "headings above pi", int((ep["heading"] > np.pi).sum()))
    path = os.path.join(HERE, "iou_front_ref.npz")
    save_npz(path, out)
    print("iou_front_ref.npz %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
