"""A fixed list of batches of the three scene loaders as one sha256 per tensor, to show that a change of
the loaders' host code leaves every batch as it was:

    python tools/loader_identity.py [--out FILE] [--against FILE]

The list: ScanNet and SUN RGB-D (votes from the file and from the boxes) x colour off / on x pretrain,
semi, semi with unlabeled_labels, eval x the device's own draws / explicit draws, and ScanLoader for
both datasets x colour off / on x own / explicit draws.  Scenes of 50, 1500, 3000 and 2500 points from
the modules' synthetic writers, N = 2049.  `host` holds the hashes of host_batch, always; `device` those
of the device builds when a GPU is present.  Only the loaders' public methods are used, so the same
file runs on an older tree.  Prints ONE JSON object (--out: also written there); --against FILE compares
with an earlier result and exits 1 when a hash differs or is missing.
"""
import argparse
import hashlib
import importlib
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
importlib.import_module("3dioumatch_amd")
V = importlib.import_module("3dioumatch_amd.votenet")
SN = importlib.import_module("3dioumatch_amd.votenet.scannet_data")
SU = importlib.import_module("3dioumatch_amd.votenet.sunrgbd_data")
SC = importlib.import_module("3dioumatch_amd.votenet.scan_data")
SIZES, N, COUNTER = (50, 1500, 3000, 2500), 2049, 9
KINDS = {"pretrain": ("pretrain", [0, 2], None, False), "semi": ("semi", [0, 1], [1, 0, 1], False),
         "semi_labels": ("semi", [0, 1], [1, 0, 1], True), "eval": ("eval", [0, 1], None, False)}


def digest(batch):
    out = {}
    for k, v in sorted(batch.items()):
        if torch.is_tensor(v):
            v = v.cpu().numpy()
        if isinstance(v, np.ndarray):
            head = ("%s%s" % (v.dtype, v.shape)).encode()
            out[k] = hashlib.sha256(head + np.ascontiguousarray(v).tobytes()).hexdigest()
        else:
            out[k] = repr(v)
    return out


def labeled_loaders(tmp, device):
    """(case prefix, loader) for every store of the list; device=None: host copies only."""
    sn, su = os.path.join(tmp, "scannet"), os.path.join(tmp, "sunrgbd")
    os.makedirs(sn)
    os.makedirs(su)
    sn_names, su_names = ["scene%04d_00" % i for i in range(4)], ["%06d" % (i + 1) for i in range(4)]
    for i, n in enumerate(SIZES):
        SN.write_synthetic_scans(sn, [sn_names[i]], num_points=n, instances=11, boxes=9 if i else 0, seed=50 + i)
        SU.write_synthetic_scans(su, [su_names[i]], num_points=n, boxes=7 if i else 0, seed=60 + i,
                                 dtype=np.float64 if i == 1 else np.float32)
    for color in (False, True):
        scenes = SN.ScanNetScenes(sn, sn_names, device, use_color=color, use_height=True)
        yield "scannet/color%d" % color, SN.ScanNetLoader(scenes, V.scannet_config(), N, seed=4,
                                                          labeled=sn_names[:3], unlabeled=sn_names[2:])
        for votes in ("file", "boxes"):
            scenes = SU.SunRgbdScenes(su, su_names, device, use_color=color, use_height=True, votes=votes)
            yield "sunrgbd-%s/color%d" % (votes, color), SU.SunRgbdLoader(
                scenes, V.sunrgbd_config(), N, seed=4, labeled=su_names[:3], unlabeled=su_names[2:])


def scan_loaders(device):
    for dataset in SC.DATASETS:
        clouds = [SC.synthetic_clouds(1, n, seed=70 + i, dataset=dataset)[0] for i, n in enumerate(SIZES)]
        store = SC.ScanStore(clouds, device, dataset)
        for color in (False, True):
            yield "scan-%s/color%d" % (dataset, color), SC.ScanLoader(store, N, use_color=color, seed=4)


def collect(device):
    """case -> {tensor: sha256}: host_batch with device=None, the device builds otherwise."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for prefix, loader in labeled_loaders(tmp, device):
            for name, (kind, lab, unl, labels) in KINDS.items():
                for explicit in (False, True):
                    draws = loader.host_draws(kind, lab, unl, COUNTER + 100) if explicit else None
                    if device is None:
                        b = loader.host_batch(kind, lab, unl, COUNTER, unlabeled_labels=labels, draws=draws)
                    elif kind == "semi":
                        b = loader.semi_batch(lab, unl, COUNTER, unlabeled_labels=labels, draws=draws)
                    else:
                        build = loader.pretrain_batch if kind == "pretrain" else loader.eval_batch
                        b = build(lab, COUNTER, draws=draws)
                    out["%s/%s/%s" % (prefix, name, "explicit" if explicit else "own")] = digest(b)
    for prefix, loader in scan_loaders(device):
        for explicit in (False, True):
            draws = loader.host_draws([3, 0, 2], COUNTER + 100) if explicit else None
            if device is None:
                b = loader.host_batch([3, 0, 2], COUNTER, draws=draws)
            else:
                b = loader.batch([3, 0, 2], COUNTER, draws=draws)
            out["%s/%s" % (prefix, "explicit" if explicit else "own")] = digest(b)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--against")
    args = ap.parse_args()
    result = {"host": collect(None)}
    if torch.cuda.is_available():
        result["device"] = collect(torch.device("cuda", 0))
    text = json.dumps(result, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if args.against:
        with open(args.against) as f:
            other = json.load(f)
        bad = [(half, case) for half in result if half in other
               for case in set(result[half]) | set(other[half])
               if result[half].get(case) != other[half].get(case)]
        halves = [h for h in result if h in other]
        print("compared %s: %d cases, %d differ" % (halves, sum(len(result[h]) for h in halves), len(bad)),
              file=sys.stderr)
        for item in sorted(bad):
            print("differs: %s %s" % item, file=sys.stderr)
        sys.exit(1 if bad or not halves else 0)


if __name__ == "__main__":
    main()
