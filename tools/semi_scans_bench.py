"""Measure the semi-supervised batch whose unlabeled rows come from label-free scans
(SceneLoader(unlabeled_scans=...), csrc/scan_batch.hip:scan_semi_kernel) against the labeled loader's
semi_batch for the same rows, on one GPU:

    python tools/semi_scans_bench.py [--repeats 5] [--out profiles/semi_scans.json]

16 ScanNet-sized synthetic scans (50k points, 40 instances, 25 boxes, float32 xyz + rgb) are written in
the preprocessed layout: 8 labeled, 8 unlabeled.  The labeled loader holds all 16 with their labels; the
mixed loader holds the 8 labeled ones and a ScanStore of the other 8 `_vert.npy` files.  One JSON line:
  build_ms      device time of one 4 + 8 x 40 000 semi batch: 20 builds captured into one graph,
                replayed 200 times between events; the two loaders alternated, --repeats each: median,
                spread (max - min) and the runs
  launches      kernel launches per batch, by the builders' code (scene_batch_build: boxes, points,
                votes; scene_scan_semi_build: one) -- `rocprofv3 --kernel-trace --stats` shows them
  store_bytes   device bytes of the 8 unlabeled scans in the labeled store (cloud, instance and semantic
                arrays, boxes, tables) and in the ScanStore (raw rows, floors, table), without and with
                colour
  equal         the two loaders' batches compared word for word at the timed shape
Nothing here asserts a time."""
import argparse
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
SD = importlib.import_module("3dioumatch_amd.votenet.scannet_data")
SC = importlib.import_module("3dioumatch_amd.votenet.scan_data")
NPTS, LAB, UNL, SCANS = 40000, 4, 8, 16
BUILDS, REPLAYS = 20, 200


def dev_bytes(store):
    return int(sum(t.numel() * t.element_size() for t in store.dev.values()))


def captured(loader):
    """A graph of BUILDS semi batches into one output set -> a function: device ms per build."""
    out = loader.allocate("semi", LAB, UNL)
    lab, unl = np.arange(LAB) % len(loader.labeled), np.arange(UNL) % len(loader.unlabeled)
    loader.semi_batch(lab, unl, 0, out=out)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for c in range(BUILDS):
            loader.semi_batch(lab, unl, 1000 + c, out=out)
    graph.replay()
    torch.cuda.synchronize()

    def run():
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(REPLAYS):
            graph.replay()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / (REPLAYS * BUILDS)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = V.scannet_config()
    names = ["scene%04d_00" % i for i in range(SCANS)]
    lab, unl = names[:SCANS // 2], names[SCANS // 2:]
    result = {"num_points": NPTS, "labeled_rows": LAB, "unlabeled_rows": UNL, "scan_points": 50000,
              "launches": {"labeled": 3, "mixed": 4}, "store_bytes": {}}
    with tempfile.TemporaryDirectory() as tmp:
        SD.write_synthetic_scans(tmp, names, num_points=50000, instances=40, boxes=25, seed=0)
        files = [os.path.join(tmp, s + "_vert.npy") for s in unl]
        store = SC.ScanStore.from_files(files, dev, "scannet")
        for colour in (False, True):
            whole = SD.ScanNetScenes(tmp, names, dev, use_color=colour, use_height=True)
            part = SD.ScanNetScenes(tmp, lab, dev, use_color=colour, use_height=True)
            result["store_bytes"]["colour" if colour else "xyz_height"] = {
                "labeled_store_8_scans": dev_bytes(whole) - dev_bytes(part), "scan_store_8_scans": dev_bytes(store)}
            if not colour:
                both = SD.ScanNetLoader(whole, cfg, NPTS, seed=0, labeled=lab, unlabeled=unl)
                mixed = SD.ScanNetLoader(part, cfg, NPTS, seed=0, unlabeled_scans=store)
        xyz = SC.ScanStore([c[:, :3] for c in store.clouds], dev, "scannet")
        result["store_bytes"]["xyz_height"]["scan_store_8_scans_xyz_files"] = dev_bytes(xyz)
    ids = (np.arange(LAB), np.arange(UNL))
    a, b = both.semi_batch(ids[0], ids[1], 7), mixed.semi_batch(ids[0], ids[1], 7)
    result["equal"] = all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32))
                          for k in a if torch.is_tensor(a[k]))
    runs = {"labeled": captured(both), "mixed": captured(mixed)}
    times = {k: [] for k in runs}
    for _ in range(args.repeats):
        for k, run in runs.items():
            times[k].append(run())
    result["build_ms"] = {k: {"median": round(float(np.median(v)), 4), "spread": round(max(v) - min(v), 4),
                              "runs": [round(x, 4) for x in v]} for k, v in times.items()}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
