"""Time detect() against the host restatement a user would write without it, in ONE process.

    python tools/detect_bench.py [--scans 64] [--points 150000] [--repeats 3] [--out profiles/detect.json]

--scans synthetic scans of --points points (xyz), B = 8, N = 40 000, ScanNet config, random weights:
  (a) votenet.detect(): store on the device (upload + scene_scan_prepare), batches built by
      scene_scan_batch_build, engine.run, parse_predictions_device, scene_detections_pack, one copy
      of the arena at the end;
  (b) the same engine fed from the host: np.percentile per scan, the height channel and the sample in
      numpy (ScanLoader.host_batch of a host store), one upload per batch, parse_predictions per batch.
Both are wall clock from host clouds to host-readable detections, alternated per repeat after a warm-up
of each.  Also the device time between two events of the three new launches at these shapes, and
scene_scan_prepare on one scan of 1 M points.  One JSON line; nothing here asserts a time."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
importlib.import_module("3dioumatch_amd")
V = importlib.import_module("3dioumatch_amd.votenet")
SC = importlib.import_module("3dioumatch_amd.votenet.scan_data")
D = importlib.import_module("3dioumatch_amd.votenet.detect")
E = importlib.import_module("3dioumatch_amd.votenet.eval_helper")
I = importlib.import_module("3dioumatch_amd.votenet.inference")
step = importlib.import_module("3dioumatch_amd.votenet.step")

DEV = torch.device("cuda:0")
B, N = 8, 40000


def config_dict(cfg):
    return {"dataset_config": cfg, "remove_empty_box": False, "use_3d_nms": True, "nms_iou": 0.25,
            "use_old_type_nms": False, "cls_nms": True, "use_iou_for_nms": False,
            "per_class_proposal": True, "conf_thresh": 0.05}


def device_ms(fn, reps=20):
    """median device time between two events of fn(), after three warm-up calls"""
    out = []
    for it in range(reps + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if it >= 3:
            out.append(e0.elapsed_time(e1))
    return round(statistics.median(out), 4)


def run_device(engine, clouds, cd):
    store = SC.ScanStore(clouds, DEV, "scannet")
    found = V.detect(engine, SC.ScanLoader(store, N), cd, batch_size=B)
    return found.planes()["count"]


def run_host(engine, clouds, host_loader, cd):
    floors = [np.percentile(c[:, 2], 0.99) for c in clouds]  # what every __getitem__ recomputes
    assert len(floors) == len(clouds)
    ids = [np.arange(s, min(len(clouds), s + B)) for s in range(0, len(clouds), B)]

    def feed():
        for i, rows in enumerate(ids):
            yield torch.from_numpy(host_loader.host_batch(rows, i)["point_clouds"]).to(DEV)

    counts = []
    for end_points in engine.run(feed()):
        counts += [len(scene) for scene in E.parse_predictions(end_points, cd)]
    return counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=64)
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("detect_bench: needs the GPU (no timing without it)")
    cfg = V.scannet_config()
    cd = config_dict(cfg)
    engine = I.InferenceEngine(step.build_detector(cfg, seed=0).to(DEV).eval())
    clouds = SC.synthetic_clouds(args.scans, args.points, seed=1, color=False)
    host_loader = SC.ScanLoader(SC.ScanStore(clouds, None, "scannet"), N)

    times = {"detect": [], "host": []}
    for rep in range(args.repeats + 1):  # rep 0: warm-up (graph capture)
        for name, fn in (("detect", lambda: run_device(engine, clouds, cd)),
                         ("host", lambda: run_host(engine, clouds, host_loader, cd))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            counts = fn()
            torch.cuda.synchronize()
            if rep:
                times[name].append(time.perf_counter() - t0)
    # the per-class listing of (b) repeats every kept box for each class
    kept = int(np.sum(counts)) // cfg.num_class

    store = SC.ScanStore(clouds, DEV, "scannet")
    loader = SC.ScanLoader(store, N)
    d = store.dev
    out_set = loader.allocate(B)
    ep = engine(loader.batch(np.arange(B), 0)["point_clouds"])
    pred = E.parse_predictions_device(ep, cd)
    size64, heading64 = E.decode_boxes(ep, cfg)
    obj = torch.softmax(ep["objectness_scores"], -1)[:, :, 1].contiguous()
    K = pred["keep"].shape[1]
    arena = D.new_arena(B, K, cfg.num_class, DEV)
    big = SC.synthetic_clouds(1, 1000000, seed=2, color=False)
    big_store = SC.ScanStore(big, DEV, "scannet")
    bd = big_store.dev
    out = {
        "what": "detect() against the host restatement, %d synthetic scans of %d points, B = %d, N = %d, "
                "K = %d, ScanNet config" % (args.scans, args.points, B, N, K),
        "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "kept_boxes_last_run": kept,
        "detect_scans_per_s": round(args.scans / statistics.median(times["detect"]), 1),
        "host_scans_per_s": round(args.scans / statistics.median(times["host"]), 1),
        "detect_s_repeats": [round(x, 4) for x in times["detect"]],
        "host_s_repeats": [round(x, 4) for x in times["host"]],
        "scene_scan_prepare_store_ms": device_ms(lambda: SC.scan_prepare_gpu(d["cloud"], d["offset"], d["count"])),
        "scene_scan_batch_build_ms": device_ms(lambda: loader.batch(np.arange(B), 0, out=out_set)),
        "scene_detections_pack_ms": device_ms(lambda: D.pack_gpu(
            arena, B, 0, pred["keep"], obj, pred["cls"], pred["score"], ep["center"], size64, heading64,
            pred["corners"])),
        "scene_scan_prepare_1M_points_ms": device_ms(
            lambda: SC.scan_prepare_gpu(bd["cloud"], bd["offset"], bd["count"]), reps=10),
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
