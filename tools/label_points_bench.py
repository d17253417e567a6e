"""Time label_points (votenet/point_labels.py) on one floor of 1 M points, in ONE process.

    python tools/label_points_bench.py [--repeats 5] [--out profiles/label_points.json]

The input is tools/scan_voxel_bench.py's synthetic floor (two overlapping scans of a 28 m x 20 m room
shell, 1 M points) and the merged boxes of a 4 x 4 detect_tiled run on it (ScanNet config, random
weights, tiles of 8 m x 6 m, seam NMS, per-class scores).  The floor is labelled in two row orders: as
generated (each scan's rows are in random order over its half of the floor, so a workgroup's 256 points
span the whole half) and sorted by 0.5 m cell (what a downsampled or a scanner-ordered cloud looks like).

For each order: the device time between two events of scene_detections_frames and of
scene_points_label with the cull on and off, the three alternated (medians of 20 after 3 warm-ups);
label_points end to end from resident store and arena to resident labels (wall clock, synchronised);
the share of (workgroup, eligible row) pairs the cull drops, recomputed in numpy; the point-in-box
tests per second of the cull-off launch next to the rate the vector units could issue them at
(VALU_PER_TEST instructions per test, read off the inner loop's ISA: 3 v_sub_f32, 4 v_pk_mul / v_pk_add,
3 v_cmp_le per test and a v_mov per four; a wave64 VALU instruction takes 4 cycles on one of a CU's 4
SIMDs, 2.4 GHz nominal).  Once: host_label_points on the same planes and cloud, and whether the device's
labels equal it bit for bit.  One JSON line; nothing here asserts a time."""
import argparse
import importlib
import importlib.util
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
ST = importlib.import_module("3dioumatch_amd.votenet.scan_tiles")
PL = importlib.import_module("3dioumatch_amd.votenet.point_labels")
I = importlib.import_module("3dioumatch_amd.votenet.inference")
step = importlib.import_module("3dioumatch_amd.votenet.step")

DEV = torch.device("cuda:0")
B, N = 8, 40000
TILE, OVERLAP = (8.0, 6.0), 1.0
SORT_CELL = 0.5
VALU_PER_TEST = 10.25
CLOCK_HZ = 2.4e9


def floor_cloud(points):
    spec = importlib.util.spec_from_file_location("scan_voxel_bench", os.path.join(ROOT, "tools", "scan_voxel_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.floor_cloud(points)


def alternated_ms(fns, reps=20, warm=3):
    """{name: median device ms between two events}, the functions taken in turn"""
    times = {name: [] for name in fns}
    for it in range(reps + warm):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= warm:
                times[name].append(e0.elapsed_time(e1))
    return {name: round(statistics.median(v), 4) for name, v in times.items()}


def detections(parent):
    cfg = V.scannet_config()
    cd = {"dataset_config": cfg, "remove_empty_box": False, "use_3d_nms": True, "nms_iou": 0.25,
          "use_old_type_nms": False, "cls_nms": True, "use_iou_for_nms": False, "per_class_proposal": True,
          "conf_thresh": 0.05}
    engine = I.InferenceEngine(step.build_detector(cfg, seed=0).to(DEV).eval())
    tiles = ST.TileStore.from_store(parent, TILE, overlap=OVERLAP)
    return tiles, V.detect_tiled(engine, SC.ScanLoader(tiles, N), cd, batch_size=B, seam_nms=True)


def cull_share(cloud, frames, rank, radius):
    """of the (workgroup, eligible row) pairs of one scan, the share the cull drops (float64, as the kernel)"""
    n = len(cloud)
    blocks = -(-n // PL.LABEL_BLOCK)
    pad = np.full((blocks * PL.LABEL_BLOCK, 3), np.nan, np.float64)
    pad[:n] = cloud[:, 0:3]
    pad = pad.reshape(blocks, PL.LABEL_BLOCK, 3)
    lo, hi = np.nanmin(pad, 1), np.nanmax(pad, 1)
    rows = np.nonzero(rank)[0]
    centre, reach = frames[rows, 2:5].astype(np.float64), radius[rows].astype(np.float64)
    dropped = 0
    for b0 in range(0, blocks, 512):
        gap = np.maximum(np.maximum(lo[b0:b0 + 512, None] - centre[None], centre[None] - hi[b0:b0 + 512, None]), 0.0)
        dropped += int(((gap * gap).sum(-1) > reach[None] * reach[None]).sum())
    return round(dropped / max(1, blocks * len(rows)), 4), len(rows)


def order_arm(found, store, repeats):
    d, S, cap = store.dev, len(store), found.cap
    layout, arena = found.layout, found.arena

    def plane(name, dtype):
        at, shape = layout[name]
        flat = arena[at:at + int(np.prod(shape))]
        return (flat if dtype == torch.float32 else flat.view(dtype)).view(*shape)

    count, cls = plane("count", torch.int32), plane("cls", torch.int32)
    score, box = plane("score", torch.float32), plane("box", torch.float32)
    frames, points, scratch = PL.frames_gpu(count, cls, score, box, found.K)
    P = int(store.count.sum(dtype=np.int64))
    instance = torch.empty(P, dtype=torch.int32, device=DEV)
    semantic = torch.empty(P, dtype=torch.int32, device=DEV)
    blocks = PL.max_blocks_of(store.count)

    def label(cull):
        return lambda: PL.label_gpu(d["cloud"], d["offset"], d["count"], blocks, count, frames, scratch, found.K,
                                    points, cull=cull, instance=instance, semantic=semantic)

    row = alternated_ms({
        "scene_detections_frames_ms": lambda: PL.frames_gpu(count, cls, score, box, found.K, frames=frames,
                                                            points=points, scratch=scratch),
        "scene_points_label_cull_on_ms": label(True), "scene_points_label_cull_off_ms": label(False)})
    times = {True: [], False: []}
    for rep in range(repeats + 1):
        for cull in (True, False):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            labels = PL.label_points(found, store, cull=cull)
            torch.cuda.synchronize()
            if rep:
                times[cull].append(time.perf_counter() - t0)
    for cull, name in ((True, "label_points_cull_on_s"), (False, "label_points_cull_off_s")):
        row[name] = round(statistics.median(times[cull]), 6)
        row[name + "_repeats"] = [round(x, 6) for x in times[cull]]
    rank, _, radius = PL.scratch_views(scratch, S, cap)
    share, eligible = cull_share(store.clouds[0], frames[0].cpu().numpy(), rank[0].cpu().numpy(), radius[0].cpu().numpy())
    tests = P * eligible
    row.update(points=P, rows=int(count.cpu()[0]), eligible_rows=eligible, tests=tests, cull_drops_share=share,
               labelled_points=int((labels.instance >= 0).sum()), owners=int((labels.points > 0).sum()))
    row["tests_per_s_cull_off"] = round(tests / (row["scene_points_label_cull_off_ms"] * 1e-3), 0)
    return row, labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--no-host", dest="host", action="store_false", help="skip host_label_points (minutes at full size)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("label_points_bench: needs the GPU (no timing without it)")
    clouds = floor_cloud(args.points)
    parent = SC.ScanStore(clouds, DEV, "scannet")
    tiles, found = detections(parent)
    cells = np.floor(clouds[0][:, 0:3].astype(np.float64) / SORT_CELL).astype(np.int64)
    order = np.lexsort((cells[:, 2], cells[:, 1], cells[:, 0]))
    ordered = SC.ScanStore([clouds[0][order]], DEV, "scannet")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    issue_rate = cus * 4 * 16 * CLOCK_HZ / VALU_PER_TEST
    out = {"what": "label_points on one floor of %d points with the merged boxes of a %d-tile detect_tiled run "
                   "(seam NMS, random weights)" % (args.points, len(tiles)),
           "command": "python tools/label_points_bench.py --repeats %d --points %d" % (args.repeats, args.points),
           "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "tiles": len(tiles), "cap": found.cap,
           "label_block": PL.LABEL_BLOCK, "label_box_chunk": PL.LABEL_BOX_CHUNK, "valu_per_test": VALU_PER_TEST,
           "vector_issue_tests_per_s": round(issue_rate, 0), "compute_units": cus}
    out["as_generated"], labels = order_arm(found, parent, args.repeats)
    out["sorted_by_cell"], sorted_labels = order_arm(found, ordered, args.repeats)
    for arm in ("as_generated", "sorted_by_cell"):
        out[arm]["share_of_vector_issue_cull_off"] = round(out[arm]["tests_per_s_cull_off"] / issue_rate, 3)
    instance = labels.instance.cpu().numpy()
    out["sorted_is_the_permutation"] = bool(np.array_equal(sorted_labels.instance.cpu().numpy(), instance[order]))
    if args.host:
        planes = found.planes()
        t0 = time.perf_counter()
        want = PL.host_label_points({k: planes[k] for k in ("count", "cls", "score", "box")}, clouds,
                                    frames=labels.frames.cpu().numpy())
        out["host_label_points_s"] = round(time.perf_counter() - t0, 3)
        out["device_is_host"] = bool(np.array_equal(instance, want["instance"]) and
                                     np.array_equal(labels.points.cpu().numpy(), want["points"]) and
                                     np.array_equal(labels.semantic.cpu().numpy(), want["semantic"]))
        own = PL.host_frames({k: planes[k] for k in ("count", "cls", "score", "box")})["frames"]
        out["frame_values_differing_from_numpy"] = int((np.nan_to_num(own).view(np.uint32) !=
                                                        np.nan_to_num(labels.frames.cpu().numpy()).view(np.uint32)).sum())
        out["host_over_device"] = round(out["host_label_points_s"] / out["as_generated"]["label_points_cull_on_s"], 1)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
