"""Time the mask matching (votenet/mask_eval.py) on one floor of 1 M points, in ONE process.

    python tools/mask_eval_bench.py [--repeats 5] [--out profiles/mask_eval.json]

The input is tools/label_points_bench.py's: the synthetic floor of tools/scan_voxel_bench.py, the merged
boxes of a 4 x 4 detect_tiled run on it (ScanNet config, random weights, seam NMS, per-class scores) and
label_points' owners, in two row orders: as generated (random over each scan's half of the floor) and
sorted by 0.5 m cell (what a scanner-ordered or downsampled cloud looks like: long runs of lanes share
a key).  The truth is synthetic: one instance per 2 m x 2 m cell of the floor plan and half of the
height (G = 280), a tenth of the points unannotated, the class a function of the cell.

For each order, alternated (medians of 20 device times between two events after 3 warm-ups): the overlap
launch alone in both forms -- equal keys of a wave merged before the atomic, and one atomic per lane --
without its clear launch (the tables just grow: the atomics are the same), the same two with the clear,
and the match launch; MaskAPCalculator.step end to end from resident labels, detections and truth (wall
clock, synchronised).  Once: host_match_masks on the same arrays and whether the device equals it bit for
bit.  The form that ships is the one that wins on the sorted order unless it loses more than 10 % on the
random one.  One JSON line; nothing here asserts a time."""
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
SC = importlib.import_module("3dioumatch_amd.votenet.scan_data")
PL = importlib.import_module("3dioumatch_amd.votenet.point_labels")
ME = importlib.import_module("3dioumatch_amd.votenet.mask_eval")

DEV = torch.device("cuda:0")
CELL = 2.0  # metres: the side of a truth instance's footprint


def label_bench():
    spec = importlib.util.spec_from_file_location("label_points_bench", os.path.join(ROOT, "tools", "label_points_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def floor_truth(cloud, seed=9):
    """(instance, class) per point: 14 x 10 x 2 cells of the 28 m x 20 m x 2.9 m storey"""
    g = np.random.default_rng(seed)
    ix = np.clip(np.floor((cloud[:, 0] + 14.0) / CELL), 0, 13).astype(np.int64)
    iy = np.clip(np.floor((cloud[:, 1] + 10.0) / CELL), 0, 9).astype(np.int64)
    cell = (ix * 10 + iy) * 2 + (cloud[:, 2] >= 1.45)
    instance = np.where(g.random(len(cloud)) < 0.1, 0, cell + 1).astype(np.int32)
    return instance, (cell % 20 - 1).astype(np.int32)  # -1 and 18: not a class


def order_arm(LB, found, store, truth, repeats):
    labels = PL.label_points(found, store)
    S, cap, G, d = len(store), labels.cap, truth.G, truth.dev
    blocks = PL.max_blocks_of(truth.count)
    scratch = torch.empty(ME.table_entries(S, cap, G), dtype=torch.int32, device=DEV)

    def overlap(merge, clear):
        return lambda: ME.overlap_gpu(d["offset"], d["count"], blocks, labels.instance, d["instance"], d["klass"], S, cap,
                                      G, merge=merge, clear=clear, scratch=scratch)

    at, shape = found.layout["cls"]
    cls = found.arena[at:at + int(np.prod(shape))].view(torch.int32).view(*shape)
    at, shape = found.layout["score"]
    score = found.arena[at:at + int(np.prod(shape))].view(*shape)
    overlap(True, True)()
    out = ME.match_gpu(labels.rows, cls, score, labels.points, scratch, G, found.num_class)
    row = LB.alternated_ms({
        "overlap_merged_ms": overlap(True, False), "overlap_plain_ms": overlap(False, False),
        "overlap_merged_with_clear_ms": overlap(True, True), "overlap_plain_with_clear_ms": overlap(False, True),
        "match_ms": lambda: ME.match_gpu(labels.rows, cls, score, labels.points, scratch, G, found.num_class, out=out)})
    times = []
    for rep in range(repeats + 1):
        meter = ME.MaskAPCalculator((0.25, 0.5))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        meter.step(labels, found, truth)
        torch.cuda.synchronize()
        if rep:
            times.append(time.perf_counter() - t0)
    row["step_s"] = round(statistics.median(times), 6)
    row["step_s_repeats"] = [round(x, 6) for x in times]
    both = (labels.instance >= 0) & (d["instance"] > 0)
    row.update(points=int(truth.count.sum()), rows=int(labels.rows.cpu()[0]), cap=cap, G=G,
               table_bytes=ME.mask_scratch_bytes(S, cap, G), labelled_and_annotated_points=int(both.sum()),
               annotated_points=int((d["instance"] > 0).sum()))
    return row, labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mask_eval_bench: needs the GPU (no timing without it)")
    LB = label_bench()
    clouds = LB.floor_cloud(args.points)
    parent = SC.ScanStore(clouds, DEV, "scannet")
    tiles, found = LB.detections(parent)
    cells = np.floor(clouds[0][:, 0:3].astype(np.float64) / LB.SORT_CELL).astype(np.int64)
    order = np.lexsort((cells[:, 2], cells[:, 1], cells[:, 0]))
    ordered = SC.ScanStore([clouds[0][order]], DEV, "scannet")
    instance, klass = floor_truth(clouds[0])
    out = {"what": "match_masks on one floor of %d points with the merged boxes of a %d-tile detect_tiled run (seam NMS, "
                   "random weights) against %d synthetic truth instances" % (args.points, len(tiles), int(instance.max())),
           "command": "python tools/mask_eval_bench.py --repeats %d --points %d" % (args.repeats, args.points),
           "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "mask_block": ME.MASK_BLOCK,
           "merge_rounds": ME.MASK_MERGE_ROUNDS}
    arms = {}
    for arm, store, perm in (("as_generated", parent, None), ("sorted_by_cell", ordered, order)):
        truth = ME.PointTruth(store.names, [instance if perm is None else instance[perm]],
                              [klass if perm is None else klass[perm]], DEV)
        out[arm], labels = order_arm(LB, found, store, truth, args.repeats)
        arms[arm] = (labels, truth)
    coherent, random = out["sorted_by_cell"], out["as_generated"]
    merged_wins = coherent["overlap_merged_ms"] < coherent["overlap_plain_ms"]
    winner, other = ("merged", "plain") if merged_wins else ("plain", "merged")
    loss = random["overlap_%s_ms" % winner] / random["overlap_%s_ms" % other] - 1.0
    rule = winner if loss <= 0.10 else other
    out["rule_picks"] = rule
    out["shipped"] = "merged" if ME.MERGE else "plain"
    out["why"] = ("%s wins on the sorted order (%.4f ms against %.4f ms) and on the random order it is %+.1f %% against "
                  "the other form (%.4f ms against %.4f ms; the limit is +10 %%)"
                  % (winner, coherent["overlap_%s_ms" % winner], coherent["overlap_%s_ms" % other], 100 * loss,
                     random["overlap_%s_ms" % winner], random["overlap_%s_ms" % other]))
    labels, truth = arms["as_generated"]
    host_truth = ME.PointTruth(parent.names, [instance], [klass], None)
    h, planes = labels.host(), found.planes()
    t0 = time.perf_counter()
    want = ME.host_match_masks(h["instance"], h["points"], planes, host_truth, found.num_class)
    out["host_match_masks_s"] = round(time.perf_counter() - t0, 3)
    got = ME.match_masks(labels, found, truth).host()
    out["device_is_host"] = bool(all(np.array_equal(got[k], want[k]) for k in ("inter", "size", "klass", "jmax", "key", "npos"))
                                 and np.array_equal(got["ovmax"].view(np.uint64), want["ovmax"].view(np.uint64)))
    out["detections"] = int((want["key"] != ME.NOT_A_DETECTION).sum())
    out["matched_detections"] = int(np.isfinite(want["ovmax"]).sum())
    out["host_over_device_step"] = round(out["host_match_masks_s"] / out["as_generated"]["step_s"], 1)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
