"""Time PointLabels.index() (votenet/point_index.py) on one floor of 1 M points, in ONE process.

    python tools/point_index_bench.py [--repeats 5] [--out profiles/point_index.json]
    python tools/point_index_bench.py --trace as_generated        # the launch alone, for a kernel trace
    python tools/point_index_bench.py --kernel-stats as_generated=a/g_kernel_stats.csv sorted_by_cell=b/g_kernel_stats.csv ...

The input is tools/label_points_bench.py's: the synthetic floor (two overlapping scans of a 28 m x 20 m
room shell, 1 M points), the merged boxes of a 4 x 4 detect_tiled run on it (seam NMS, random weights,
cap = 4096) and label_points' instance plane, in two row orders: as generated (random over each scan's
half of the floor) and sorted by 0.5 m cell (coherent: long runs of one label).

For each order, alternated inside this run (medians of 20 after 3 warm-ups, device time between two
events): scene_points_index with its outputs and scratch resident, and the tensor library's way to
`order`, torch.sort(bucket, stable=True) on the same device plane (the keys already mapped to buckets,
which is not timed; it gives no `start`).  Then PointLabels.index() from resident labels to a resident
index (wall clock, synchronised), host_point_index on the same plane, the old points_of called once per
packed row (every call scans the scan's labels on the host; the one host copy is timed apart), and
whether the device's index equals the host's bit for bit.  The launches one by one come from a kernel
trace of the --trace arm, taken in a run of its own per order and merged in with --kernel-stats (the
average of each kernel's calls there).  The streaming floor quoted is one read of 4 bytes and one
write of 4 bytes per point per pass plus the digit table (written once, read and rewritten once, read
once) over HBM_BYTES_PER_S.  One JSON line; nothing here asserts a time."""
import argparse
import csv
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
PI = importlib.import_module("3dioumatch_amd.votenet.point_index")

DEV = torch.device("cuda:0")
ORDERS = ("as_generated", "sorted_by_cell")
KERNELS = ("count_kernel", "segments_kernel", "digits_kernel", "scatter_kernel", "boundary_kernel")
HBM_BYTES_PER_S = 6.3e12  # what a float4 copy reaches on this part (8.0e12 on paper)


def label_bench():
    spec = importlib.util.spec_from_file_location("label_points_bench", os.path.join(ROOT, "tools", "label_points_bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def workload(points):
    """{order: (store, labels)} and the detections: label_points_bench's floor in its two row orders"""
    LB = label_bench()
    clouds = LB.floor_cloud(points)
    parent = SC.ScanStore(clouds, DEV, "scannet")
    tiles, found = LB.detections(parent)
    cells = np.floor(clouds[0][:, 0:3].astype(np.float64) / LB.SORT_CELL).astype(np.int64)
    order = np.lexsort((cells[:, 2], cells[:, 1], cells[:, 0]))
    ordered = SC.ScanStore([clouds[0][order]], DEV, "scannet")
    return {"as_generated": (parent, PL.label_points(found, parent)),
            "sorted_by_cell": (ordered, PL.label_points(found, ordered))}, found, len(tiles)


def launch_of(store, labels):
    """(fn, start, order): scene_points_index on the labels' instance plane with everything resident"""
    S, cap, P = len(store), labels.cap, int(store.count.sum(dtype=np.int64))
    segments = PI.max_segments_of(store.count)
    d = store.dev
    start = torch.empty((S, cap + 1), dtype=torch.int32, device=DEV)
    order = torch.empty(P, dtype=torch.int32, device=DEV)
    scratch = torch.empty(PI.index_scratch_bytes(S, cap, segments, P), dtype=torch.uint8, device=DEV)

    def fn():
        PI.point_index_gpu(labels.instance, d["offset"], d["count"], cap, start=start, order=order, scratch=scratch,
                           max_segments=segments)
    return fn, start, order


def stream_floor(P, cap, segments):
    """(bytes, seconds): 8 bytes per point per pass and four passes over each pass's digit table"""
    total = 0
    for p in range(PI.passes_of(cap)):
        digits = min(1 << PI.INDEX_DIGIT_BITS, (cap >> (PI.INDEX_DIGIT_BITS * p)) + 1)
        total += 8 * P + 4 * 4 * segments * digits
    return total, total / HBM_BYTES_PER_S


def order_arm(store, labels, repeats, host):
    LB = label_bench()
    cap, P = labels.cap, int(store.count.sum(dtype=np.int64))
    fn, start, order = launch_of(store, labels)
    key = labels.instance
    bucket = torch.where((key >= 0) & (key < cap), key, torch.full_like(key, cap))
    row = LB.alternated_ms({"scene_points_index_ms": fn,
                            "torch_sort_stable_ms": lambda: torch.sort(bucket, stable=True)})
    row["torch_sort_over_index"] = round(row["torch_sort_stable_ms"] / row["scene_points_index_ms"], 3)
    row["torch_sort_is_order"] = bool(torch.equal(torch.sort(bucket, stable=True)[1].int(), order))
    times = []
    for rep in range(repeats + 1):
        labels._index = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        index = labels.index()
        torch.cuda.synchronize()
        if rep:
            times.append(time.perf_counter() - t0)
    row["index_s"] = round(statistics.median(times), 6)
    row["index_s_repeats"] = [round(x, 6) for x in times]
    floor_bytes, floor_s = stream_floor(P, cap, PI.max_segments_of(store.count))
    starts = index.start.cpu().numpy()
    row.update(points=P, cap=cap, passes=PI.passes_of(cap), segments=PI.max_segments_of(store.count),
               owned_points=int(starts[0, cap]), rows_with_points=int((np.diff(starts[0]) > 0).sum()),
               stream_floor_bytes=floor_bytes, stream_floor_ms=round(floor_s * 1e3, 4),
               floor_over_index=round(floor_s * 1e3 / row["scene_points_index_ms"], 3))
    if host:
        instance = labels.instance.cpu().numpy()
        t0 = time.perf_counter()
        want = PI.host_point_index(instance, store.offset, store.count, cap)
        row["host_point_index_s"] = round(time.perf_counter() - t0, 4)
        row["device_is_host"] = bool(np.array_equal(starts, want["start"]) and
                                     np.array_equal(index.order.cpu().numpy(), want["order"]))
        rows = int(labels.rows.cpu()[0])
        labels._index, labels._host = None, None  # the old path: one host copy, then a nonzero per call
        t0 = time.perf_counter()
        labels.host()
        t1 = time.perf_counter()
        lengths = [len(labels.points_of(0, r)) for r in range(rows)]
        t2 = time.perf_counter()
        row.update(old_points_of_calls=rows, old_points_of_host_copy_s=round(t1 - t0, 4),
                   old_points_of_all_rows_s=round(t2 - t1, 4),
                   old_points_of_is_index=bool(np.array_equal(lengths, np.diff(starts[0])[:rows])))
        row["host_over_index"] = round(row["host_point_index_s"] / row["index_s"], 1)
        row["old_points_of_over_index"] = round((t2 - t0) / row["index_s"], 1)
    return row


def kernel_stats(path):
    """{kernel: {calls, average_us, min_us}} of the index's kernels from a rocprofv3 kernel_stats.csv"""
    out = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            for k in KERNELS:
                if "::%s(" % k in r["Name"] and "Pass" in r["Name"]:
                    out[k] = {"calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1000, 2),
                              "min_us": round(float(r["MinNs"]) / 1000, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--no-host", dest="host", action="store_false", help="skip host_point_index and the old points_of")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", default=None, choices=ORDERS, help="run that order's launch alone (20 times): for a kernel trace")
    ap.add_argument("--kernel-stats", dest="kernel_stats", nargs="+", default=[], metavar="ORDER=CSV",
                    help="kernel_stats.csv files of the --trace arms")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("point_index_bench: needs the GPU (no timing without it)")
    arms, found, tiles = workload(args.points)
    if args.trace:
        fn, _, _ = launch_of(*arms[args.trace])
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        return
    out = {"what": "PointLabels.index() on one floor of %d points labelled by the merged boxes of a %d-tile detect_tiled "
                   "run (seam NMS, random weights)" % (args.points, tiles),
           "command": "python tools/point_index_bench.py --repeats %d --points %d%s" % (
               args.repeats, args.points, " --kernel-stats <ORDER=kernel_stats.csv of: rocprofv3 --kernel-trace --stats "
               "--output-format csv -- python tools/point_index_bench.py --trace ORDER>" if args.kernel_stats else ""),
           "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "tiles": tiles, "cap": found.cap,
           "index_digit_bits": PI.INDEX_DIGIT_BITS, "index_segment": PI.INDEX_SEGMENT, "index_tile": PI.INDEX_TILE,
           "hbm_bytes_per_s": HBM_BYTES_PER_S}
    for name in ORDERS:
        out[name] = order_arm(*arms[name], args.repeats, args.host)
    for item in args.kernel_stats:
        name, path = item.split("=", 1)
        if name not in ORDERS:
            raise SystemExit("--kernel-stats ORDER=CSV: ORDER is one of %s" % (ORDERS,))
        out[name]["kernel_trace"] = kernel_stats(path)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
