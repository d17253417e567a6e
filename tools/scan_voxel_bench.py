"""Time the voxel downsample of a scan store (votenet/scan_voxels.py), in ONE process.

    python tools/scan_voxel_bench.py [--repeats 5] [--out profiles/scan_voxels.json]
    python tools/scan_voxel_bench.py --trace            # the launches alone, for a kernel trace
    python tools/scan_voxel_bench.py --kernel-stats trace/g_kernel_stats.csv --out profiles/scan_voxels.json

The input is one synthetic floor of 1 M points: two registered scans of a room shell (floor, ceiling,
outer and inner walls of a 28 m x 20 m x 2.9 m storey, 3 mm of noise along the normals), one covering
x <= 4 m, the other x >= -4 m, so that the middle third is seen twice; voxel 5 cm; `first` and `nearest`.

For each keep mode: the device time between two events of scene_scan_voxel_mark (clear and insert
together: one entry point), scene_scan_voxel_count, scene_scan_voxel_gather and scene_scan_prepare on
the result; VoxelStore.from_store from resident store to resident store (wall clock, synchronised);
host_voxels on the same cloud; the kept fraction; the bytes the insert streams (rows read once, a slot
written per row) next to its atomics; and, once, TileStore.from_store + detect_tiled with and without
the downsample in front, alternated (ScanNet config, random weights, B = 8, N = 40 000, tiles of
8 m x 6 m).  Clear and insert one by one come from a kernel trace of the --trace arm, taken in a run
of its own and merged in with --kernel-stats (the average of each kernel's calls there).  One JSON
line; nothing here asserts a time."""
import argparse
import csv
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
ST = importlib.import_module("3dioumatch_amd.votenet.scan_tiles")
SV = importlib.import_module("3dioumatch_amd.votenet.scan_voxels")
I = importlib.import_module("3dioumatch_amd.votenet.inference")
step = importlib.import_module("3dioumatch_amd.votenet.step")

DEV = torch.device("cuda:0")
B, N = 8, 40000
TILE, OVERLAP = (8.0, 6.0), 1.0
VOXEL = 0.05
KERNELS = ("voxel_clear_kernel", "voxel_insert_kernel", "voxel_count_kernel", "voxel_gather_kernel",
           "scan_prepare_kernel")


def shell_scan(points, x_lo, x_hi, g):
    """`points` rows on the surfaces of the storey with x_lo <= x <= x_hi"""
    X, Y, Z = (x_lo, x_hi), (-10.0, 10.0), (0.0, 2.9)
    lx, ly, lz = X[1] - X[0], Y[1] - Y[0], Z[1] - Z[0]
    inner = [x for x in (-9.0, -2.0, 2.0, 9.0) if x_lo <= x <= x_hi]
    # (axis that is constant, its value, area)
    faces = [(2, Z[0], lx * ly), (2, Z[1], lx * ly), (1, Y[0], lx * lz), (1, Y[1], lx * lz)]
    faces += [(0, x, ly * lz) for x in (-14.0, 14.0) if x_lo <= x <= x_hi] + [(0, x, ly * lz) for x in inner]
    area = np.array([f[2] for f in faces])
    which = g.choice(len(faces), points, p=area / area.sum())
    p = g.random((points, 3)) * [lx, ly, lz] + [X[0], Y[0], Z[0]]
    for i, (axis, value, _) in enumerate(faces):
        rows = which == i
        p[rows, axis] = value + g.normal(0.0, 0.003, int(rows.sum()))
    return p.astype(np.float32)


def floor_cloud(points, seed=4):
    g = np.random.default_rng(seed)
    return [np.concatenate([shell_scan(points // 2, -14.0, 4.0, g), shell_scan(points - points // 2, -4.0, 14.0, g)])]


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


def wall(fns, repeats):
    """{name: seconds per repeat}, the functions alternated, after one warm-up round"""
    times = {name: [] for name, _ in fns}
    for rep in range(repeats + 1):
        for name, fn in fns:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep:
                times[name].append(time.perf_counter() - t0)
    return times


def launch_set(parent, keep):
    """the four entry points as closures over resident buffers, as VoxelStore.from_store chains them"""
    d, G = parent.dev, ST._segments(parent.count)
    args = (d["cloud"], d["offset"], d["count"])
    mark = SV.voxel_mark_gpu(*args, parent.count, VOXEL, keep, G)
    counts = SV.voxel_count_gpu(*args, VOXEL, keep, mark, G).cpu().numpy()
    count, offset, base = ST.gather_bases(counts)
    rows = int(count.sum(dtype=np.int64))
    base_dev = ST.to_device(base, DEV)
    out, source = SV.voxel_gather_gpu(*args, VOXEL, keep, mark, base_dev, rows, G)
    o, c = ST.to_device(offset, DEV), ST.to_device(count, DEV)
    given = {k: mark[k] for k in ("scratch", "slot", "table")}
    return rows, mark["total_slots"], {
        "scene_scan_voxel_mark": lambda: SV.voxel_mark_gpu(*args, parent.count, VOXEL, keep, G, **given),
        "scene_scan_voxel_count": lambda: SV.voxel_count_gpu(*args, VOXEL, keep, mark, G),
        "scene_scan_voxel_gather": lambda: SV.voxel_gather_gpu(*args, VOXEL, keep, mark, base_dev, rows, G,
                                                               out=out, source=source),
        "scene_scan_prepare": lambda: SC.scan_prepare_gpu(out, o, c)}


def keep_arm(parent, clouds, keep, repeats):
    rows, slots, fns = launch_set(parent, keep)
    P, C = int(parent.count.sum(dtype=np.int64)), parent.columns
    row = {"parent_rows": P, "kept_rows": rows, "kept_fraction": round(rows / P, 4), "table_slots": slots,
           "table_bytes": 16 * slots}
    for name, fn in fns.items():
        row[name + "_ms"] = device_ms(fn)
    times = wall((("from_store", lambda: SV.VoxelStore.from_store(parent, VOXEL, keep=keep)),), repeats)["from_store"]
    row["from_store_s"] = round(statistics.median(times), 5)
    row["from_store_s_repeats"] = [round(x, 5) for x in times]
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        kept = SV.host_voxels(clouds, VOXEL, keep)
        host.append(time.perf_counter() - t0)
    row["host_voxels_s"] = round(statistics.median(host), 4)
    row["host_over_device"] = round(row["host_voxels_s"] / row["from_store_s"], 1)
    store = SV.VoxelStore.from_store(parent, VOXEL, keep=keep)
    row["device_is_host"] = bool(np.array_equal(store.source, np.concatenate(kept)))
    # what the insert moves as a stream: every row's line read once, one int32 slot written per row; and
    # its atomics: one 8-byte compare-and-swap per probe (at least one per row) and one 8-byte minimum
    row["insert_stream_bytes"] = P * C * 4 + P * 4
    row["insert_atomic_bytes_at_least"] = P * 16
    row["gather_stream_bytes"] = P * 4 + rows * (2 * C * 4 + 4)  # slots read, kept rows read and written, source
    return row


def tiled_arm(parent, repeats):
    """TileStore.from_store + detect_tiled on the parent, and with the downsample in front, alternated"""
    cfg = V.scannet_config()
    cd = {"dataset_config": cfg, "remove_empty_box": False, "use_3d_nms": True, "nms_iou": 0.25,
          "use_old_type_nms": False, "cls_nms": True, "use_iou_for_nms": False, "per_class_proposal": True,
          "conf_thresh": 0.05}
    engine = I.InferenceEngine(step.build_detector(cfg, seed=0).to(DEV).eval())

    def run(store):
        tiles = ST.TileStore.from_store(store, TILE, overlap=OVERLAP)
        return tiles, V.detect_tiled(engine, SC.ScanLoader(tiles, N), cd, batch_size=B).planes()["count"]

    times = wall((("plain", lambda: run(parent)),
                  ("voxel_first", lambda: run(SV.VoxelStore.from_store(parent, VOXEL)))), repeats)
    plain, voxel = run(parent)[0], run(SV.VoxelStore.from_store(parent, VOXEL))[0]
    row = {"tiles_plain": len(plain), "tiles_voxel": len(voxel),
           "tile_rows_plain": int(plain.count.sum(dtype=np.int64)), "tile_rows_voxel": int(voxel.count.sum(dtype=np.int64))}
    for k, v in times.items():
        row["tile_and_detect_%s_s" % k] = round(statistics.median(v), 5)
        row["tile_and_detect_%s_s_repeats" % k] = [round(x, 5) for x in v]
    return row


def kernel_stats(path):
    """{kernel: {calls, average_us}} of the downsample's kernels from a rocprofv3 kernel_stats.csv"""
    out = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            for k in KERNELS:
                if k in r["Name"]:
                    out[k] = {"calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1000, 2),
                              "min_us": round(float(r["MinNs"]) / 1000, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true", help="run the launches alone (`first`, 10 times): for a kernel trace")
    ap.add_argument("--kernel-stats", dest="kernel_stats", default=None, help="a kernel_stats.csv of the --trace arm")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scan_voxel_bench: needs the GPU (no timing without it)")
    clouds = floor_cloud(args.points)
    parent = SC.ScanStore(clouds, DEV, "scannet")
    if args.trace:
        _, _, fns = launch_set(parent, "first")
        for _ in range(10):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        return
    out = {"what": "VoxelStore.from_store on one floor of %d points (two overlapping scans of a room shell), voxel %g m"
                   % (args.points, VOXEL),
           "command": "python tools/scan_voxel_bench.py --repeats %d --points %d%s" % (
               args.repeats, args.points, " --kernel-stats <kernel_stats.csv of: rocprofv3 --kernel-trace --stats "
               "--output-format csv -- python tools/scan_voxel_bench.py --trace>" if args.kernel_stats else ""),
           "device": torch.cuda.get_device_name(0), "repeats": args.repeats}
    for keep in SV.KEEP:
        out[keep] = keep_arm(parent, clouds, keep, args.repeats)
    out["tiled"] = tiled_arm(parent, args.repeats)
    if args.kernel_stats:
        out["kernel_trace_first"] = kernel_stats(args.kernel_stats)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
