"""Time the tiled scan path: the store's launches, the merge, and detect_tiled() end to end against the
host restatement, in ONE process.

    python tools/detect_tiled_bench.py [--repeats 3] [--out profiles/detect_tiled.json]
    python tools/detect_tiled_bench.py --seam [--repeats 5] [--out profiles/detect_tiled_seam.json]

Two workloads, ScanNet config, random weights, B = 8, N = 40 000:
  big    one synthetic scan of 1 M points over 28 m x 20 m, tiles of 8 m x 6 m with 1 m overlap: 4 x 4;
  rooms  64 room-sized scans of 150 000 points (tools/detect_bench.py's), same tile: one tile per scan.
For each: the device time between two events of scene_scan_bounds (two launches),
scene_scan_tile_count, scene_scan_tile_gather and scene_detections_merge; and wall clock from host
clouds to host-readable merged detections of
  (a) ScanStore + TileStore.from_store + detect_tiled + the one copy of the merged arena,
  (b) the same result through the host: host_bounds + tile_grid + host_tiles, a ScanStore of the crops,
      detect, host_merge,
alternated per repeat after a warm-up of each.  On `rooms` also detect() on the parent store against
detect_tiled() on its one-tile TileStore (stores built before the clock starts), alternated, with the
merge launch's device time next to them.  One JSON line; nothing here asserts a time.

--seam times the NMS across the cuts instead, on `big` alone (seam_arm): the four launches of
scene_detections_merge_nms together against the plain merge launch between device events,
detect_tiled() with and without seam_nms end to end, alternated, detect() on the tiles (the forward
passes alone), host_merge_nms on the same arena, and the partner pairs and resolve rounds of the run.
The launches one by one come from a kernel trace of this arm (seam_rows_kernel, seam_partners_kernel,
seam_resolve_kernel, seam_write_kernel; tile_merge_kernel is the plain merge)."""
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
ST = importlib.import_module("3dioumatch_amd.votenet.scan_tiles")
D = importlib.import_module("3dioumatch_amd.votenet.detect")
I = importlib.import_module("3dioumatch_amd.votenet.inference")
step = importlib.import_module("3dioumatch_amd.votenet.step")

DEV = torch.device("cuda:0")
B, N = 8, 40000
TILE, OVERLAP = (8.0, 6.0), 1.0


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


def big_cloud(points, seed):
    g = np.random.default_rng(seed)
    return [(g.random((points, 3)) * [28.0, 20.0, 3.0] - [14.0, 10.0, 0.1]).astype(np.float32)]


def run_device(engine, clouds, cd):
    tiles = ST.TileStore.from_store(SC.ScanStore(clouds, DEV, "scannet"), TILE, overlap=OVERLAP)
    return V.detect_tiled(engine, SC.ScanLoader(tiles, N), cd, batch_size=B).planes()["count"]


def run_host(engine, clouds, cd):
    grid = ST.tile_grid(ST.host_bounds(clouds), TILE, OVERLAP)
    built, crops = ST.host_tiles(clouds, grid)
    tiles = np.bincount(grid["parent"][built], minlength=len(clouds))
    first = np.concatenate([[0], np.cumsum(tiles)[:-1]])
    found = V.detect(engine, SC.ScanLoader(SC.ScanStore(crops, DEV, "scannet"), N), cd, batch_size=B)
    return D.host_merge(found.planes(), first, tiles, grid["core"][built])["count"]


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


def launches(engine, clouds, cd):
    """device ms of the store's three entry points and of the merge on `clouds`"""
    parent = SC.ScanStore(clouds, DEV, "scannet")
    d = parent.dev
    G = ST._segments(parent.count)
    tiles = ST.TileStore.from_store(parent, TILE, overlap=OVERLAP)
    t = tiles.dev
    base = ST.to_device(ST.gather_bases(
        ST.tile_count_gpu(d["cloud"], d["offset"], d["count"], t["parent"], t["window"], G).cpu().numpy())[2], DEV)
    rows = int(tiles.count.sum(dtype=np.int64))
    found = V.detect_tiled(engine, SC.ScanLoader(tiles, N), cd, batch_size=B)
    S, T, K, NC, cap = len(parent), len(tiles), found.K, found.NC, found.cap
    merged = D.new_merged_arena(S, cap, NC, DEV)
    return {"tiles": T, "tile_rows": rows, "parent_rows": int(parent.count.sum(dtype=np.int64)), "cap": cap,
            "scene_scan_bounds_ms": device_ms(lambda: ST.scan_bounds_gpu(d["cloud"], d["offset"], d["count"], G)),
            "scene_scan_tile_count_ms": device_ms(lambda: ST.tile_count_gpu(
                d["cloud"], d["offset"], d["count"], t["parent"], t["window"], G)),
            "scene_scan_tile_gather_ms": device_ms(lambda: ST.tile_gather_gpu(
                d["cloud"], d["offset"], d["count"], t["parent"], t["window"], base, rows, G)),
            "scene_detections_merge_ms": device_ms(lambda: D.merge_gpu(
                merged, found.tiles.arena, t["first"], t["tiles"], t["core"], S, T, K, NC, cap,
                int(tiles.tiles.max())))}


def seam_arm(engine, clouds, cd, repeats):
    """the --seam arm on `clouds` (module docstring)"""
    parent = SC.ScanStore(clouds, DEV, "scannet")
    tiles = ST.TileStore.from_store(parent, TILE, overlap=OVERLAP)
    loader = SC.ScanLoader(tiles, N)
    t = tiles.dev
    found = V.detect_tiled(engine, loader, cd, batch_size=B, seam_nms=True)
    S, T, K, NC, cap, most = len(parent), len(tiles), found.K, found.NC, found.cap, int(tiles.tiles.max())
    st = found.seam
    reach = tiles.reach_dev[st["seam"]]
    merged = D.new_merged_arena(S, cap, NC, DEV)
    scratch = torch.empty((D.seam_scratch_bytes(S, T, K, most) + 7) // 8, dtype=torch.float64, device=DEV)
    row = {"scans": S, "tiles": T, "K": K, "cap": cap, "seam": st, "scratch_bytes": scratch.numel() * 8,
           "scene_detections_merge_ms": device_ms(lambda: D.merge_gpu(
               merged, found.tiles.arena, t["first"], t["tiles"], t["core"], S, T, K, NC, cap, most)),
           "scene_detections_merge_nms_ms": device_ms(lambda: D.merge_nms_gpu(
               merged, found.tiles.arena, t["first"], t["tiles"], t["core"], t["iy"], t["ix"], reach, S, T, K, NC, cap,
               most, st["thresh"], st["old_type"], st["same_class"], st["dims"], scratch=scratch))}
    times = wall((("seam_off", lambda: V.detect_tiled(engine, loader, cd, batch_size=B).planes()),
                  ("seam_on", lambda: V.detect_tiled(engine, loader, cd, batch_size=B, seam_nms=True).planes()),
                  ("tiles_only", lambda: V.detect(engine, loader, cd, batch_size=B).planes())), repeats)
    for k, v in times.items():
        row["detect_tiled_%s_s" % k] = round(statistics.median(v), 5)
        row["detect_tiled_%s_s_repeats" % k] = [round(x, 5) for x in v]
    planes, host, info = found.tiles.planes(), [], {}
    for _ in range(3):
        t0 = time.perf_counter()
        want = D.host_merge_nms(planes, tiles.first, tiles.tiles, tiles.core, tiles.iy, tiles.ix, found.reach,
                                st["thresh"], st["old_type"], st["same_class"], st["dims"], info=info)
        host.append(time.perf_counter() - t0)
    plain = D.host_merge(planes, tiles.first, tiles.tiles, tiles.core)
    row.update({"host_merge_nms_s": round(statistics.median(host), 5), "packed_rows": int(planes["count"].sum()),
                "kept_rows": int(found.planes()["count"].sum()), "plain_rows": int(plain["count"].sum()),
                "device_is_host": bool(np.array_equal(found.planes()["count"], want["count"])),
                "partner_pairs": info["pairs"], "resolve_rounds": info["rounds"],
                "kept_guests": info["kept_guests"], "dropped_owned": info["dropped_owned"]})
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--big_points", type=int, default=1000000)
    ap.add_argument("--rooms", type=int, default=64)
    ap.add_argument("--room_points", type=int, default=150000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--seam", action="store_true", help="time the NMS across the cuts on `big` instead")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("detect_tiled_bench: needs the GPU (no timing without it)")
    cfg = V.scannet_config()
    cd = config_dict(cfg)
    engine = I.InferenceEngine(step.build_detector(cfg, seed=0).to(DEV).eval())
    out = {"what": "detect_tiled() against the host restatement; tiles of %g m x %g m, overlap %g m, B = %d, "
                   "N = %d, ScanNet config" % (TILE + (OVERLAP, B, N)),
           "device": torch.cuda.get_device_name(0), "repeats": args.repeats}
    if args.seam:
        out["what"] = "detect_tiled(seam_nms=True) against the plain merge; " + out["what"].split("; ", 1)[1]
        out["big"] = seam_arm(engine, big_cloud(args.big_points, 2), cd, args.repeats)
    workloads = () if args.seam else (
        ("big", big_cloud(args.big_points, 2)),
        ("rooms", SC.synthetic_clouds(args.rooms, args.room_points, seed=1, color=False)))
    for name, clouds in workloads:
        times = wall((("detect_tiled", lambda: run_device(engine, clouds, cd)),
                      ("host", lambda: run_host(engine, clouds, cd))), args.repeats)
        row = launches(engine, clouds, cd)
        row["scans"] = len(clouds)
        for k, v in times.items():
            row[k + "_scans_per_s"] = round(len(clouds) / statistics.median(v), 2)
            row[k + "_s_repeats"] = [round(x, 4) for x in v]
        out[name] = row
        if name == "rooms":  # one tile per scan: detect_tiled must cost detect plus the merge launch
            parent = SC.ScanStore(clouds, DEV, "scannet")
            tiles = ST.TileStore.from_store(parent, TILE, overlap=OVERLAP)
            assert tiles.tiles.tolist() == [1] * len(clouds)
            plain, tiled = SC.ScanLoader(parent, N), SC.ScanLoader(tiles, N)
            times = wall((("detect", lambda: V.detect(engine, plain, cd, batch_size=B).planes()),
                          ("detect_tiled", lambda: V.detect_tiled(engine, tiled, cd, batch_size=B).planes())),
                         max(args.repeats, 5))
            out["one_tile_per_scan"] = {
                "detect_s": round(statistics.median(times["detect"]), 5),
                "detect_tiled_s": round(statistics.median(times["detect_tiled"]), 5),
                "detect_s_repeats": [round(x, 5) for x in times["detect"]],
                "detect_tiled_s_repeats": [round(x, 5) for x in times["detect_tiled"]],
                "scene_detections_merge_ms": row["scene_detections_merge_ms"]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
