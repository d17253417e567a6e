"""Cases the CPU and the GPU tests of the tiled scan path share (test_scan_tiles.py,
test_scan_tiles_gpu.py): clouds with points on window bounds, an empty and a one-point tile, and
hand-made tile arenas for the merge."""
import importlib

import numpy as np

from conftest import load_pkg

load_pkg()
ST = importlib.import_module("3dioumatch_amd.votenet.scan_tiles")

INF = np.float32(np.inf)
TILE, OVERLAP = (4.0, 3.0), 1.0


def edge_clouds(columns=6):
    """three scans: a 10 m x 5 m one (3 x 2 tiles) with points exactly on lower and upper window
    bounds, one whose middle tile of three is empty and whose last holds one point, and a room"""
    g = np.random.default_rng(12)
    a = (g.random((3000, columns)) * [10, 5, 3, 255, 255, 255][:columns]).astype(np.float32)
    a[0, :2], a[1, :2] = (0, 0), (10, 5)  # the extent, exactly
    xw = ST.axis_windows(0, 10, TILE[0], OVERLAP)
    yw = ST.axis_windows(0, 5, TILE[1], OVERLAP)
    at = 2
    for bound in np.concatenate([xw[0][1:], xw[1][:-1]]):  # lower bounds 3, 6 and upper bounds 4, 7 of x
        a[at:at + 20, 0] = bound
        at += 20
    for bound in (yw[0][1], yw[1][0]):
        a[at:at + 20, 1] = bound
        at += 20
    b = (g.random((500, columns)) * [2.5, 2, 3, 255, 255, 255][:columns]).astype(np.float32)
    b[0, :2] = (0, 0)
    b[-1, :2] = (9.75, 1.0)  # alone in the last of three tiles; nothing in the middle one
    c = (g.random((700, columns)) * [3.9, 2.9, 3, 255, 255, 255][:columns]).astype(np.float32)
    return [a, b, c]


def hand_made_tiles(NC):
    """two scans: scan 0 of four tiles (2 x 2, cuts at x = 5, y = 3) -- one empty, one full, one all of
    whose rows it owns, one that owns none -- and scan 1 of one all-infinite tile; K = 6"""
    g = np.random.default_rng(9)
    T, K = 5, 6
    core = np.array([[-INF, 5, -INF, 3], [5, INF, -INF, 3], [-INF, 5, 3, INF], [5, INF, 3, INF],
                     [-INF, INF, -INF, INF]], np.float32)
    count = np.array([0, K, 4, 3, 5], np.int32)
    box = g.standard_normal((T, K, 7)).astype(np.float32)
    box[1, :, 0:2] = [[6, 1], [5, 2], [4.99, 1], [7, 3], [8, -2], [np.nextafter(np.float32(5), -INF), 0]]
    #   tile 1 owns x >= 5, y < 3: rows 0, 1 (x exactly on the cut: the upper tile's) and 4
    box[2, :4, 0:2] = [[1, 3], [2, 8], [-7, 3.5], [4, 100]]   # all owned (y exactly on the cut: the upper tile's)
    box[3, :3, 0:2] = [[4, 4], [6, 2], [5, np.nextafter(np.float32(3), -INF)]]  # none owned
    planes = {"count": count, "proposal": g.integers(0, 256, (T, K)).astype(np.int32),
              "cls": g.integers(0, 18, (T, K)).astype(np.int32),
              "score": g.random((T, K, NC) if NC else (T, K)).astype(np.float32), "box": box,
              "corners": g.standard_normal((T, K, 8, 3)).astype(np.float32)}
    for name in ("proposal", "cls", "score", "box", "corners"):  # rows past count are zero, as the pack leaves them
        for t in range(T):
            planes[name][t, count[t]:] = 0
    first, tiles = np.array([0, 4], np.int32), np.array([4, 1], np.int32)
    want_rows = [[(1, 0), (1, 1), (1, 4), (2, 0), (2, 1), (2, 2), (2, 3)], [(4, r) for r in range(5)]]
    return planes, first, tiles, core, want_rows
