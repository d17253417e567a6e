"""Cases the CPU and the GPU tests of the voxel downsample share (test_scan_voxels.py,
test_scan_voxels_gpu.py): a hand-made scan with rows on cell faces, zeros of both signs, duplicates,
a crowded cell and ties; eleven scans at the kernels' size boundaries; a scan with a cell per row; a
scan in one cell; a random cloud at an anisotropic, non-dyadic voxel.  Every cloud comes from a fixed
seed; a 6-column cloud is its 3-column one with colours behind it, so both keep the same rows.  The
host results (`kept`) are computed once per case and keep mode and shared."""
import importlib

import numpy as np

from conftest import load_pkg

load_pkg()
SV = importlib.import_module("3dioumatch_amd.votenet.scan_voxels")

F = np.float32
EDGE_VOXEL = 0.25  # a power of two: the faces are exact
BOUNDARY_SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 65535, 65536, 65537, 131073)
BOUNDARY_VOXEL = 0.1
ONE_CELL_ROWS = 70001  # a segment boundary (65536) inside
DISTINCT_ROWS = 4096   # a power of two: the table of 2 n slots is exactly half full
ANISO_VOXEL = (0.05, 0.1, 0.2)
KEEPS = ("first", "nearest")


def _with_colour(xyz, columns, seed):
    xyz = np.ascontiguousarray(xyz, F)
    if columns == 3:
        return xyz
    rgb = np.random.default_rng(seed).integers(0, 256, (len(xyz), 3)).astype(F)
    return np.ascontiguousarray(np.concatenate([xyz, rgb], 1))


# rows of edge_cloud by name; CROWD: the 300 rows of one cell
EDGE = {"face": 0, "below_face": 1, "neg_face": 2, "above_neg_face": 3, "neg_zero": 4, "pos_zero": 5,
        "twin_a": 6, "twin_b": 7, "far_pos": 8, "far_neg": 9, "crowd": 10, "mirror_first": 310, "mirror_lo": 311,
        "mirror_hi": 312, "centre_first": 313, "centre": 314}
CROWD = 300


def edge_cloud(columns=3):
    """One scan at voxel 0.25 (see EDGE for the rows):
      face / below_face         x = 0.25 and the float32 below it: cells 1 and 0 of x;
      neg_face / above_neg_face x = -0.25 and the float32 above it: both cell -1;
      neg_zero / pos_zero       x = -0.0 and +0.0 (in a cell of their own in y): both cell 0;
      twin_a / twin_b           two bit-identical rows;
      far_pos / far_neg         cells at +-1000 m;
      crowd ..                  300 rows of one cell, more than four waves contending for one word;
      mirror_first, lo, hi      a cell whose first row is off-centre and whose next two are mirrored about
                                the centre: equal d2, so `nearest` keeps mirror_lo, `first` mirror_first;
      centre_first, centre      a cell whose second row sits exactly on its centre."""
    g = np.random.default_rng(31)
    below, above = np.nextafter(F(0.25), F(0)), np.nextafter(F(-0.25), F(0))
    rows = [(0.25, 0.1, 0.1), (below, 0.1, 0.1), (-0.25, 0.1, 0.1), (above, 0.1, 0.1),
            (-0.0, 0.6, 0.1), (0.0, 0.6, 0.1), (3.1, 3.1, 0.3), (3.1, 3.1, 0.3),
            (1000.1, -1000.1, 0.1), (-1000.1, 1000.1, 0.1)]
    crowd = g.random((CROWD, 3)) * 0.2499 + [2.0, 2.0, 0.5]
    tail = [(5.01, 5.01, 0.01), (5.125 - 0.0625, 5.125, 0.125), (5.125 + 0.0625, 5.125, 0.125),
            (6.01, 6.01, 0.01), (6.125, 6.125, 0.125)]
    xyz = np.concatenate([np.array(rows, F), crowd.astype(F), np.array(tail, F)])
    assert xyz.shape[0] == EDGE["centre"] + 1
    return _with_colour(xyz, columns, 32)


def _aligned_box(n, i, g):
    """n rows uniform over a box of whole cells of BOUNDARY_VOXEL, about 1.5 rows per cell, at an
    origin of its own (negative cells too)"""
    cells = max(1.0, n / 1.5)
    ky = max(1, int(round(np.sqrt(cells / 2))))
    kx = max(1, int(np.ceil(cells / (2 * ky))))
    shift = np.array([-3 - 5 * i, 2 * i, -1], np.float64)
    return ((g.random((n, 3)) * [kx, ky, 2] + shift) * BOUNDARY_VOXEL).astype(F)


def boundary_clouds(columns=3):
    """eleven scans of one store: a row, a wave, a workgroup, a segment and two segments, each under,
    at and over"""
    g = np.random.default_rng(33)
    return [_with_colour(_aligned_box(n, i, g), columns, 34 + i) for i, n in enumerate(BOUNDARY_SIZES)]


def all_distinct(n=DISTINCT_ROWS, columns=3):
    """every row the centre of a cell of its own, in a shuffled order: the table at its full load,
    and the output is the input"""
    g = np.random.default_rng(35)
    idx = g.permutation(n)
    cells = np.stack([idx % 64 - 32, (idx // 64) % 64 - 32, idx // 4096 - 1], 1)
    return _with_colour((cells + 0.5) * EDGE_VOXEL, columns, 36)


def one_cell(n=ONE_CELL_ROWS, columns=3):
    """every row in the cell (2, 2, 2) of voxel 0.25: one row is kept"""
    g = np.random.default_rng(37)
    return _with_colour(g.random((n, 3)) * 0.2499 + 0.5, columns, 38)


def anisotropic(columns=3):
    g = np.random.default_rng(39)
    return _with_colour((g.random((20000, 3)) - 0.5) * [4.0, 4.0, 3.0], columns, 40)


# name -> (clouds(columns), voxel)
CASES = {
    "edge": (lambda columns: [edge_cloud(columns)], EDGE_VOXEL),
    "boundary": (boundary_clouds, BOUNDARY_VOXEL),
    "all_distinct": (lambda columns: [all_distinct(columns=columns)], EDGE_VOXEL),
    "one_cell": (lambda columns: [one_cell(columns=columns)], EDGE_VOXEL),
    "anisotropic": (lambda columns: [anisotropic(columns)], ANISO_VOXEL),
}

_clouds, _kept = {}, {}


def clouds(case, columns=3):
    """The case's clouds (shared: do not write to them)."""
    if (case, columns) not in _clouds:
        _clouds[case, columns] = CASES[case][0](columns)
        for c in _clouds[case, columns]:
            c.setflags(write=False)
    return _clouds[case, columns]


def voxel(case):
    return CASES[case][1]


def kept(case, keep):
    """host_voxels of the case, computed once."""
    if (case, keep) not in _kept:
        _kept[case, keep] = SV.host_voxels(clouds(case), voxel(case), keep)
        for k in _kept[case, keep]:
            k.setflags(write=False)
    return _kept[case, keep]


def _check_boundary_fractions():
    """every boundary scan of 64 rows or more keeps between 30 % and 70 % of them"""
    for keep in KEEPS:
        for n, k in zip(BOUNDARY_SIZES, kept("boundary", keep)):
            assert n < 64 or 0.3 * n <= len(k) <= 0.7 * n, (keep, n, len(k))


_check_boundary_fractions()
