"""Raw ScanNet scan folders -> the preprocessed layout: the front end of votenet/scannet_raw.py, in
place of the reference's scannet/batch_load_scannet_data.py.

    python tools/prepare_scannet.py --scans scans --label_map scannetv2-labels.combined.tsv --out data
    python tools/prepare_scannet.py --scans scans --label_map labels.tsv --out data --names train.txt --device cpu

--scans holds one folder per scan (`<scan>/<scan>_vh_clean_2.ply`, `<scan>.aggregation.json`,
`<scan>_vh_clean_2.0.010000.segs.json`, `<scan>.txt`); --names lists the scans to export (default:
every folder with a mesh file).  --out gets `<scan>_vert.npy`, `_ins_label.npy`, `_sem_label.npy` and
`_bbox.npy`, the folder votenet/scannet_data.ScanNetScenes reads.  --device cpu runs the numpy
restatement.  A scan with more than --max_points vertices keeps the draw (--seed, 0, its place in the
list); a scan that cannot be exported stops the run with its name."""
import argparse
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = 16  # scans read, exported and written at a time


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--scans', required=True, metavar='DIR')
    ap.add_argument('--label_map', required=True, metavar='TSV')
    ap.add_argument('--out', required=True, metavar='DIR')
    ap.add_argument('--names', default=None, metavar='FILE', help='one scan name per line')
    ap.add_argument('--max_points', type=int, default=50000)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--device', default='cuda:0', help="'cpu': the numpy restatement")
    return ap


def main(argv=None):
    flags = parser().parse_args(argv)
    sys.path.insert(0, ROOT)
    importlib.import_module("3dioumatch_amd")
    R = importlib.import_module("3dioumatch_amd.votenet.scannet_raw")
    if flags.names:
        with open(flags.names) as f:
            names = [x.strip() for x in f.read().splitlines() if x.strip()]
    else:
        names = R.raw_scan_names(flags.scans)
    if not names:
        raise SystemExit("no scans under %s" % flags.scans)
    device = None if flags.device == 'cpu' else flags.device
    label_map = R.read_label_map(flags.label_map)
    os.makedirs(flags.out, exist_ok=True)
    for start in range(0, len(names), BATCH):
        part = names[start:start + BATCH]
        records = (R.read_raw_scan(flags.scans, s, label_map) for s in part)
        # the draw of a scan is keyed by its place in the whole list
        arrays = R.export_raw_scans(records, device, flags.max_points, flags.seed, first_index=start)
        for s, a in zip(part, arrays):
            R.save_export(flags.out, s, a)
            print("%s: %d vertices, %d boxes" % (s, a["vert"].shape[0], a["bbox"].shape[0]))


if __name__ == "__main__":
    main()
