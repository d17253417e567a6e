"""A raw SUN RGB-D `sunrgbd_trainval/` folder -> the prepared layout: the front end of
votenet/sunrgbd_raw.py, in place of the reference's sunrgbd/sunrgbd_data.py --gen_v1_data / --gen_v2_data.

    python tools/prepare_sunrgbd.py --trainval sunrgbd_trainval --split train --out sunrgbd_pc_bbox_votes_50k_v1_train
    python tools/prepare_sunrgbd.py --trainval sunrgbd_trainval --split val --out val --v2 --votes --device cpu

--trainval is the folder the reference's MATLAB step leaves (depth/%06d.mat, label_v1/%06d.txt or, with
--v2, label/%06d.txt, train_data_idx.txt, val_data_idx.txt); --split train | val takes that index list,
anything else is the path of a list of data indices, one a line.  --out gets `<id>_pc.npz` and
`<id>_bbox.npy`, the folder votenet/sunrgbd_data.SunRgbdScenes reads with votes="boxes"; --votes also
writes `<id>_votes.npz`, computed from the boxes, so that the folder loads in the reference and as a
votes="file" store.  --device cpu runs the numpy restatement.  Scene number i of the list keeps the
draw (--seed, 0, i) of --num_point points; a scene that cannot be exported stops the run with its name."""
import argparse
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = 16  # scenes read, exported and written at a time


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--trainval', required=True, metavar='DIR')
    ap.add_argument('--split', required=True, metavar='train|val|FILE')
    ap.add_argument('--out', required=True, metavar='DIR')
    ap.add_argument('--v2', action='store_true', help='the V2 box labels (label/) instead of label_v1/')
    ap.add_argument('--num_point', type=int, default=50000)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--device', default='cuda:0', help="'cpu': the numpy restatement")
    ap.add_argument('--votes', action='store_true', help='write <id>_votes.npz too')
    return ap


def main(argv=None):
    flags = parser().parse_args(argv)
    sys.path.insert(0, ROOT)
    importlib.import_module("3dioumatch_amd")
    R = importlib.import_module("3dioumatch_amd.votenet.sunrgbd_raw")
    SUN = importlib.import_module("3dioumatch_amd.votenet.sunrgbd_data")
    listed = flags.split
    if listed in ('train', 'val'):
        listed = os.path.join(flags.trainval, listed + "_data_idx.txt")
    names = R.read_idx_list(listed)
    if not names:
        raise SystemExit("no scenes in %s" % listed)
    device = None if flags.device == 'cpu' else flags.device
    os.makedirs(flags.out, exist_ok=True)
    for start in range(0, len(names), BATCH):
        part = names[start:start + BATCH]
        records = (R.read_trainval_scene(flags.trainval, s, not flags.v2) for s in part)
        # the draw of a scene is keyed by its place in the whole list
        arrays = R.export_trainval(records, device, flags.num_point, flags.seed, first_index=start)
        for s, a in zip(part, arrays):
            R.save_export(flags.out, s, a)
            print("%s: %d points (%s), %d boxes" % (s, a["pc"].shape[0], a["pc"].dtype, a["bbox"].shape[0]))
        if flags.votes:  # from the boxes, on the device where there is one
            SUN.SunRgbdScenes(flags.out, part, device, votes="boxes").export_votes(flags.out)


if __name__ == "__main__":
    main()
