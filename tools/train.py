"""Train the detector: the front end of votenet/trainer.py with the reference's flag names
(train.py:31-70, pretrain.py:28-62) for what is supported.

    python tools/train.py --stage pretrain --data_dir scans --meta_dir meta --log_dir log
    python tools/train.py --stage semi --synthetic 24 --max_epoch 4 --eval_interval 2 --log_dir /tmp/run
    python tools/train.py --stage semi --synthetic 24 --max_epoch 6 --resume --log_dir /tmp/run
    python tools/train.py --stage semi --data_dir scans --meta_dir meta --unlabeled_scans captures

--stage pretrain is pretrain.py (labeled scenes, no teacher), --stage semi is train.py (labeled +
unlabeled scenes, EMA teacher).  --synthetic N trains on N seeded stand-in scans
(scannet_data.write_synthetic_scans), so that the loop runs with no dataset at hand.  The statistics
are summed on the device and read once per --print_interval steps; --no_guard / --clip_grad_norm
choose what stands in front of the update (votenet/step.py).  --unlabeled_scans DIR takes the
unlabeled scans of --stage semi from a folder of bare clouds, every `.npy` / `.npz` in it (xyz or xyz +
rgb, no label files: votenet/scan_data.py), instead of the unlabeled split of --data_dir.
--raw_scans DIR --label_map TSV stand in place of --data_dir: DIR holds raw ScanNet scan folders
(`<scan>/<scan>_vh_clean_2.ply`, ...), whose labels and boxes are built on the device at start-up
(votenet/scannet_raw.py), so no preprocessing step comes before training.

--dataset sunrgbd trains on SUN RGB-D with the same stage defaults (the reference's run scripts pass
no dataset-specific flag):

    python tools/train.py --dataset sunrgbd --stage pretrain --data_dir sunrgbd_pc_bbox_votes_50k_v1_train \
        --val_dir sunrgbd_pc_bbox_votes_50k_v1_val --log_dir log
    python tools/train.py --dataset sunrgbd --stage semi --raw_trainval sunrgbd_trainval \
        --labeled_sample_list sunrgbd_v1_train_0.05.txt --log_dir log

--data_dir / --val_dir are the two prepared folders; --votes boxes reads no `_votes.npz` and computes
the vote labels from the boxes.  --raw_trainval DIR stands in place of both: DIR is the
`sunrgbd_trainval/` folder the reference's MATLAB step leaves (depth/, label_v1/ or, with
--use_sunrgbd_v2, label/, train_data_idx.txt, val_data_idx.txt), subsampled and turned into store rows
on the device at start-up (votenet/sunrgbd_raw.py).  --meta_dir holds --labeled_sample_list (default:
--raw_trainval's folder, where the reference keeps its lists); without a list every train scene is
labeled.  --unlabeled_scans DIR then also takes `.mat` depth clouds."""
import argparse
import importlib
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--stage', choices=('pretrain', 'semi'), default='semi')
    ap.add_argument('--synthetic', type=int, default=0, metavar='N', help='train on N synthetic scans')
    ap.add_argument('--dataset', default='scannet', choices=('scannet', 'sunrgbd'), help='Dataset name.')
    ap.add_argument('--data_dir', default=None, help='preprocessed scans (scannet_train_detection_data; '
                    'sunrgbd: sunrgbd_pc_bbox_votes_50k_v1_train)')
    ap.add_argument('--val_dir', default=None, help='sunrgbd: sunrgbd_pc_bbox_votes_50k_v1_val')
    ap.add_argument('--votes', default='file', choices=('file', 'boxes'),
                    help="sunrgbd: read _votes.npz, or compute the vote labels from the boxes")
    ap.add_argument('--raw_trainval', default=None, metavar='DIR',
                    help='sunrgbd: a raw sunrgbd_trainval folder in place of --data_dir and --val_dir')
    ap.add_argument('--use_sunrgbd_v2', action='store_true', help='Use V2 box labels for SUN RGB-D dataset')
    ap.add_argument('--raw_scans', default=None, metavar='DIR',
                    help='raw ScanNet scan folders in place of --data_dir (needs --label_map)')
    ap.add_argument('--label_map', default=None, metavar='TSV', help='scannetv2-labels.combined.tsv')
    ap.add_argument('--meta_dir', default=None, help='the split lists (scannet/meta_data)')
    ap.add_argument('--labeled_sample_list', default='scannetv2_train.txt')
    ap.add_argument('--unlabeled_scans', default=None, metavar='DIR',
                    help="--stage semi: the unlabeled scans are the .npy / .npz clouds of DIR, which need no "
                         "label files ('synthetic' with --synthetic N: the _vert.npy of the unlabeled half)")
    ap.add_argument('--detector_checkpoint', default='none')
    ap.add_argument('--log_dir', default='./temp', help='Dump dir to save model checkpoint')
    ap.add_argument('--num_point', type=int, default=40000, help='Point Number')
    ap.add_argument('--use_color', action='store_true')
    ap.add_argument('--no_height', action='store_true')
    ap.add_argument('--num_target', type=int, default=None, help='Proposal number [256 / 128]')
    ap.add_argument('--ap_iou_thresh', type=float, default=0.25)
    ap.add_argument('--max_epoch', type=int, default=1001, help='Epoch to run')
    ap.add_argument('--batch_size', default=None, help="'8' (pretrain) or labeled,unlabeled: '4,8' (semi)")
    ap.add_argument('--learning_rate', type=float, default=None, help='[0.001 pretrain / 0.002 semi]')
    ap.add_argument('--lr_decay_steps', default=None, help="[train.py: '400, 600, 800, 900']")
    ap.add_argument('--lr_decay_rates', default=None, help="[train.py: '0.3, 0.3, 0.1, 0.1']")
    ap.add_argument('--ema_decay', type=float, default=0.999, metavar='ALPHA')
    ap.add_argument('--unlabeled_loss_weight', type=float, default=2.0, metavar='WEIGHT')
    ap.add_argument('--print_interval', type=int, default=25, help='batch interval to print loss')
    ap.add_argument('--eval_interval', type=int, default=25, help='epoch interval to evaluate model')
    ap.add_argument('--save_interval', type=int, default=200, help='epoch interval to save model')
    ap.add_argument('--resume', action='store_true', help='continue from log_dir/checkpoint.tar')
    ap.add_argument('--conf_thresh', type=float, default=0.05)
    ap.add_argument('--view_stats', action='store_true')
    ap.add_argument('--no_guard', action='store_true', help='the plain update: no non-finite guard')
    ap.add_argument('--clip_grad_norm', type=float, default=None, metavar='NORM')
    ap.add_argument('--seed', type=int, default=None, help='re-seed torch with seed + epoch at every epoch')
    ap.add_argument('--device', default='cuda:0')
    return ap


def settings(flags):
    """The flags resolved against the stage's defaults (train.py:46-70 / pretrain.py:40-62)."""
    semi = flags.stage == 'semi'
    batch = flags.batch_size or ('4,8' if semi else '8')
    sizes = [int(x) for x in str(batch).split(',')]
    if len(sizes) != (2 if semi else 1):
        raise SystemExit("--batch_size: 'labeled,unlabeled' for --stage semi, one number for pretrain")
    steps = flags.lr_decay_steps or ('400, 600, 800, 900' if semi else '400, 600, 800')
    rates = flags.lr_decay_rates or ('0.3, 0.3, 0.1, 0.1' if semi else '0.1, 0.1, 0.1')
    steps, rates = [int(x) for x in steps.split(',')], [float(x) for x in rates.split(',')]
    if len(steps) != len(rates):
        raise SystemExit("--lr_decay_steps and --lr_decay_rates differ in length")
    return {
        'semi': semi, 'labeled_batch': sizes[0], 'unlabeled_batch': sizes[1] if semi else 0,
        'learning_rate': flags.learning_rate if flags.learning_rate is not None else (2e-3 if semi else 1e-3),
        'lr_decay_steps': steps, 'lr_decay_rates': rates,
        'num_target': flags.num_target if flags.num_target is not None else (128 if semi else 256),
        'guard': not flags.no_guard, 'clip_grad_norm': flags.clip_grad_norm,
    }


def eval_config_dict(cfg, flags):
    """train.py:263-275"""
    return {'dataset_config': cfg, 'remove_empty_box': False, 'use_3d_nms': True, 'nms_iou': 0.25,
            'use_old_type_nms': False, 'cls_nms': True, 'use_iou_for_nms': False,
            'per_class_proposal': True, 'conf_thresh': flags.conf_thresh}


def check_dataset_flags(flags, opt):
    """Refuse the flags of the other dataset and --dataset sunrgbd's own contradictions."""
    if flags.dataset == 'scannet':
        for name in ('val_dir', 'raw_trainval', 'use_sunrgbd_v2'):
            if getattr(flags, name):
                raise SystemExit("--%s belongs to --dataset sunrgbd" % name)
        if flags.votes != 'file':
            raise SystemExit("--votes belongs to --dataset sunrgbd")
        return
    if flags.raw_scans or flags.label_map:
        raise SystemExit("--raw_scans and --label_map belong to --dataset scannet")
    if flags.synthetic:
        return
    if flags.raw_trainval and (flags.data_dir or flags.val_dir):
        raise SystemExit("--raw_trainval DIR stands in place of --data_dir and --val_dir")
    if not flags.raw_trainval and not (flags.data_dir and flags.val_dir):
        raise SystemExit("--dataset sunrgbd: --data_dir and --val_dir, or --raw_trainval DIR, or --synthetic N")
    if flags.use_sunrgbd_v2 and not flags.raw_trainval:
        raise SystemExit("--use_sunrgbd_v2 chooses the label folder of --raw_trainval")
    if flags.labeled_sample_list != 'scannetv2_train.txt' and not (flags.meta_dir or flags.raw_trainval):
        raise SystemExit("--labeled_sample_list needs --meta_dir, the folder that holds it")
    if opt['semi'] and flags.unlabeled_scans is None and flags.labeled_sample_list == 'scannetv2_train.txt':
        raise SystemExit("--dataset sunrgbd --stage semi: --labeled_sample_list (e.g. sunrgbd_v1_train_0.05.txt) "
                         "or --unlabeled_scans DIR")


def sunrgbd_loaders(flags, opt, dev, V, SC):
    """-> (config, the train loader, the val loader) of --dataset sunrgbd."""
    SUN = importlib.import_module("3dioumatch_amd.votenet.sunrgbd_data")
    RAW = importlib.import_module("3dioumatch_amd.votenet.sunrgbd_raw")
    cfg = V.sunrgbd_config()
    color, height, seed = flags.use_color, not flags.no_height, flags.seed or 0
    tmp, list_path = None, None
    if flags.synthetic:
        tmp = tempfile.TemporaryDirectory()
        names = ["%06d" % i for i in range(1, flags.synthetic + 1)]
        SUN.write_synthetic_scans(tmp.name, names, num_points=max(flags.num_point, 2000) * 5 // 4, seed=0)
        # a quarter for evaluation, the rest halved into labeled and unlabeled scans
        n_val = max(1, flags.synthetic // 4)
        val, train = names[:n_val], names[n_val:]
        labeled = train[:len(train) // 2] if opt['semi'] else train
        unlabeled = train[len(train) // 2:] if opt['semi'] else None
        data_dir = val_dir = tmp.name
    else:
        if flags.labeled_sample_list != 'scannetv2_train.txt':
            list_path = os.path.join(flags.meta_dir or flags.raw_trainval, flags.labeled_sample_list)
        if flags.raw_trainval:
            train = RAW.read_idx_list(os.path.join(flags.raw_trainval, "train_data_idx.txt"))
            val = RAW.read_idx_list(os.path.join(flags.raw_trainval, "val_data_idx.txt"))
        else:
            data_dir, val_dir = flags.data_dir, flags.val_dir
            train, val = SUN.available_scans(data_dir), SUN.val_split(val_dir)
        listed = SUN._read_list(list_path) if list_path else list(train)
        labeled = [s for s in listed if s in set(train)]  # listed scans without files are skipped
        unlabeled = None
        if opt['semi'] and flags.unlabeled_scans is None:  # sunrgbd_ssl_dataset.py:193-203
            unlabeled = sorted(train if len(train) == len(listed) else set(train) - set(listed))
    scans = None
    if flags.unlabeled_scans == 'synthetic':
        files = [os.path.join(data_dir, s + "_pc.npz") for s in unlabeled]
    elif flags.unlabeled_scans is not None:
        files = sorted(os.path.join(flags.unlabeled_scans, f) for f in os.listdir(flags.unlabeled_scans)
                       if f.endswith((".npy", ".npz", ".mat")))
        if not files:
            raise SystemExit("--unlabeled_scans %s: no .npy, .npz or .mat cloud in it" % flags.unlabeled_scans)
    if flags.unlabeled_scans is not None:  # the labeled store then holds no unlabeled scan
        scans = SC.ScanStore.from_files(files, dev, "sunrgbd")
        unlabeled = None
    names = sorted(set(labeled) | set(unlabeled or ()))
    if flags.raw_trainval and not flags.synthetic:
        v1 = not flags.use_sunrgbd_v2
        scenes = SUN.SunRgbdScenes.from_raw(flags.raw_trainval, names, dev, color, height, use_v1=v1, seed=seed)
        val_scenes = SUN.SunRgbdScenes.from_raw(flags.raw_trainval, val, dev, color, height, use_v1=v1, seed=seed)
    else:
        scenes = SUN.SunRgbdScenes(data_dir, names, dev, color, height, votes=flags.votes)
        val_scenes = SUN.SunRgbdScenes(val_dir, val, dev, color, height, votes=flags.votes)
    if tmp is not None:
        tmp.cleanup()  # the stores are resident
    loader = SUN.SunRgbdLoader(scenes, cfg, flags.num_point, seed=seed, labeled=labeled, unlabeled=unlabeled,
                               unlabeled_scans=scans)
    return cfg, loader, SUN.SunRgbdLoader(val_scenes, cfg, flags.num_point, seed=seed, labeled=val)


def scannet_loaders(flags, opt, dev, V, SC):
    """-> (config, the train loader, the val loader) of --dataset scannet."""
    SD = importlib.import_module("3dioumatch_amd.votenet.scannet_data")
    cfg = V.scannet_config()
    use_height = not flags.no_height

    tmp = None
    if flags.synthetic:
        tmp = tempfile.TemporaryDirectory()
        names = ["scene%04d_00" % i for i in range(flags.synthetic)]
        SD.write_synthetic_scans(tmp.name, names, num_points=max(flags.num_point, 2000) * 5 // 4, seed=0)
        # a quarter for evaluation, the rest halved into labeled and unlabeled scans
        n_val = max(1, flags.synthetic // 4)
        val, train = names[:n_val], names[n_val:]
        labeled = train[:len(train) // 2] if opt['semi'] else train
        unlabeled = train[len(train) // 2:] if opt['semi'] else None
        data_dir = tmp.name
    else:
        if flags.raw_scans and (flags.data_dir or not flags.label_map):
            raise SystemExit("--raw_scans DIR --label_map TSV stand in place of --data_dir")
        if not (flags.data_dir or flags.raw_scans) or not flags.meta_dir:
            raise SystemExit("--data_dir (or --raw_scans and --label_map) and --meta_dir (or --synthetic N)")
        data_dir = flags.data_dir or flags.raw_scans  # the splits need the scans' names only
        labeled = SD.labeled_split(data_dir, flags.meta_dir, flags.labeled_sample_list)
        split = opt['semi'] and flags.unlabeled_scans is None
        unlabeled = SD.unlabeled_split(data_dir, flags.meta_dir, flags.labeled_sample_list) if split else None
        val = SD.val_split(data_dir, flags.meta_dir)
        names = sorted(set(labeled) | set(unlabeled or ()) | set(val))
    scans = None
    if flags.unlabeled_scans == 'synthetic':
        files = [os.path.join(data_dir, s + "_vert.npy") for s in unlabeled]
    elif flags.unlabeled_scans is not None:
        files = sorted(os.path.join(flags.unlabeled_scans, f) for f in os.listdir(flags.unlabeled_scans)
                       if f.endswith((".npy", ".npz")))
        if not files:
            raise SystemExit("--unlabeled_scans %s: no .npy or .npz cloud in it" % flags.unlabeled_scans)
    if flags.unlabeled_scans is not None:  # the labeled store then holds no unlabeled scan
        scans = SC.ScanStore.from_files(files, dev, "scannet")
        names = [s for s in names if s in set(labeled) | set(val)]
        unlabeled = None
    if flags.raw_scans and not flags.synthetic:
        scenes = SD.ScanNetScenes.from_raw(data_dir, names, flags.label_map, dev, use_color=flags.use_color,
                                           use_height=use_height)
    else:
        scenes = SD.ScanNetScenes(data_dir, names, dev, use_color=flags.use_color, use_height=use_height)
    if tmp is not None:
        tmp.cleanup()  # the stores are resident
    loader = SD.ScanNetLoader(scenes, cfg, flags.num_point, seed=flags.seed or 0, labeled=labeled,
                              unlabeled=unlabeled, unlabeled_scans=scans)
    return cfg, loader, SD.ScanNetLoader(scenes, cfg, flags.num_point, seed=flags.seed or 0, labeled=val)


def main(argv=None):
    flags = parser().parse_args(argv)
    opt = settings(flags)
    check_dataset_flags(flags, opt)
    if flags.unlabeled_scans is not None:
        if not opt['semi']:
            raise SystemExit("--unlabeled_scans: --stage pretrain trains on labeled scans only")
        if flags.view_stats:
            raise SystemExit("--unlabeled_scans with --view_stats: the statistics compare the pseudo-labels with "
                             "the unlabeled scans' own labels, which a folder of bare clouds does not have")
        if flags.unlabeled_scans == 'synthetic' and not flags.synthetic:
            raise SystemExit("--unlabeled_scans synthetic needs --synthetic N")
    sys.path.insert(0, ROOT)
    import torch
    importlib.import_module("3dioumatch_amd")
    V = importlib.import_module("3dioumatch_amd.votenet")
    SD = importlib.import_module("3dioumatch_amd.votenet.scene_loader")  # eval_batches
    SC = importlib.import_module("3dioumatch_amd.votenet.scan_data")
    T = importlib.import_module("3dioumatch_amd.votenet.trainer")
    U = importlib.import_module("3dioumatch_amd.votenet.losses_unlabeled")
    dev = torch.device(flags.device)
    if dev.type != "cuda":
        raise SystemExit("tools/train.py builds its batches on the GPU (--device cuda:N)")
    loaders = sunrgbd_loaders if flags.dataset == 'sunrgbd' else scannet_loaders
    cfg, loader, val_loader = loaders(flags, opt, dev, V, SC)

    common = dict(num_proposal=opt['num_target'], lr=opt['learning_rate'], meter=True, guard=opt['guard'],
                  clip_grad_norm=opt['clip_grad_norm'])
    if opt['semi']:
        cd = U.default_config_dict(cfg, unlabeled_batch_size=opt['unlabeled_batch'], view_stats=flags.view_stats)
        runner = V.SemiSupervisedStep(cfg, dev, unlabeled_loss_weight=flags.unlabeled_loss_weight,
                                      ema_decay=flags.ema_decay, config_dict=cd, **common)
    else:
        runner = V.SupervisedStep(cfg, dev, **common)
    if flags.detector_checkpoint != 'none':  # train.py:205-215: both networks start from the pretrained one
        ckpt = torch.load(flags.detector_checkpoint, map_location=dev, weights_only=False)
        runner.net.load_state_dict(ckpt['model_state_dict'])
        if opt['semi']:
            runner.teacher.load_state_dict(ckpt['model_state_dict'])

    batches = T.loader_epochs(runner, loader, flags.stage, opt['labeled_batch'], opt['unlabeled_batch'],
                              seed=flags.seed or 0, unlabeled_labels=flags.view_stats)
    eval_bs = opt['labeled_batch'] + opt['unlabeled_batch']
    evaluate = T.engine_evaluator(lambda: SD.eval_batches(val_loader, eval_bs), eval_config_dict(cfg, flags),
                                  ap_iou_thresholds=(flags.ap_iou_thresh, 0.5)
                                  if flags.ap_iou_thresh != 0.5 else (0.25, 0.5))
    trainer = T.Trainer(runner, batches, evaluate=evaluate, log_dir=flags.log_dir,
                        print_interval=flags.print_interval, eval_interval=flags.eval_interval,
                        save_interval=flags.save_interval, base_lr=opt['learning_rate'],
                        lr_decay_steps=opt['lr_decay_steps'], lr_decay_rates=opt['lr_decay_rates'],
                        seed=flags.seed)
    trainer.log(str(flags))
    if flags.resume:
        path = os.path.join(flags.log_dir, 'checkpoint.tar')
        trainer.log('resumed %s at epoch %d' % (path, trainer.resume(path)))
    trainer.fit(flags.max_epoch)
    torch.cuda.synchronize(dev)
    trainer.log('host reads of the training statistics: %d' % runner.meter.host_reads)
    if opt['guard']:
        trainer.log('guard: %s' % runner.guard_report())
    return trainer


if __name__ == '__main__':
    main()
