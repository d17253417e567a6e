"""What `view_stats` costs the semi-supervised step (BASELINE semi configuration: 4 labeled + 8
unlabeled scenes, N = 40 000 points, 256 proposals, the default filter), in ONE process:

    python tools/view_stats_bench.py [--steps 20] [--rounds 5]

Two captured SemiSupervisedStep runners from the same start, view_stats off and on, timed in
alternating rounds of `--steps` steps each (the next batch's index chain prefetched, as bench.py
feeds the step); the median step time of each arm and their difference.  Then the lhs_pseudo_stats
pass alone (20 calls captured into one graph, replayed) on the flag-on runner's buffers: as the
step ran it (the default filter keeps no pseudo label on random weights), and with every slot kept
(each coverage tile then evaluates all of its 16 x 64 box pairs).  Prints one JSON line.
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LABELED, UNLABELED, NPTS = 4, 8, 40000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    importlib.import_module("3dioumatch_amd")
    V = importlib.import_module("3dioumatch_amd.votenet")
    U = importlib.import_module("3dioumatch_amd.votenet.losses_unlabeled")
    P = importlib.import_module("3dioumatch_amd.votenet.pseudo_nms")
    dev = torch.device("cuda:0")
    cfg = V.scannet_config()
    batches = [{k: v.to(dev) for k, v in V.make_semi_batch(LABELED, UNLABELED, NPTS, cfg, seed=100 + s,
                                                          unlabeled_labels=True).items()} for s in range(2)]
    runners = {}
    for flag in (False, True):
        cd = U.default_config_dict(cfg, unlabeled_batch_size=UNLABELED, view_stats=flag)
        runners[flag] = V.SemiSupervisedStep(cfg, dev, num_proposal=256, lr=2e-3, config_dict=cd)

    def run(runner, steps):
        views = [dict(batches[i % 2]) for i in range(steps + 1)]
        runner.prefetch_geometry(views[0])
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for i in range(steps):
            runner.prefetch_geometry(views[i + 1])
            runner(views[i])
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / steps

    for flag in (False, True):
        run(runners[flag], args.warmup)
    times = {False: [], True: []}
    for _ in range(args.rounds):
        for flag in (False, True):
            times[flag].append(run(runners[flag], args.steps))
    off, on = statistics.median(times[False]), statistics.median(times[True])

    # the pass alone, on the buffers of the flag-on runner's captured step
    r = runners[True]
    ep, ema, tail = r._end_points, r._ema_end_points, slice(LABELED, None)
    teacher = [ema[k][tail] for k in ("objectness_scores", "sem_cls_scores", "iou_scores", "heading_scores",
                                      "heading_residuals", "size_scores", "size_residuals", "center",
                                      "aggregated_vote_xyz")]
    aug = [r._cur[k][tail] for k in ("flip_x_axis", "flip_y_axis", "rot_mat", "scale")]
    gt = {k: r._cur[k] for k in U.GT_KEYS}
    cd = r.config_dict

    def pass_us(mask, iters=20):
        def once():
            P.pseudo_label_stats_gpu(*teacher, cfg.mean_size(dev), mask, gt, LABELED, ep["objectness_scores"][tail],
                                     ep["aggregated_vote_xyz"][tail], *aug, cd["obj_threshold"],
                                     cd["cls_threshold"], cd["iou_threshold"])
        for _ in range(3):
            once()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(iters):
                once()
        g.replay()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        g.replay()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / iters

    mask = ep["unlabeled_box_label_mask"].clone()
    print(json.dumps({
        "workload": "semi-supervised step, view_stats off vs on", "labeled": LABELED, "unlabeled": UNLABELED,
        "points": NPTS, "proposals": 256, "steps_per_round": args.steps, "rounds": args.rounds,
        "step_ms_off": round(off, 4), "step_ms_on": round(on, 4), "delta_ms": round(on - off, 4),
        "rounds_ms_off": [round(t, 4) for t in times[False]], "rounds_ms_on": [round(t, 4) for t in times[True]],
        "kept_slots": int(mask.sum()),
        "stats_pass_us": round(pass_us(mask), 2),
        "stats_pass_us_all_slots_kept": round(pass_us(torch.ones_like(mask)), 2),
        "graphs": bool(runners[False].graphs and runners[True].graphs)}))


if __name__ == "__main__":
    main()
