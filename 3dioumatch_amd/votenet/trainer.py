"""The training loop around the captured steps (train.py:305-371 and :540-611; pretrain.py:310-347 and
its train()): epochs of steps, one host read per print interval, evaluation every `eval_interval`
epochs through the inference engine, and checkpoints with the reference's keys.

    runner = SemiSupervisedStep(cfg, dev, meter=True, guard=True)
    trainer = Trainer(runner, loader_epochs(runner, loader, "semi", 4, 8),
                      evaluate=engine_evaluator(eval_batches_fn, config_dict), log_dir="log")
    trainer.fit(1001)

What the loop adds to a step is host work only: the statistics are summed on the device by the
runner's TrainMeter (votenet/train_meter.py) and read once per print interval; the guard's verdict
(votenet_adam_step_guarded) is never read inside the loop.

Deviations from the reference, both for a reproducible resume:
  * resume() continues the EMA ramp from Adam's step count (train.py restarts global_step at 0);
  * `seed`: when given, torch's generators are re-seeded with seed + epoch (per rank) at the head
    of every epoch (train.py calls np.random.seed() there)."""
import os

import torch

from .step import bn_momentum_at, lr_at
from .train_meter import tb_name  # noqa: F401  (the loop's naming of a logged key, for callers)

def loader_epochs(runner, loader, kind, batch_size, unlabeled_batch_size=0, seed=0, rank=0, world=1,
                  unlabeled_labels=False):
    """epoch_batches for a ScanNetLoader or SunRgbdLoader: epoch -> the batches of scene_loader.epoch_plan,
    built on the device and prefetched by scene_loader.feed."""
    from .scene_loader import epoch_plan, feed

    def epoch_batches(epoch):
        semi = kind == "semi"
        plan = epoch_plan(len(loader.labeled), batch_size, epoch, seed=seed,
                          num_unlabeled=len(loader.unlabeled) if semi else 0,
                          unlabeled_batch_size=unlabeled_batch_size if semi else 0, rank=rank, world=world)
        return feed(runner, loader, plan, kind=kind, unlabeled_labels=unlabeled_labels)
    return epoch_batches


def engine_evaluator(eval_batches, config_dict, ap_iou_thresholds=(0.25, 0.5), graphs=True):
    """evaluate(net) for Trainer: evaluate_one_epoch (train.py:378-428) as inference.evaluate(device_ap=True,
    with_loss=True) on an InferenceEngine around `net` (made once, its folded weights refreshed per call).
    eval_batches() -> the evaluation batches.  -> (the loss statistics, one metrics dict per threshold)."""
    from . import inference
    engines = {}

    def evaluate(net):
        engine = engines.get(id(net))
        if engine is None:
            engine = engines[id(net)] = inference.InferenceEngine(net, graphs=graphs)
        else:
            engine.refresh()
        import numpy as np
        with np.errstate(invalid="ignore", divide="ignore"):
            metrics, stats = inference.evaluate(engine, eval_batches(), config_dict,
                                                ap_iou_thresholds=ap_iou_thresholds, device_ap=True,
                                                with_loss=True)
        return stats, metrics
    evaluate.ap_iou_thresholds = tuple(ap_iou_thresholds)
    return evaluate


class Trainer(object):
    def __init__(self, runner, epoch_batches, evaluate=None, log_dir=None, print_interval=25,
                 eval_interval=25, save_interval=200, base_lr=None, log=print, group=None,
                 lr_decay_steps=None, lr_decay_rates=None, seed=None):
        if getattr(runner, "meter", None) is None:
            raise ValueError("Trainer: the runner must be built with meter=True")
        self.runner, self.epoch_batches, self.evaluate = runner, epoch_batches, evaluate
        self.semi = hasattr(runner, "teacher")
        self.log_dir = log_dir
        self.print_interval, self.eval_interval, self.save_interval = \
            int(print_interval), int(eval_interval), int(save_interval)
        # train.py:49 / pretrain.py:48
        self.base_lr = float(base_lr) if base_lr is not None else (2e-3 if self.semi else 1e-3)
        self.lr_decay_steps, self.lr_decay_rates = lr_decay_steps, lr_decay_rates
        self._log, self.group, self.seed = log, group, seed
        self.rank = torch.distributed.get_rank(group) if group is not None else 0
        self.world = torch.distributed.get_world_size(group) if group is not None else 1
        self.best_map = [0.0, 0.0]
        self.loss = 0
        self.start_epoch = 0
        self.last_stats = None
        if log_dir is not None and self.rank == 0:
            os.makedirs(log_dir, exist_ok=True)

    # ------------------------------------------------------------------ logging
    def log(self, text):
        if self.rank != 0:
            return
        if self.log_dir is not None:
            with open(os.path.join(self.log_dir, "log_train.txt"), "a") as f:
                f.write(text + "\n")
        if self._log is not None:
            self._log(text)

    def learning_rate(self, epoch):
        if self.lr_decay_steps is None:
            return lr_at(epoch, self.base_lr)
        return lr_at(epoch, self.base_lr, self.lr_decay_steps, self.lr_decay_rates)

    def _set_epoch(self, epoch):
        runner = self.runner
        runner.set_epoch(epoch, self.base_lr)
        if self.lr_decay_steps is not None:
            lr = self.learning_rate(epoch)
            for group in runner.optimizer.param_groups:
                if torch.is_tensor(group["lr"]):
                    group["lr"].fill_(lr)
                else:
                    group["lr"] = lr
        if self.seed is not None:
            seed = int(self.seed) + epoch * self.world + self.rank
            torch.manual_seed(seed)
            if runner.device.type == "cuda":
                torch.cuda.manual_seed_all(seed)

    # ------------------------------------------------------------------ one epoch
    def _report(self, batch_idx):
        stats = self.runner.meter.result(reset=True, group=self.group)  # the interval's one host read
        self.last_stats = stats
        self.log(' ---- batch: %03d ----' % (batch_idx + 1))
        for key in sorted(stats):
            if key not in ("steps", "skipped_steps"):
                self.log('mean %s: %f' % (key, stats[key]))
        if stats["skipped_steps"]:
            self.log('skipped steps: %d' % stats["skipped_steps"])
        return stats

    def train_one_epoch(self, epoch):
        """train_one_epoch of train.py:305-371 / pretrain.py:310-347 -> the number of steps"""
        runner = self.runner
        self._set_epoch(epoch)
        runner.net.train()
        if self.semi:
            runner.teacher.train()
        runner.meter.reset()  # stat_dict = {} (train.py:306): no step of the last epoch in this one's means
        steps = 0
        for batch_idx, batch in enumerate(self.epoch_batches(epoch)):
            runner(batch)
            steps += 1
            if (batch_idx + 1) % self.print_interval == 0:
                self._report(batch_idx)
        return steps

    # ------------------------------------------------------------------ evaluation
    def evaluate_one_epoch(self):
        """evaluate_one_epoch (train.py:378-428) on the student, the network the reference evaluates;
        training mode is restored.  -> (mean loss, [mAP per threshold])"""
        net = self.runner.net
        net.eval()
        try:
            stats, metrics = self.evaluate(net)
        finally:
            net.train()
        for key in sorted(stats):
            if key != "mean_loss":
                self.log('eval mean %s: %f' % (key, stats[key]))
        thresholds = getattr(self.evaluate, "ap_iou_thresholds", (0.25, 0.5))
        maps = []
        for thresh, metrics_dict in zip(thresholds, metrics):
            self.log('-' * 10 + ' iou_thresh: %f ' % thresh + '-' * 10)
            for key in metrics_dict:
                self.log('eval %s: %f' % (key, metrics_dict[key]))
            maps.append(float(metrics_dict['mAP']))
        # train.py:427 averages detection_loss, pretrain.py's evaluation the loss: one criterion here
        return float(stats["mean_loss"]), maps

    # ------------------------------------------------------------------ checkpoints
    def checkpoint(self, epoch):
        """The reference's save_dict (train.py:570-579; pretrain.py's has no teacher)."""
        runner = self.runner
        clone = lambda sd: {k: v.detach().clone() for k, v in sd.items()}  # noqa: E731
        save_dict = {'epoch': epoch + 1,  # after training one epoch, the start_epoch should be epoch+1
                     'optimizer_state_dict': runner.optimizer_state_dict(),
                     'loss': self.loss,
                     'model_state_dict': clone(runner.net.state_dict())}
        if self.semi:
            save_dict['ema_model_state_dict'] = clone(runner.teacher.state_dict())
        return save_dict

    def _save(self, epoch, name):
        if self.log_dir is None or self.rank != 0:
            return
        torch.save(self.checkpoint(epoch), os.path.join(self.log_dir, name))

    def resume(self, path):
        """Load a checkpoint written here or by the reference (pretrain.py:190-200, train.py:205-222) ->
        the epoch to start from."""
        runner = self.runner
        ckpt = torch.load(path, map_location=runner.device, weights_only=False)
        runner.net.load_state_dict(ckpt['model_state_dict'])
        if self.semi:
            runner.teacher.load_state_dict(ckpt.get('ema_model_state_dict', ckpt['model_state_dict']))
        opt = ckpt.get('optimizer_state_dict')
        if opt is not None and opt.get("state"):
            runner.load_optimizer_state_dict(opt)
            step = runner.optimizer.state[runner.flat_params]["step"]
            runner.global_step = int(float(step))
        self.loss = ckpt.get('loss', 0)
        self.start_epoch = int(ckpt.get('epoch', 0))
        return self.start_epoch

    # ------------------------------------------------------------------ the loop
    def fit(self, max_epoch, start_epoch=None):
        start_epoch = self.start_epoch if start_epoch is None else int(start_epoch)
        for epoch in range(start_epoch, max_epoch):
            self.log('**** EPOCH %03d, STEP %d ****' % (epoch, self.runner.global_step))
            self.log('Current learning rate: %f' % self.learning_rate(epoch))
            self.log('Current BN decay momentum: %f' % bn_momentum_at(epoch))
            self.train_one_epoch(epoch)
            maps = None
            if epoch > 0 and epoch % self.eval_interval == 0 and self.evaluate is not None:
                self.loss, maps = self.evaluate_one_epoch()
            self._save(epoch, 'checkpoint.tar')
            if epoch % self.save_interval == 0:
                self._save(epoch, 'checkpoint_%d.tar' % epoch)
            if maps is not None:
                if sum(maps) > sum(self.best_map):  # train.py:596
                    self.best_map = list(maps)
                    self._save(epoch, 'best_checkpoint_sum.tar')
                self.log('epoch: %d best: %s' % (epoch, ', '.join('%f' % m for m in self.best_map)))
        return self.best_map
