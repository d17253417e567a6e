"""Device-side statistics of the training loop (train.py:356-369, pretrain.py:335-347).

The reference adds `end_points[key].item()` to a host dict for every key containing 'loss', 'acc',
'ratio' or 'value', every step: 30-60 host round trips against a step that is otherwise a few graph
replays.  TrainMeter keeps the same sums in one device vector of doubles:

  * captured step: the static scalars of the graph's end_points never move, so their addresses go
    into a pointer table once and ONE launch of votenet_train_meter_add, captured behind the Adam
    call, adds all of them (and reads the guard's verdict: a skipped step is only counted);
  * eager step and CPU: the scalars are fresh tensors every step, so the same arithmetic -- double
    accumulation in key order -- runs as tensor operations, without a host read either.

result() is the only host read: one copy per print interval (after one all-reduce of the vector when
a process group is given)."""
import torch


def is_logged_key(key):
    """the reference's rule (train.py:358)"""
    return 'loss' in key or 'acc' in key or 'ratio' in key or 'value' in key


def logged_keys(end_points):
    return sorted(k for k, v in end_points.items()
                  if isinstance(k, str) and is_logged_key(k) and torch.is_tensor(v) and v.numel() == 1)


def tb_name(key):
    """train.py:292-302 (`grad_norm_value` files under value/)"""
    for tag in ('loss', 'acc', 'ratio', 'value'):
        if tag in key:
            return tag + '/' + key
    return 'other/' + key


class TrainMeter(object):
    def __init__(self, device, guarded=False):
        self.device = torch.device(device)
        self.guarded = bool(guarded)
        self.keys = None
        self.accum = None       # len(keys) + 3 doubles: the sums, steps, skipped steps, gradient norms
        self._table = None      # captured mode: device pointers of the static scalars
        self._pending = None
        self._stage = None
        self.host_reads = 0

    # ------------------------------------------------------------------ keys
    def prepare(self, end_points):
        """Pick the keys (first step, or the warm-up of a capture) and make the buffers."""
        keys = logged_keys(end_points)
        if self.keys is not None and keys != self.keys:
            raise RuntimeError("TrainMeter: the logged keys changed between steps: %s"
                               % sorted(set(keys) ^ set(self.keys)))
        if self.keys is None:
            self.keys = keys
            self.accum = torch.zeros(len(keys) + 3, dtype=torch.float64, device=self.device)
        return self.keys

    # ------------------------------------------------------------------ one step
    def add(self, end_points, guard=None):
        """The step's scalars into the sums; `guard`: the record of the guarded Adam step or None."""
        if guard is None and self.guarded:
            raise ValueError("TrainMeter.add: a guarded meter needs the guard record")
        keys = self.prepare(end_points)
        if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            return self._add_captured(end_points, guard)
        count = len(keys)
        values = torch.stack([end_points[k].detach().reshape(()).double() for k in keys]) \
            if count else torch.zeros(0, dtype=torch.float64, device=self.device)
        if guard is None:
            self.accum[:count] += values
            self.accum[count] += 1.0
            return
        skipped = guard[2] != 0
        zero = torch.zeros((), dtype=torch.float64, device=self.device)
        self.accum[:count] += torch.where(skipped, zero, values)
        self.accum[count] += torch.where(skipped, zero, zero + 1.0)
        self.accum[count + 1] += guard[2]
        self.accum[count + 2] += torch.where(skipped, zero, guard[0])

    def _add_captured(self, end_points, guard):
        import importlib
        _L = importlib.import_module("3dioumatch_amd._lib")
        count = len(self.keys)
        if self._table is None or self._table.numel() != max(count, 1):
            raise RuntimeError("TrainMeter: prepare() and bind_table() run outside the capture first")
        scalars, staged = [], 0
        for k in self.keys:
            t = end_points[k].detach()
            if t.dtype != torch.float32 or not t.is_cuda:
                self._stage[staged].copy_(t.reshape(()))
                t = self._stage[staged]
                staged += 1
            scalars.append(t)
        self._pending = scalars  # (kept: the table points into them)
        with torch.cuda.device(self.device):
            _L.check(_L.lib.votenet_train_meter_add(
                count, self._table.data_ptr(), None if guard is None else guard.data_ptr(),
                self.accum.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream),
                "votenet_train_meter_add")

    def bind_table(self, end_points):
        """Before a capture (from the warm-up's end_points): the table the captured launch reads."""
        keys = self.prepare(end_points)
        self._table = torch.zeros(max(len(keys), 1), dtype=torch.int64, device=self.device)
        odd = sum(1 for k in keys if end_points[k].dtype != torch.float32)
        self._stage = torch.zeros(max(odd, 1), dtype=torch.float32, device=self.device)
        self._pending = None

    def finish_capture(self):
        """After the capture: the addresses of the graph's static scalars into the table."""
        if self._pending is None:
            raise RuntimeError("TrainMeter: the capture did not reach the meter's launch")
        if self._pending:
            self._table.copy_(torch.tensor([t.data_ptr() for t in self._pending], dtype=torch.int64))
        self._static = self._pending

    # ------------------------------------------------------------------ read-out
    def reset(self):
        if self.accum is not None:
            self.accum.zero_()

    def result(self, reset=True, group=None):
        """{key: mean over the applied steps} + steps, skipped_steps (+ grad_norm_value with the
        guard).  The only host read; with `group` the sums of all ranks are added first."""
        if self.accum is None:
            raise ValueError("TrainMeter.result: no step was taken")
        vec = self.accum
        if group is not None:
            vec = vec.clone()
            torch.distributed.all_reduce(vec, group=group)
        host = vec.cpu().tolist()
        self.host_reads += 1
        if reset:
            self.accum.zero_()
        count = len(self.keys)
        steps = host[count]
        out = {k: (host[i] / steps if steps else float("nan")) for i, k in enumerate(self.keys)}
        if self.guarded:
            out["grad_norm_value"] = host[count + 2] / steps if steps else float("nan")
        out["steps"] = int(steps)
        out["skipped_steps"] = int(host[count + 1])
        return out
