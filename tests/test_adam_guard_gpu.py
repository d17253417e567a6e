"""votenet_adam_step_guarded through the C ABI on the MI355X (csrc/optim.hip): the device-side verdict in
front of the flat Adam step -- bit-equal to votenet_adam_step whenever it applies unclipped, nothing written
when an element of the gradient or the loss is not finite, torch.nn.utils.clip_grad_norm_ otherwise.

n covers one element, the float4 / tail split, one span of the partial-sum kernel less one, exactly, plus
one, several spans with a tail, and the detector's own size class (1e6)."""
import importlib
import math

import numpy as np
import pytest
import torch

from conftest import load_pkg
from dirty_memory import FILL_IDS, FILLS, poisoned
from test_gpu_mlp import close

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _lib():
    load_pkg()
    return importlib.import_module("3dioumatch_amd._lib")


def _span():
    return int(_lib().lib.votenet_adam_guard_span())


def _sizes():
    s = _span()
    return [1, 5, 1023, 1024, 1027, s - 1, s, s + 1, 3 * s + 7, 1000003]


# (the span is a property of the built library: read when the cases are made)
try:
    SIZES = _sizes()
except Exception:  # noqa: BLE001  -- no library: the tests below fail on their own import
    SIZES = [1, 5, 1023, 1024, 1027, 4095, 4096, 4097, 12295, 1000003]


class State(object):
    """p, m, v, step, lr, teacher, its weight and the scratch of one optimizer, on the device"""

    def __init__(self, n, teacher, seed=0):
        g = torch.Generator().manual_seed(seed + n)
        self.n = n
        self.p = torch.randn(n, generator=g).to(DEV)
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.step = torch.zeros((), device=DEV)
        self.lr = torch.tensor(2e-3, device=DEV)
        self.ema = self.p.clone() if teacher else None
        self.w = torch.tensor(0.25, device=DEV)
        self.scratch = torch.zeros(2, device=DEV)

    def clone(self):
        other = State.__new__(State)
        other.n = self.n
        for k, t in self.__dict__.items():
            if k != "n":
                setattr(other, k, None if t is None else t.clone())
        return other

    def tensors(self):
        return [t for t in (self.p, self.m, self.v, self.step, self.ema) if t is not None]


def bits_equal(a, b):
    """bit for bit (NaN payloads and the sign of zero included)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def plain(L, st, grad, grad_scale=1.0):
    L.check(L.lib.votenet_adam_step(st.n, st.p.data_ptr(), grad.data_ptr(), st.m.data_ptr(), st.v.data_ptr(),
                                    st.step.data_ptr(), st.lr.data_ptr(), 0.9, 0.999, 1e-8, 0.0, grad_scale,
                                    st.ema.data_ptr() if st.ema is not None else None,
                                    st.w.data_ptr() if st.ema is not None else None, st.scratch.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream), "votenet_adam_step")


class Guard(object):
    def __init__(self, L, n):
        self.rec = torch.zeros(4, dtype=torch.float64, device=DEV)
        self.count = int(L.lib.votenet_adam_guard_partials(n))
        # (uninitialised on purpose: the first launch writes every partial before the second reads one)
        self.partials = torch.empty(self.count, dtype=torch.float64, device=DEV)


def guarded(L, st, grad, guard, grad_scale=1.0, loss=None, max_norm=0.0):
    L.check(L.lib.votenet_adam_step_guarded(
        st.n, st.p.data_ptr(), grad.data_ptr(), st.m.data_ptr(), st.v.data_ptr(), st.step.data_ptr(),
        st.lr.data_ptr(), 0.9, 0.999, 1e-8, 0.0, grad_scale, st.ema.data_ptr() if st.ema is not None else None,
        st.w.data_ptr() if st.ema is not None else None, st.scratch.data_ptr(),
        None if loss is None else loss.data_ptr(), max_norm, guard.rec.data_ptr(), guard.partials.data_ptr(),
        torch.cuda.current_stream().cuda_stream), "votenet_adam_step_guarded")


def norm64(grad, grad_scale):
    """sqrt of the exactly summed squares of the float32 products g * grad_scale"""
    scaled = (grad * grad_scale).cpu().numpy().astype(np.float64)
    return math.sqrt(math.fsum((scaled * scaled).tolist()))


def test_partial_count_and_span():
    L = _lib()
    s = _span()
    assert s > 0 and s % 1024 == 0  # whole float4 rounds of a 256-lane workgroup
    for n in SIZES:
        assert L.lib.votenet_adam_guard_partials(n) == -(-n // s)
    assert L.lib.votenet_adam_guard_partials(0) == 0
    assert SIZES == _sizes()


@pytest.mark.parametrize("n", SIZES)
def test_finite_gradients_are_the_unguarded_step(n):
    L = _lib()
    for teacher in (False, True):
        for grad_scale in (1.0, 0.5):
            a = State(n, teacher)
            b = a.clone()
            guard = Guard(L, n)
            g = torch.Generator().manual_seed(n + 7)
            for it in range(4):  # as test_flat_adam_step_matches_torch
                grad = (torch.randn(n, generator=g) * (10.0 ** (it - 2))).to(DEV)
                if it == 2:
                    a.lr.fill_(5e-4)
                    b.lr.fill_(5e-4)
                a.w.fill_(1.0 - min(1 - 1 / (it + 1), 0.999))
                b.w.copy_(a.w)
                ga, gb = grad.clone(), grad.clone()
                plain(L, a, ga, grad_scale)
                guarded(L, b, gb, guard, grad_scale, loss=torch.tensor(1.0, device=DEV))
                for x, y in zip(a.tensors() + [ga], b.tensors() + [gb]):
                    assert bits_equal(x, y), (teacher, grad_scale, it)
                rec = guard.rec.cpu().tolist()
                want = norm64(grad, grad_scale)
                print("n %d it %d norm %.17g want %.17g" % (n, it, rec[0], want))
                assert abs(rec[0] - want) <= n * 2.0 ** -53 * want
                assert rec[1:] == [1.0, 0.0, 0.0]
            assert float(b.step) == 4.0


def _bad_positions(n):
    s = _span()
    at = {0, n - 1, s - 1, s}
    if n % 4:
        at.add((n // 4) * 4)  # the first element of the tail
    return sorted(i for i in at if 0 <= i < n)


@pytest.mark.parametrize("n", SIZES)
def test_non_finite_step_writes_nothing(n):
    L = _lib()
    g = torch.Generator().manual_seed(n + 11)
    st = State(n, teacher=True)
    guard = Guard(L, n)
    first = (torch.randn(n, generator=g) * 0.1).to(DEV)
    guarded(L, st, first.clone(), guard, 0.5)  # moments and step are no longer zero
    finite = (torch.randn(n, generator=g) * 0.1).to(DEV)
    ok_loss = torch.tensor(2.5, device=DEV)
    cases = [(i, bad, ok_loss) for i in _bad_positions(n) for bad in (float("nan"), float("inf"), -float("inf"))]
    cases += [(None, None, torch.tensor(v, device=DEV)) for v in (float("inf"), float("nan"))]
    skipped = 0
    for at, bad, loss in cases:
        grad = finite.clone()
        if at is not None:
            grad[at] = bad
        before, grad_before = [t.clone() for t in st.tensors()], grad.clone()
        guarded(L, st, grad, guard, 0.5, loss=loss)
        skipped += 1
        for x, y in zip(before + [grad_before], st.tensors() + [grad]):
            assert bits_equal(x, y), (at, bad, float(loss))
        rec = guard.rec.cpu().tolist()
        assert rec[2] == 1.0 and rec[3] == float(skipped), (at, bad, rec)
        assert float(st.step) == 1.0
    # a finite call behind the skipped ones applies, with t advanced by one only
    twin = st.clone()
    ga, gb = finite.clone(), finite.clone()
    plain(L, twin, ga, 0.5)
    guarded(L, st, gb, guard, 0.5, loss=ok_loss)
    for x, y in zip(twin.tensors() + [ga], st.tensors() + [gb]):
        assert bits_equal(x, y)
    assert float(st.step) == 2.0
    rec = guard.rec.cpu().tolist()
    assert rec[2] == 0.0 and rec[3] == float(skipped)


@pytest.mark.parametrize("n", [n for n in SIZES if n >= 5])
def test_two_huge_entries_do_not_skip(n):
    """3e38 squared twice is finite in the double sum and its root is above the float range"""
    L = _lib()
    g = torch.Generator().manual_seed(n + 13)
    a = State(n, teacher=True)
    b = a.clone()
    guard = Guard(L, n)
    grad = torch.randn(n, generator=g).to(DEV)
    grad[1], grad[n - 2] = 3e38, -3e38
    ga, gb = grad.clone(), grad.clone()
    plain(L, a, ga)
    guarded(L, b, gb, guard, loss=torch.tensor(0.5, device=DEV))
    for x, y in zip(a.tensors() + [ga], b.tensors() + [gb]):
        assert bits_equal(x, y)
    rec = guard.rec.cpu().tolist()
    assert rec[2] == 0.0 and rec[3] == 0.0 and float(b.step) == 1.0
    assert 3.4e38 < rec[0] < float("inf") and abs(rec[0] - norm64(grad, 1.0)) <= n * 2.0 ** -53 * rec[0]


@pytest.mark.parametrize("teacher", [False, True], ids=["plain", "ema"])
@pytest.mark.parametrize("n", SIZES)
def test_clipping_matches_clip_grad_norm(n, teacher):
    """== clip_grad_norm_ + torch.optim.Adam + lerp_ (in float64: the reference adds no rounding of its own,
    neither to the norm nor to the coefficient), the gradient 1/world-scaled first; steps 0 and 1 stay under
    max_norm, steps 2 and 3 are clipped."""
    L = _lib()
    world = 2
    max_norm = 0.3 * math.sqrt(n) / world
    g = torch.Generator().manual_seed(n + 17)
    st = State(n, teacher)
    guard = Guard(L, n)
    ref = st.p.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=2e-3)
    ema_ref = st.p.double().clone()
    clipped = []
    for it in range(4):
        grad = (torch.randn(n, generator=g) * (10.0 ** (it - 2))).to(DEV)
        if it == 2:
            st.lr.fill_(5e-4)
            opt.param_groups[0]["lr"] = 5e-4
        st.w.fill_(1.0 - min(1 - 1 / (it + 1), 0.999))
        ref.grad = grad.double() / world
        torch.nn.utils.clip_grad_norm_([ref], max_norm)
        opt.step()
        ema_ref.lerp_(ref.data, st.w.double())
        norm = norm64(grad, 1.0 / world)
        guarded(L, st, grad, guard, 1.0 / world, loss=None, max_norm=max_norm)  # (rewrites grad)
        rec = guard.rec.cpu().tolist()
        want = min(1.0, max_norm / (norm + 1e-6))
        print("n %d it %d norm %.17g coefficient %.17g want %.17g" % (n, it, rec[0], rec[1], want))
        assert abs(rec[0] - norm) <= n * 2.0 ** -53 * norm
        assert abs(rec[1] - want) <= (n + 4) * 2.0 ** -53 * want and rec[2] == 0.0
        clipped.append(rec[1] < 1.0)
        close(grad, ref.grad, 1e-7)  # rewritten with the value used
    assert clipped == [False, False, True, True] or n < 1000  # (a handful of draws: the norms scatter)
    assert float(st.step) == 4.0
    close(st.p, ref.data, 2e-6)
    close(st.m, opt.state[ref]["exp_avg"], 2e-6)
    close(st.v, opt.state[ref]["exp_avg_sq"], 2e-6)
    if teacher:
        close(st.ema, ema_ref, 2e-6)


@pytest.mark.parametrize("n", SIZES)
def test_repeat_launches_give_equal_bits(n):
    L = _lib()
    g = torch.Generator().manual_seed(n + 19)
    grad = torch.randn(n, generator=g).to(DEV)
    outs = []
    for _ in range(2):
        st = State(n, teacher=False)
        guard = Guard(L, n)
        guarded(L, st, grad.clone(), guard, 0.5, max_norm=1.0)
        outs.append((guard.rec.clone(), guard.partials.clone(), st.p.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert bits_equal(outs[0][2], outs[1][2])


def _sequence(L, n):
    """a clipped step, a skipped one, an applied one -- every buffer the entry only writes from torch.empty"""
    g = torch.Generator().manual_seed(n + 23)
    st = State(n, teacher=True)
    st.scratch = torch.empty(2, device=DEV)
    guard = Guard(L, n)
    out = []
    for it in range(3):
        grad = torch.randn(n, generator=g).to(DEV)
        if it == 1:
            grad[n // 2] = float("inf")
        guarded(L, st, grad, guard, 0.5, loss=torch.tensor(1.0, device=DEV), max_norm=1.0)
        out += [t.clone() for t in st.tensors()] + [grad, guard.rec.clone(), guard.partials.clone()]
    return out


@pytest.mark.parametrize("n", [1027, 1000003])
def test_poisoned_allocations_change_nothing(n):
    L = _lib()
    clean = _sequence(L, n)
    for fill, name in zip(FILLS, FILL_IDS):
        with poisoned(fill) as record:
            dirty = _sequence(L, n)
        assert record.count >= 2, name  # the partial sums and the scratch arrived filled
        for i, (x, y) in enumerate(zip(clean, dirty)):
            same = torch.equal(x.view(torch.int64), y.view(torch.int64)) if x.dtype == torch.float64 \
                else bits_equal(x, y)
            assert same, (name, i)
