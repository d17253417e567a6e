"""pointnet2.pytorch_utils -- shared-MLP building blocks (host-side mirror).

Public names, constructor arguments and the MODULE TREE (hence state_dict keys such as
`layer0.conv.weight`, `layer0.bn.bn.running_mean`) follow the reference
pointnet2/pytorch_utils.py:14-39 (SharedMLP), :42-67 (BatchNorm wrappers), :70-124
(_ConvBase), :127-236 (Conv1d/2d/3d), :239-270 (FC), :272-299 (BN momentum scheduler), so
checkpoints are interchangeable.  The implementation is written fresh around one builder.
"""
import contextlib
import os

import torch
import torch.nn as nn
from torch.autograd import Function


class _BNBase(nn.Sequential):
    """A batch-norm layer wrapped in a Sequential under the child name `<name>bn`
    (weight 1, bias 0), as the reference does at pytorch_utils.py:42-50."""

    def __init__(self, in_size, batch_norm=None, name=""):
        super().__init__()
        layer = batch_norm(in_size)
        nn.init.constant_(layer.weight, 1.0)
        nn.init.constant_(layer.bias, 0)
        self.add_module(name + "bn", layer)


class BatchNorm1d(_BNBase):
    def __init__(self, in_size, *, name=""):
        super().__init__(in_size, batch_norm=nn.BatchNorm1d, name=name)


class BatchNorm2d(_BNBase):
    def __init__(self, in_size, name=""):
        super().__init__(in_size, batch_norm=nn.BatchNorm2d, name=name)


class BatchNorm3d(_BNBase):
    def __init__(self, in_size, name=""):
        super().__init__(in_size, batch_norm=nn.BatchNorm3d, name=name)


def _assemble(seq, name, core_name, core, bn_unit, activation, preact):
    """Order the (bn, activation, core) children: pre-activation puts bn/act first."""
    tail = []
    if bn_unit is not None:
        tail.append((name + "bn", bn_unit))
    if activation is not None:
        tail.append((name + "activation", activation))
    parts = tail + [(name + core_name, core)] if preact else [(name + core_name, core)] + tail
    for child_name, child in parts:
        seq.add_module(child_name, child)


class _ConvBase(nn.Sequential):
    """conv (bias only without bn) [+ bn] [+ activation]; kaiming-normal weights by default."""

    def __init__(self, in_size, out_size, kernel_size, stride, padding, activation, bn, init,
                 conv=None, batch_norm=None, bias=True, preact=False, name=""):
        super().__init__()
        use_bias = bias and (not bn)
        conv_unit = conv(in_size, out_size, kernel_size=kernel_size, stride=stride,
                         padding=padding, bias=use_bias)
        init(conv_unit.weight)
        if use_bias:
            nn.init.constant_(conv_unit.bias, 0)
        bn_unit = batch_norm(in_size if preact else out_size) if bn else None
        _assemble(self, name, "conv", conv_unit, bn_unit, activation, preact)


def _conv_class(conv, batch_norm, ones):
    class _Conv(_ConvBase):
        def __init__(self, in_size, out_size, *, kernel_size=ones, stride=ones,
                     padding=tuple(0 for _ in ones) if isinstance(ones, tuple) else 0,
                     activation=nn.ReLU(inplace=True), bn=False, init=nn.init.kaiming_normal_,
                     bias=True, preact=False, name=""):
            super().__init__(in_size, out_size, kernel_size, stride, padding, activation, bn,
                             init, conv=conv, batch_norm=batch_norm, bias=bias, preact=preact,
                             name=name)
    return _Conv


Conv1d = _conv_class(nn.Conv1d, BatchNorm1d, 1)
Conv1d.__name__ = Conv1d.__qualname__ = "Conv1d"
Conv2d = _conv_class(nn.Conv2d, BatchNorm2d, (1, 1))
Conv2d.__name__ = Conv2d.__qualname__ = "Conv2d"
Conv3d = _conv_class(nn.Conv3d, BatchNorm3d, (1, 1, 1))
Conv3d.__name__ = Conv3d.__qualname__ = "Conv3d"


class _BNReLU(Function):
    """z = relu(batch_norm(y)) with the fused gfx950 kernels (pointnet2._mlp_ext).  Saves y and
    four per-channel vectors; the ReLU mask and x-hat are recomputed in the backward."""

    @staticmethod
    def forward(ctx, y, gamma, beta, running_mean, running_var, momentum, eps, training, tickets=None):
        from pointnet2 import _mlp_ext as K
        y = y.contiguous()
        mean, invstd, scale, shift = K.bn_coefficients(y, gamma, beta, running_mean, running_var,
                                                       momentum, eps, training, tickets)
        ctx.save_for_backward(y, gamma, scale, shift, mean, invstd)
        ctx.training, ctx.tickets = training, tickets
        return K.bn_relu_apply(y, scale, shift)

    @staticmethod
    def backward(ctx, dz):
        from pointnet2 import _mlp_ext as K
        y, gamma, scale, shift, mean, invstd = ctx.saved_tensors
        dy, dgamma, dbeta = K.bn_relu_backward(y, dz.contiguous(), gamma, scale, shift, mean,
                                               invstd, ctx.training, ctx.tickets)
        return dy, dgamma, dbeta, None, None, None, None, None, None


class _BNReLUMaxPool(Function):
    """(B,C,m,ns) -> (B,C,m): max over nsample of relu(batch_norm(y)) in one pass."""

    @staticmethod
    def forward(ctx, y, gamma, beta, running_mean, running_var, momentum, eps, training, tickets=None):
        from pointnet2 import _mlp_ext as K
        y = y.contiguous()
        mean, invstd, scale, shift = K.bn_coefficients(y, gamma, beta, running_mean, running_var,
                                                       momentum, eps, training, tickets)
        pooled, argmax, ymax = K.bn_relu_pool(y, scale, shift)
        ctx.save_for_backward(y, gamma, scale, shift, mean, invstd, argmax, ymax)
        ctx.training, ctx.tickets = training, tickets
        return pooled

    @staticmethod
    def backward(ctx, dpooled):
        from pointnet2 import _mlp_ext as K
        y, gamma, scale, shift, mean, invstd, argmax, ymax = ctx.saved_tensors
        dy, dgamma, dbeta = K.bn_relu_pool_backward(y, dpooled.contiguous(), argmax, ymax, gamma,
                                                    scale, shift, mean, invstd, ctx.training, ctx.tickets)
        return dy, dgamma, dbeta, None, None, None, None, None, None


class Pregathered(object):
    """Layer 0 applied BEFORE the gather (csrc/mlp_pregather.hip): the chain's input is then the packed
    point-major operand src_ext (B, 3+C, n+m) of _mlp_ext.pregather_pack instead of the grouped tensor
    (B, 3+C, m, ns), which is never formed: y_0 = (W_0 . src_ext)[.., idx] - (W_0 . src_ext)[.., n + j].
    idx (B,m,ns) int32; inverse = its _ext.group_inverse, or None where no gradient is expected."""

    def __init__(self, idx, inverse, n):
        self.idx, self.inverse, self.n = idx, inverse, n
        self.extent = tuple(idx.shape)  # (B, m, ns) of layer 0's output

    def forward(self, w, x, bn=None):
        """y_0; with bn = (gamma, beta, running_mean, running_var, momentum, eps) also its training-mode
        (mean, invstd, scale, shift): the gather kernel leaves the rows' moments behind."""
        from pointnet2 import _mlp_ext as K
        z = K.gemm_forward(w, x)  # over the n + m points, not the m * ns gathered columns
        return K.pregather_forward(z, self.idx, self.n, bn)

    def backward(self, w, x, fly, need_dx):
        """(dw, dx) of layer 0: the BatchNorm / ReLU backward of fly = (y_0, dz, ...) formed on the fly,
        scatter-added over idx and summed per group; then two GEMMs over the n + m points."""
        from pointnet2 import _ext
        from pointnet2 import _mlp_ext as K
        inverse = self.inverse
        if inverse is None:  # forward ran without it (no gradient expected then): build it now
            inverse = _ext.group_inverse(self.idx, self.n)
        return K.both(w, x, need_dx=need_dx, dy=K.pregather_backward(fly, inverse, self.n))


class Interpolated(object):
    """Layer 0 commuted with a three-point interpolation: its input cat([rel (3 rows),
    three_interpolate(x, idx, weight)]) over n >> m queries is not formed -- the GEMM runs over the m
    source points x (B,C,m), then ONE kernel interpolates its output and adds the coordinate rows'
    part.  idx / weight (B,n,3), rel (B,3,n); shape = (B, c, npoint, nsample) of layer 0's output,
    n = npoint * nsample.  x carries no gradient (SharedMLP.interp_first_ok)."""

    def __init__(self, idx, weight, rel, shape):
        self.idx, self.weight, self.rel, self.shape = idx, weight, rel, shape
        self.extent = (shape[0], shape[2], shape[3])

    def forward(self, w, x):
        from pointnet2 import _ext
        from pointnet2 import _mlp_ext as K
        # (both column slices of w are read in place)
        z = K.gemm_forward(w[:, 3:], x)
        y = _ext.three_interpolate_affine(z, self.idx, self.weight, w[:, :3], self.rel)
        return y.view(self.shape)

    def input(self, x):
        """The layer's real input (B, 3+C, npoint, nsample), for its weight gradient: formed once, in
        the backward pass."""
        from pointnet2 import _ext
        b, c = x.shape[0], 3 + x.shape[1]
        feats = torch.empty((b, c, self.rel.shape[2]), dtype=torch.float32, device=x.device)
        _ext.three_interpolate_rows_into(x, self.idx, self.weight, feats, 3, self.rel, 0)
        return feats.view(b, c, self.shape[2], self.shape[3])


def chain_forms(ws, x, pre, pool, training, input_grad):
    """(first, last): the forms _FusedMLPChain runs its first and last layers in, from host-side
    shape gates only.  ws: the layers' weights as (out, in) matrices; x, pre as the chain takes them.
    first: "plain"; "pregathered" / "interpolated" (pre); "virtual": a 4 -> 64 first layer followed
    by 64 -> 64 (SA1) is never stored -- its output is a rank-4 function of x, so its BatchNorm
    statistics follow from the second moments of x and every kernel that needs a row of it recomputes
    that row (four FMAs per element) instead of a 268 MB tensor being written once and read three
    times; "chained": virtual, and layers 1 + 2 (64 -> 64 -> 128, max-pooled) as ONE register-chained
    kernel (csrc/mlp_chain.hip) -- layer 1's activation never leaves the registers, statistics and
    pooled extrema are in-lane reductions of the second GEMM's accumulators.
    last: "apply" (no pool); "bn_relu_pool" over the stored raw output; "extrema": the per-group
    extrema the max over nsample needs come out of the GEMM epilogue; "gram": so do they, and the raw
    output is not stored -- its backward runs from the Gram matrix of the layer's input
    (csrc/mlp_pool_gram.hip, csrc/mlp_pool_gram256.hip: 537 MB at SA1, 268 MB at SA2)."""
    from pointnet2 import _mlp_ext as K
    n = len(ws)
    if pre is not None and (n < 2 or x.dim() != 3):
        raise RuntimeError("the pre-gather form needs src_ext (B, 3+C, n+m) and two layers or more")
    first = "plain"
    if isinstance(pre, Pregathered):
        first = "pregathered"
    elif isinstance(pre, Interpolated):
        first = "interpolated"
    elif training and n >= 3 and x.dim() == 4 and not input_grad and K.lin4_supported(ws[0], ws[1], x):
        chained = pool and n == 3 and K.chain_lin4_supported(ws[0], ws[1], ws[2], x, x.shape[3])
        first = "chained" if chained else "virtual"
    if not pool:
        return first, "apply"
    b, m, ns = pre.extent if pre is not None else (x.shape[0], x.shape[2], x.shape[3])
    y_in = (b, ws[-1].shape[1], m, ns)  # the last layer's input
    if first == "chained":
        return first, "gram" if K.pool_gram_supported(ws[2], y_in, ns) else "extrema"
    if not (training and n >= 2 and K.forward_pool_supported(ws[-1], y_in, True)):
        return first, "bn_relu_pool"
    return first, "gram" if K.pool_gram_supported(ws[-1], y_in, ns) else "extrema"


class _FusedMLPChain(Function):
    """The whole conv(1x1)+BN+ReLU stack (and optionally the final max over nsample) as ONE
    autograd node on the gfx950 kernels: MFMA GEMMs whose operand loads apply the previous
    layer's BatchNorm+ReLU (forward) or form the BatchNorm/ReLU backward of the incoming
    gradient (backward) on the fly.  Per layer only the raw GEMM output y_i is kept; no
    normalised / rectified activation and no mask is ever written to memory.

    apply(x, pool, training, momenta, epss, pre, tickets, w_0, g_0, b_0, rm_0, rv_0, w_1, ...)

    tickets = the module's counters for the one-launch reductions (_mlp_ext.tickets_of; None: a
    fresh zeroed array per reduction).
    pre = None, or the Pregathered / Interpolated form of layer 0's input (x is then that form's
    operand).  chain_forms decides how the first and last layers run; the backward follows the
    recorded decision."""

    @staticmethod
    def forward(ctx, x, pool, training, momenta, epss, pre, tickets, *params):
        from pointnet2 import _mlp_ext as K
        n = len(params) // 5
        x = x.contiguous()
        ws = [w.reshape(w.shape[0], -1) for w in params[0::5]]
        bns = [tuple(params[5 * i + 1:5 * i + 5]) + (momenta[i], epss[i]) for i in range(n)]
        first, last = chain_forms(ws, x, pre, pool, training, ctx.needs_input_grad[0])
        # a pass that no backward follows (the EMA teacher, evaluation in training mode) stores no raw
        # output it can do without
        store = any(ctx.needs_input_grad)
        ys, coefs = [], []  # raw output (None: not stored), (mean, invstd, scale, shift) per layer
        moments, ext = None, None
        if first in ("virtual", "chained"):
            moments = K.first4_moments(x)
            ys.append(None)
            coefs.append(K.first4_bn(moments, x.numel() // 4, ws[0], *bns[0]))
        if first == "chained":
            y1, c1, y2, c2, ext = K.chain_lin4_forward(x, ws[0], coefs[0][2:], (ws[1],) + bns[1],
                                                       (ws[2],) + bns[2], store=store, store_last=last != "gram")
            ys += [y1, y2]
            coefs += [c1, c2]
        elif first == "virtual":
            y, *c = K.gemm_forward_bn_lin4(ws[1], x, ws[0], coefs[0][2:], *bns[1])
            ys.append(y)
            coefs.append(tuple(c))
        elif first == "pregathered" and training:
            y, *c = pre.forward(ws[0], x, bns[0])
            ys.append(y)
            coefs.append(tuple(c))
        elif pre is not None:
            ys.append(pre.forward(ws[0], x))
            coefs.append(K.bn_coefficients(ys[0], *bns[0], training, tickets))
        for i in range(len(ys), n):
            cur, coeff = (x, None) if i == 0 else (ys[i - 1], coefs[i - 1][2:])
            if i == n - 1 and last in ("extrema", "gram"):
                y, *c, ext = K.gemm_forward_bn(ws[i], cur, coeff, *bns[i], pool=True, tickets=tickets,
                                               store=store and last == "extrema")
            elif training:  # batch statistics come out of the GEMM epilogue where the shape allows
                y, *c = K.gemm_forward_bn(ws[i], cur, coeff, *bns[i], tickets=tickets)
            else:
                y = K.gemm_forward(ws[i], cur, coeff)
                c = K.bn_coefficients(y, *bns[i], False, tickets)
            ys.append(y)
            coefs.append(tuple(c))
        scale, shift = coefs[-1][2:]
        argmax = ymax = None
        if last == "apply":
            out = K.bn_relu_apply(ys[-1], scale, shift)
        elif last == "bn_relu_pool":
            out, argmax, ymax = K.bn_relu_pool(ys[-1], scale, shift)
        else:
            out, argmax, ymax = K.pool_from_extrema(ext, scale, shift)
        ctx.save_for_backward(x, moments, argmax, ymax, *ys, *[t for c in coefs for t in c], *params)
        ctx.n_layers, ctx.training, ctx.tickets, ctx.pre = n, training, tickets, pre
        ctx.first, ctx.last = first, last
        return out

    @staticmethod
    def backward(ctx, dout):
        from pointnet2 import _mlp_ext as K
        n, training, tickets, first, last = ctx.n_layers, ctx.training, ctx.tickets, ctx.first, ctx.last
        x, moments, argmax, ymax, *rest = ctx.saved_tensors
        ys, rest = rest[:n], rest[n:]
        coefs, params = [tuple(rest[4 * i:4 * i + 4]) for i in range(n)], rest[4 * n:]
        ws = [w.reshape(w.shape[0], -1) for w in params[0::5]]
        if first == "interpolated":
            # the layer's weight gradient needs its real input: formed here, once, instead of in the
            # forward pass
            x = ctx.pre.input(x)
        need_dx, virtual = ctx.needs_input_grad[0], first in ("virtual", "chained")
        grads = [None] * (5 * n)
        dz, below = dout.contiguous(), None
        for i in range(n - 1, -1, -1):
            gamma = params[5 * i + 1]
            mean, invstd, scale, shift = coefs[i]
            if i == n - 1 and last == "gram":
                # the layer's raw output does not exist: both products of its backward from the Gram
                # matrix of its input and one sparse column per (channel, group)
                ns = ys[i - 1].shape[3]
                dgamma, dbeta, coef = K.bn_relu_pool_backward_stats(None, dz, argmax, ymax, gamma, scale, shift,
                                                                    mean, invstd, training, ns=ns,
                                                                    tickets=tickets)
                dz, dw, below = K.pool_gram_backward(ws[i], ys[i - 1], coefs[i - 1], params[5 * i - 4], coef,
                                                     coefs[i], dz, argmax, ymax, ns, training)
                grads[5 * i:5 * i + 3] = dw.view_as(params[5 * i]), dgamma, dbeta
                continue
            if i == 0 and virtual:
                # the layer above never wrote the gradient w.r.t. this layer's output: its one-pass
                # backward left the gated sums (dz) the weight gradient needs, and the BatchNorm sums
                dgamma, dbeta, coef = below
                dw = K.wgrad_first4_from_gated(ws[0], dz, mean, invstd, coef, moments)
                grads[0:3] = dw.view_as(params[0]), dgamma, dbeta
                break
            if i == n - 1 and last != "apply":
                # dz of the pooled layer is one value per (channel, group): the GEMM operand
                # loads rebuild dy from y, dpooled and the arg-max, nothing dense is written
                dgamma, dbeta, coef = K.bn_relu_pool_backward_stats(ys[i], dz, argmax, ymax, gamma, scale, shift,
                                                                    mean, invstd, training, tickets=tickets)
                grad = dict(pooled=(ys[i], dz, argmax, scale, shift, mean, invstd, coef))
            elif below is not None or (i == 0 and first == "pregathered"):
                # the sums left behind by the fused backward GEMM of layer i+1; or the pre-gather layer,
                # whose dy is never written (pregather_backward forms it on the fly)
                dgamma, dbeta, coef = below if below is not None else K.bn_relu_backward_stats(
                    ys[i], dz, gamma, scale, shift, mean, invstd, training, tickets)
                grad = dict(fly=(ys[i], dz, scale, shift, mean, invstd, coef))
            else:
                dgamma, dbeta, coef, grad = K.through_bn(ws[i], ys[i], dz, gamma, scale, shift, mean, invstd,
                                                         training, tickets)
            grads[5 * i + 1:5 * i + 3] = dgamma, dbeta
            if i == 0 and first == "pregathered":
                dw, dz = ctx.pre.backward(ws[0], x, grad["fly"], need_dx)
                grads[0] = dw.view_as(params[0])
                break
            lin_w = ws[0] if (i == 1 and virtual) else None
            src = x if (i == 0 or lin_w is not None) else ys[i - 1]
            src_coeff = None if i == 0 else coefs[i - 1][2:]
            src_stats = None if i == 0 else coefs[i - 1][:2] + (params[5 * i - 4], training)
            # both GEMMs from one pass over (y_i, dz) where the shape allows
            fused = None if "dy" in grad else K.gemm_backward_fused(
                ws[i], src, src_coeff, xstats=src_stats, need_dx=i > 0 or need_dx, lin_w=lin_w, **grad)
            if fused is not None:
                dsrc, dw, below = fused  # below: BatchNorm-backward sums of layer i-1
            elif lin_w is not None:
                raise RuntimeError("the virtual first layer needs the fused backward kernel of the second")
            elif i == 0 and not need_dx:  # the weight gradient alone
                dsrc, below = None, None
                dw = K.wgrad_first4(ws[0], x, grad["fly"]) if "fly" in grad else None
                if dw is None:
                    dw = K.gemm_wgrad(ws[0].shape[0], ws[0].shape[1], x, None, **grad)
            else:
                (dw, dsrc), below = K.both(ws[i], src, src_coeff, **grad), None
            grads[5 * i] = dw.view_as(params[5 * i])
            dz = dsrc  # gradient w.r.t. relu(bn(y_{i-1})) (the gated sums for a virtual layer 0), or dx
        return (dz if need_dx else None, None, None, None, None, None, None, *grads)


_deferred_counters = None
_deferred_axpy = None   # (tensor, other, alpha): tensor += alpha * other, applied at context exit
# inside deferred_bn_counters() a gradient that is identically zero (the bias of a convolution that
# feeds a training-mode BatchNorm) may be returned as None instead of a freshly zeroed tensor:
# the train step's gradient packing substitutes zeros (votenet/step.py:_pack_gradients)
zero_grads_as_none = False


@contextlib.contextmanager
def deferred_bn_counters():
    """Inside this context the fused layers collect their `num_batches_tracked += 1` updates (and
    the running-mean corrections `rm += momentum * bias` of the head chains) and apply them with
    ONE multi-tensor add each at exit (37 + 6 one-element / one-row kernels per forward otherwise)."""
    global _deferred_counters, _deferred_axpy
    previous, _deferred_counters = _deferred_counters, []
    previous_axpy, _deferred_axpy = _deferred_axpy, []
    try:
        yield
    finally:
        pending, _deferred_counters = _deferred_counters, previous
        axpy, _deferred_axpy = _deferred_axpy, previous_axpy
        if pending:
            torch._foreach_add_(pending, 1)
        by_alpha = {}
        for t, other, alpha in axpy:
            by_alpha.setdefault(float(alpha), ([], []))
            by_alpha[float(alpha)][0].append(t)
            by_alpha[float(alpha)][1].append(other)
        for alpha, (ts, others) in by_alpha.items():
            torch._foreach_add_(ts, others, alpha=alpha)


@contextlib.contextmanager
def zero_grads_none():
    """Run a backward pass with `zero_grads_as_none` set (the caller packs the gradients itself
    and treats a missing one as zeros)."""
    global zero_grads_as_none
    previous, zero_grads_as_none = zero_grads_as_none, True
    try:
        yield
    finally:
        zero_grads_as_none = previous


def deferred_axpy(tensor, other, alpha):
    """tensor += alpha * other, now or -- inside deferred_bn_counters() -- batched at its exit
    (nothing reads `tensor`, a BatchNorm running mean, before then)."""
    if _deferred_axpy is not None:
        _deferred_axpy.append((tensor, other.detach(), alpha))
    else:
        tensor.add_(other.detach(), alpha=alpha)


def bump_batches_tracked(counter):
    if _deferred_counters is not None:
        _deferred_counters.append(counter)
    else:
        counter.add_(1)


class SharedMLP(nn.Sequential):
    """Stack of 1x1 Conv2d (+BN+ReLU) layers `layer0..layerK` applied to a (B, C, npoint,
    nsample) tensor: the grouped shared MLP of a set-abstraction layer.

    Same module tree as the reference (pytorch_utils.py:14-39).  On the GPU, layers of the
    standard shape conv(1x1, no bias) -> BatchNorm2d -> ReLU run their BatchNorm/ReLU (and, via
    forward_pooled, the max-pool over nsample that follows the last layer in every SA module)
    through the fused kernels of pointnet2._mlp_ext; any other configuration, and CPU tensors,
    use the plain torch modules."""

    def __init__(self, args, *, bn=False, activation=nn.ReLU(inplace=True), preact=False,
                 first=False, name=""):
        super().__init__()
        for i in range(len(args) - 1):
            plain = first and preact and i == 0  # first pre-act layer: no bn / activation
            self.add_module(
                name + "layer{}".format(i),
                Conv2d(args[i], args[i + 1], bn=bn and not plain,
                       activation=None if plain else activation, preact=preact))

    @staticmethod
    def _fusable(layer):
        kids = dict(layer.named_children())
        if set(kids) != {"conv", "bn", "activation"} or list(kids)[0] != "conv":
            return False
        conv, bn_wrap, act = kids["conv"], kids["bn"], kids["activation"]
        bns = list(bn_wrap.children())
        return (isinstance(conv, nn.Conv2d) and conv.kernel_size == (1, 1) and conv.bias is None
                and conv.stride == (1, 1) and conv.padding == (0, 0) and len(bns) == 1
                and isinstance(bns[0], nn.BatchNorm2d) and bns[0].affine
                and bns[0].track_running_stats and bns[0].momentum is not None
                and isinstance(act, nn.ReLU))

    def _use_fused(self, x):
        return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and len(self) > 0
                and all(self._fusable(layer) for layer in self))

    def _run(self, x, pool, pre=None):
        from pointnet2 import _mlp_ext as K
        if _eval_plans is not None and pool:  # only inside fused_eval(): the inference engine
            plan = _eval_plans.get(id(self))
            if plan is not None and plan.mlp is self:
                out = plan.run(x, pre)
                if out is not None:
                    return out
        layers = list(self)
        # the module's own counters for the one-launch reductions of its layers (include/mlp_hip.h
        # `tickets`): nothing in the library is keyed by stream
        tickets = K.tickets_of(self, max(layer.conv.out_channels for layer in layers), x.device)
        bns = [next(layer.bn.children()) for layer in layers]
        training = bns[0].training
        if all(bn.training == training for bn in bns):
            params = []
            for layer, bn in zip(layers, bns):
                if training:
                    bump_batches_tracked(bn.num_batches_tracked)
                params += [layer.conv.weight, bn.weight, bn.bias, bn.running_mean,
                           bn.running_var]
            return _FusedMLPChain.apply(x, pool, training, [bn.momentum for bn in bns],
                                        [bn.eps for bn in bns], pre, tickets, *params)
        # (mixed train / eval BatchNorm: layer by layer)
        for i, layer in enumerate(layers):
            bn = next(layer.bn.children())
            y = layer.conv(x)
            training = bn.training
            if training:
                bump_batches_tracked(bn.num_batches_tracked)
            op = _BNReLUMaxPool if (pool and i == len(layers) - 1) else _BNReLU
            x = op.apply(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.momentum,
                         bn.eps, training, tickets)
        return x

    def forward(self, x):
        if self._use_fused(x):
            return self._run(x, pool=False)
        return super().forward(x)

    def pregather_ok(self, xyz, new_xyz, features, m, ns):
        """Can forward_pregathered replace forward_pooled(grouped) for these inputs (m groups of
        ns members)?"""
        if features is None or len(self) < 2:
            return False
        if not (features.is_cuda and features.dtype == torch.float32
                and all(self._fusable(layer) for layer in self)):
            return False
        bns = [next(layer.bn.children()) for layer in self]
        if any(bn.training != bns[0].training for bn in bns):
            return False
        from pointnet2 import _mlp_ext as K
        conv = self[0].conv
        return (conv.in_channels == features.shape[1] + 3 and
                K.pregather_supported(features.shape[0], conv.out_channels, xyz.shape[1], m, ns))

    def forward_pregathered(self, xyz, new_xyz, features, idx, inverse, scale):
        """forward_pooled of the grouped tensor [(xyz[idx] - new_xyz) * scale ; features[idx]]
        WITHOUT forming it: the first layer runs before the gather (csrc/mlp_pregather.hip).
        xyz (B,N,3), new_xyz (B,m,3), features (B,C,N), idx (B,m,ns) int32, inverse = its
        _ext.group_inverse; -> (B, C', m)."""
        src = _PackPoints.apply(xyz, new_xyz, features, float(scale))
        return self._run(src, pool=True, pre=Pregathered(idx, inverse, xyz.shape[1]))

    def interp_first_ok(self, features, idx):
        """forward_pooled_interp covers: features without gradient, the MFMA chain, two layers or
        more, shapes of the affine interpolation kernel."""
        from pointnet2 import _ext
        layers = list(self)
        recording = torch.is_grad_enabled()
        if recording and features.requires_grad:
            return False  # (a gradient w.r.t. the features would need the scatter form)
        return (os.environ.get("PN2_INTERP_FIRST", "1") != "0"
                and len(layers) >= 2 and features.is_cuda and features.dim() == 3
                and features.dtype == torch.float32 and hasattr(_ext, "three_interpolate_affine")
                and layers[0].conv.weight.shape[1] == features.shape[1] + 3
                and _ext.three_interpolate_affine_supported(layers[0].conv.weight.shape[0],
                                                            features.shape[2], idx.shape[1]))

    def forward_pooled_interp(self, features, idx, weight, rel, npoint, nsample):
        """forward_pooled(cat([rel, three_interpolate(features, idx, weight)]).view(B, 3 + C, npoint,
        nsample)) without that tensor: features (B,C,m) of the source points, idx / weight
        (B, npoint*nsample, 3), rel (B, 3, npoint*nsample); none of them with a gradient
        (interp_first_ok).  In a training pass the layer's real input is formed once, in the backward
        pass, for the weight gradient."""
        shape = (features.shape[0], list(self)[0].conv.weight.shape[0], npoint, nsample)
        return self._run(features.contiguous(), pool=True,
                         pre=Interpolated(idx.contiguous(), weight.contiguous(), rel.contiguous(), shape))

    def forward_pooled(self, x):
        """max over the last axis of forward(x): (B, C, npoint, nsample) -> (B, C', npoint)."""
        if self._use_fused(x):
            return self._run(x, pool=True)
        return torch.max(super().forward(x), dim=3)[0]


# ---- eval mode: the pooled MLP of a set-abstraction level in one pass (csrc/mlp_eval_pool.hip) ----
_eval_plans = None  # {id(SharedMLP): EvalPlan} while fused_eval() is in force


@contextlib.contextmanager
def fused_eval(plans):
    """Inside this context the pooled forwards of the SharedMLPs that `plans` ({id(module): EvalPlan})
    names run through their plan's one-pass kernels where its shape gate allows.  Only the inference
    engine (votenet/inference.py) enters it; outside it nothing changes."""
    global _eval_plans
    prev = _eval_plans
    _eval_plans = plans
    try:
        yield
    finally:
        _eval_plans = prev


def fold_bn_affine(gamma, beta, running_mean, running_var, eps):
    """The eval-mode BatchNorm y -> gamma (y - mean) / sqrt(var + eps) + beta as y * scale + shift, in
    the dtype of its arguments (the definition mlp_bn_eval_coeff computes on the device in fp32)."""
    scale = gamma / torch.sqrt(running_var + eps)
    return scale, beta - running_mean * scale


class EvalPlan(object):
    """Eval-mode BatchNorm of a three-layer pooled SharedMLP folded into per-channel (scale, shift)
    ONCE, plus the weight images of its one-pass kernel.  Two forms: LIN4 (4 -> 64 -> 64 -> 128, the
    grouped input of SA1) and STORED (c -> 128 -> 128 -> 128 / 256: layer 0 as the plain path runs it,
    the rest in one pass).  refresh() re-folds in place (captured graphs keep their addresses); the
    module's parameters and buffers are only read.  `hits` counts the forwards it served."""

    def __init__(self, mlp):
        layers = list(mlp)
        if len(layers) != 3 or not all(SharedMLP._fusable(layer) for layer in layers):
            raise ValueError("EvalPlan: a SharedMLP of three conv(1x1) -> BatchNorm2d -> ReLU layers")
        self.mlp = mlp
        self.shapes = [tuple(layer.conv.weight.shape[:2]) for layer in layers]  # (out, in)
        (c1, c0), (c2, _), (c3, _) = self.shapes
        if c0 == 4 and c1 == 64 and c2 == 64 and c3 == 128:
            self.form = "lin4"
        elif c1 == 128 and c2 == 128 and c3 in (128, 256):
            self.form = "stored"
        else:
            raise ValueError("EvalPlan: no one-pass kernel for layers %s" % (self.shapes,))
        self.coeffs, self.img, self.hits = None, None, 0
        self.refresh()

    def _weights(self):
        return [layer.conv.weight.detach().reshape(layer.conv.weight.shape[0], -1) for layer in self.mlp]

    def refresh(self):
        from pointnet2 import _mlp_ext as K
        bns = [next(layer.bn.children()) for layer in self.mlp]
        with torch.no_grad():
            coeffs = [K.fold_bn(bn) for bn in bns]
            w = [t.contiguous() for t in self._weights()]
            if self.coeffs is None:
                self.coeffs = coeffs
            else:
                for old, new in zip(self.coeffs, coeffs):
                    old[0].copy_(new[0])
                    old[1].copy_(new[1])
            if self.form == "lin4":
                self.img = K.eval_lin4_prepare(w[0], self.coeffs[0], w[1], w[2], self.img)
            else:
                self.img = K.eval_stored_prepare(w[1], w[2], self.img)

    def run(self, x, pre):
        """The pooled output, or None where the one-pass kernel does not apply (the caller then runs
        the plain path)."""
        from pointnet2 import _mlp_ext as K
        if torch.is_grad_enabled() or not x.is_cuda or x.dtype != torch.float32:
            return None
        if any(next(layer.bn.children()).training for layer in self.mlp):
            return None
        x = x.contiguous()
        (c1, c0), (c2, _), (c3, _) = self.shapes
        if self.form == "lin4":
            if pre is not None or x.dim() != 4 or x.shape[1] != 4 or \
                    not K.eval_lin4_supported(x.shape[0], c0, c1, c3, x.shape[2], x.shape[3]):
                return None
            self.hits += 1
            return K.eval_lin4_pool(x, self.img, self.coeffs[1], self.coeffs[2])
        if pre is None and x.dim() != 4:
            return None
        b, m, ns = pre.extent if pre is not None else (x.shape[0], x.shape[2], x.shape[3])
        if not K.eval_stored_supported(b, c1, c2, c3, m, ns):
            return None
        w0 = self._weights()[0]  # layer 0's raw output as the plain path forms it
        y0 = pre.forward(w0, x) if pre is not None else K.gemm_forward(w0, x)
        self.hits += 1
        return K.eval_stored_pool(y0.contiguous(), self.coeffs[0], self.img, self.coeffs[1], self.coeffs[2])


class _PackPoints(Function):
    """(xyz (B,N,3), new_xyz (B,m,3), features (B,C,N), s) -> src_ext (B, 3+C, N+m), the operand of
    the pre-gather first layer (_mlp_ext.pregather_pack).  Its gradient splits back into the three
    inputs: rows 0..2 are the coordinates' (columns < N: xyz, the others: new_xyz -- what
    QueryAndGroup's backward scatters / sums, pointnet2_utils.py:348-358), the other rows the
    features'."""

    @staticmethod
    def forward(ctx, xyz, new_xyz, features, s):
        from pointnet2 import _mlp_ext as K
        ctx.dims = (xyz.shape[1], new_xyz.shape[1], float(s))
        return K.pregather_pack(xyz.contiguous(), new_xyz.contiguous(), features.contiguous(), s)

    @staticmethod
    def backward(ctx, dsrc):
        from pointnet2 import _mlp_ext as K
        n, m, s = ctx.dims
        dsrc = dsrc.contiguous()
        dfeat = K.pregather_unpack_grad(dsrc, n, m) if ctx.needs_input_grad[2] else None
        dxyz = dnew = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            dc = dsrc[:, :3].transpose(1, 2)  # (B, N+m, 3)
            if s != 1.0:
                dc = dc * s
            dxyz = dc[:, :n].contiguous() if ctx.needs_input_grad[0] else None
            dnew = dc[:, n:].contiguous() if ctx.needs_input_grad[1] else None
        return dxyz, dnew, dfeat, None


class FC(nn.Sequential):
    def __init__(self, in_size, out_size, *, activation=nn.ReLU(inplace=True), bn=False,
                 init=None, preact=False, name=""):
        super().__init__()
        fc = nn.Linear(in_size, out_size, bias=not bn)
        if init is not None:
            init(fc.weight)
        if not bn:
            nn.init.constant_(fc.bias, 0)
        bn_unit = BatchNorm1d(in_size if preact else out_size) if bn else None
        _assemble(self, name, "fc", fc, bn_unit, activation, preact)


def set_bn_momentum_default(bn_momentum):
    def fn(m):
        if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d)):
            m.momentum = bn_momentum
    return fn


class BNMomentumScheduler(object):
    """Sets momentum = bn_lambda(epoch) on every batch-norm layer of `model` at each step()."""

    def __init__(self, model, bn_lambda, last_epoch=-1, setter=set_bn_momentum_default):
        if not isinstance(model, nn.Module):
            raise RuntimeError("Class '{}' is not a PyTorch nn Module".format(type(model).__name__))
        self.model = model
        self.setter = setter
        self.lmbd = bn_lambda
        self.step(last_epoch + 1)
        self.last_epoch = last_epoch

    def step(self, epoch=None):
        if epoch is None:
            epoch = self.last_epoch + 1
        self.last_epoch = epoch
        self.model.apply(self.setter(self.lmbd(epoch)))
