"""Frame-rate building blocks (reference: models/modules/dynamic.py:6-40).

State-dict keys match the reference (``net.{0,3,6,9}.weight|bias``, ``net.{1,4,7}.layer_norm.weight|bias``) so its
checkpoints load unchanged.  Inside ``NeuralWaveshaping.forward`` this arithmetic (1x1 conv -> LayerNorm over channels ->
LeakyReLU(0.01), FiLM) runs fused in ``frame_mlps16_kernel`` / ``exciter_newt_kernel``; called on their own the modules
run the stand-alone stage kernels of csrc/stages.hip (any layer sizes), one launch per call.
"""
import torch
import torch.nn as nn

from ... import ginlite as gin
from . import _standalone as sa


class FiLM(nn.Module):
    """gamma * x + beta (reference dynamic.py:6-8) on CUDA tensors; operands are broadcast like the reference's."""

    def forward(self, x, gamma, beta):
        x, gamma, beta = torch.broadcast_tensors(x, gamma, beta)
        x, gamma, beta = sa.contiguous(x, "x"), sa.contiguous(gamma, "gamma"), sa.contiguous(beta, "beta")
        return sa.call("film", x, gamma, beta)


class _Conv1x1Function(torch.autograd.Function):
    """Conv1x1.forward with its backward attached (td_mlp_grad on a one-layer stack): saves x"""

    @staticmethod
    def forward(ctx, x, module, *params):
        with torch.no_grad():
            y = module._forward_detached(x.detach())
        ctx.module = module
        ctx.save_for_backward(x)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        (x,) = ctx.saved_tensors
        need = ctx.needs_input_grad
        want = any(need[2:])
        gx, grads = ctx.module.vjp(grad_y, x, want_params=want)
        out = [grads[k].view_as(p) if n else None for (k, p), n in zip(ctx.module.named_parameters(), need[2:])] if want else [None, None]
        return (gx if need[0] else None, None, *out)


class Conv1x1(nn.Conv1d):
    """nn.Conv1d(in, out, 1) with the reference's parameters / state-dict keys whose forward is a HIP kernel (g_conv1x1_kernel,
    csrc/generic.hip): harmonic_mixer (models/neural_waveshaping.py:54) and newt.mixer (shaping.py:63-65) called on their own -
    what the forward runs instead of the fused kernels when somebody has registered forward hooks on sub-modules.

    ``differentiable`` (a plain attribute, default False): forward only.  Set to True, a forward under grad mode whose ``x``,
    weight or bias requires grad returns the same bits with a ``torch.autograd.Function`` attached that saves ``x``; its backward
    is ``vjp``: the existing ``td_mlp_grad`` op on a one-layer stack (no kernel of its own; the op always computes dL/dx too)."""

    differentiable = False      # also the value of a module unpickled from before the flag existed

    def __init__(self, in_channels, out_channels, kernel_size=1, **kw):
        if kernel_size not in (1, (1,)) or kw.get("groups", 1) != 1:
            raise RuntimeError("Conv1x1: kernel_size 1, groups 1")
        super().__init__(in_channels, out_channels, 1, **kw)

    def _forward_detached(self, x):
        wt = sa._req(self.weight.detach(), "weight")
        bt = sa._req(self.bias.detach(), "bias") if self.bias is not None else None
        return sa.call("g_conv1x1", x, wt, bt)

    def vjp(self, grad_y, x, want_params=True):
        """(dL/dx (B, in, N), {"weight": dW, "bias": db}) of ``forward`` at ``x`` for grad_y = dL/dy (B, out, N), an empty dict
        without ``want_params``: ``td_mlp_vjp`` on this one layer.  Whatever ``differentiable`` and the grad mode say; autograd
        is not involved and the results carry no graph."""
        if self.bias is None:
            raise RuntimeError("Conv1x1.vjp: the backward (td_mlp_grad) takes a layer with a bias")
        if x.dim() != 3 or x.shape[1] != self.in_channels:
            raise RuntimeError(f"Conv1d({self.in_channels}, {self.out_channels}, 1): expected (B, {self.in_channels}, N), got {tuple(x.shape)}")
        return td_mlp_vjp(x, self, grad_y, want_params)

    def forward(self, x):
        if self.differentiable and torch.is_grad_enabled() and isinstance(x, torch.Tensor):
            params = [self.weight] + ([self.bias] if self.bias is not None else [])
            if x.requires_grad or any(p.requires_grad for p in params):
                if self.bias is None:
                    raise RuntimeError("Conv1x1.differentiable: the backward (td_mlp_grad) takes a layer with a bias")
                xc = sa.contiguous(x.detach(), "x")
                if xc.dim() != 3 or xc.shape[1] != self.in_channels:
                    raise RuntimeError(f"Conv1d({self.in_channels}, {self.out_channels}, 1): expected (B, {self.in_channels}, N), got {tuple(x.shape)}")
                return _Conv1x1Function.apply(x if x.is_contiguous() else x.contiguous(), self, *params)
        x = sa.contiguous(x, "x")
        if x.dim() != 3 or x.shape[1] != self.in_channels:
            raise RuntimeError(f"Conv1d({self.in_channels}, {self.out_channels}, 1): expected (B, {self.in_channels}, N), got {tuple(x.shape)}")
        wt = sa._req(self.weight.detach(), "weight")
        bt = sa._req(self.bias.detach(), "bias") if self.bias is not None else None
        sa.no_autograd(params=[self.weight])
        return sa.call("g_conv1x1", x, wt, bt)


def upsample_linear(x, hop: int):
    """F.upsample(x, T * hop, mode="linear") on the last axis of a CUDA tensor (neural_waveshaping.py:75, shaping.py:69)."""
    x = sa.contiguous(x, "x")
    return sa.call("g_upsample", x, int(hop))


class TimeDistributedLayerNorm(nn.Module):
    """LayerNorm over the channel axis of a (B, C, T) tensor (reference dynamic.py:11-17)."""

    def __init__(self, size: int):
        super().__init__()
        self.layer_norm = nn.LayerNorm(size)

    def forward(self, x):
        x = sa.contiguous(x, "x")
        ln = self.layer_norm
        if x.dim() != 3 or x.shape[1] != ln.weight.numel():
            raise RuntimeError(f"TimeDistributedLayerNorm({ln.weight.numel()}): expected (B, {ln.weight.numel()}, T), got {tuple(x.shape)}")
        g, b = sa._req(ln.weight.detach(), "layer_norm.weight"), sa._req(ln.bias.detach(), "layer_norm.bias")
        return sa.call("td_layer_norm", x, g, b, float(ln.eps))


class _TDMLPFunction(torch.autograd.Function):
    """TimeDistributedMLP.forward with its backward attached (csrc/td_mlp_grad.hip): saves x alone; backward
    recomputes the forward per frame tile and hands gradients to x and to every parameter that requires grad"""

    @staticmethod
    def forward(ctx, x, module, *params):
        with torch.no_grad():
            y = td_mlp_forward(x.detach(), module.net)
        ctx.module = module
        ctx.save_for_backward(x)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        (x,) = ctx.saved_tensors
        named = list(ctx.module.net.named_parameters())
        want = any(ctx.needs_input_grad[2:])
        gx, grads = td_mlp_vjp(x, ctx.module.net, grad_y, want_params=want)
        out = [grads[k].view_as(p) if need else None for (k, p), need in zip(named, ctx.needs_input_grad[2:])] if want else [None] * len(named)
        return (gx if ctx.needs_input_grad[0] else None, None, *out)


@gin.configurable
class TimeDistributedMLP(nn.Module):
    """``differentiable`` (a plain attribute, default False): forward only, as the stage kernels are.  Set to True, a forward
    under grad mode returns the same bits with a ``torch.autograd.Function`` attached that saves ``x``; its backward runs
    ``td_mlp_grad`` and hands gradients to ``x`` and to every parameter that requires grad.  ``vjp`` is the same gradient
    without autograd."""

    differentiable = False      # also the value of a module unpickled from before the flag existed

    def __init__(self, in_size: int, hidden_size: int, out_size: int, depth: int = 3):
        super().__init__()
        assert depth >= 3, "Depth must be at least 3"
        widths = [in_size] + [hidden_size] * (depth - 1) + [out_size]
        stack = []
        for i, (fan_in, fan_out) in enumerate(zip(widths[:-1], widths[1:])):
            stack.append(nn.Conv1d(fan_in, fan_out, 1))
            if i != depth - 1:
                stack += [TimeDistributedLayerNorm(hidden_size), nn.LeakyReLU()]
        self.net = nn.Sequential(*stack)
        self.in_size, self.hidden_size, self.out_size, self.depth = in_size, hidden_size, out_size, depth
        self.differentiable = False

    def forward(self, x):
        """(B, in_size, T) -> (B, out_size, T) on a CUDA tensor: one launch of td_mlp_kernel (csrc/stages.hip)."""
        if self.differentiable and torch.is_grad_enabled():
            xc = sa.contiguous(x.detach(), "x")
            if xc.dim() != 3 or xc.shape[1] != self.in_size:
                raise RuntimeError(f"TimeDistributedMLP: expected (B, {self.in_size}, T), got {tuple(x.shape)}")
            params = list(self.net.parameters())
            if x.requires_grad or any(p.requires_grad for p in params):
                return _TDMLPFunction.apply(x if x.is_contiguous() else x.contiguous(), self, *params)
            return td_mlp_forward(xc, self.net)
        x = sa.contiguous(x, "x")
        if x.dim() != 3 or x.shape[1] != self.in_size:
            raise RuntimeError(f"TimeDistributedMLP: expected (B, {self.in_size}, T), got {tuple(x.shape)}")
        return td_mlp_forward(x, self.net)

    def vjp(self, grad_y, x, want_params=True):
        """(dL/dx, {state-dict key: gradient}) of ``forward`` at ``x`` for grad_y = dL/dy (B, out_size, T); keys like
        ``net.3.weight`` and ``net.1.layer_norm.bias``, an empty dict without ``want_params``.  Whatever ``differentiable`` and
        the grad mode say; autograd is not involved and the results carry no graph."""
        if x.dim() != 3 or x.shape[1] != self.in_size:
            raise RuntimeError(f"TimeDistributedMLP: expected (B, {self.in_size}, T), got {tuple(x.shape)}")
        gx, grads = td_mlp_vjp(x, self.net, grad_y, want_params)
        return gx, {"net." + k: v for k, v in grads.items()}


def _td_mlp_stack(net):
    """the checked pieces of a Conv1d(k=1) [-> TimeDistributedLayerNorm -> LeakyReLU] ... stack (or a bare Conv1d):
    (convs, weights, biases, ln weights, ln biases, eps, slope, state-dict key prefixes of the convs, of the norms)"""
    seq = isinstance(net, (nn.Sequential, list, tuple))
    mods = list(net) if seq else [net]
    convs = [m for m in mods if isinstance(m, nn.Conv1d)]
    norms = [m for m in mods if isinstance(m, TimeDistributedLayerNorm)]
    acts = [m for m in mods if isinstance(m, nn.LeakyReLU)]
    if len(norms) != len(convs) - 1 or any(c.kernel_size != (1,) or c.groups != 1 for c in convs):
        raise RuntimeError("TimeDistributedMLP: unexpected layer stack")
    ws = [sa._req(c.weight.detach(), "net weight") for c in convs]
    bs = [sa._req(c.bias.detach(), "net bias") for c in convs]
    gs = [sa._req(n.layer_norm.weight.detach(), "layer_norm.weight") for n in norms]
    ls = [sa._req(n.layer_norm.bias.detach(), "layer_norm.bias") for n in norms]
    eps = float(norms[0].layer_norm.eps) if norms else 1e-5
    slope = float(acts[0].negative_slope) if acts else 0.01
    # one eps / slope per launch (nws_td_mlp): a stack that mixes them is not what the kernel computes
    if any(float(n.layer_norm.eps) != eps for n in norms) or any(float(a.negative_slope) != slope for a in acts):
        raise RuntimeError("TimeDistributedMLP: the stage kernel takes ONE LayerNorm eps and ONE LeakyReLU slope for the whole "
                           "stack; these layers differ")
    if len(acts) != len(norms) or any(not n.layer_norm.elementwise_affine for n in norms):
        raise RuntimeError("TimeDistributedMLP: expected Conv1d -> LayerNorm(affine) -> LeakyReLU blocks")
    cpre = [f"{mods.index(c)}." if seq else "" for c in convs]
    npre = [f"{mods.index(n)}.layer_norm." for n in norms]
    return convs, ws, bs, gs, ls, eps, slope, cpre, npre


def td_mlp_forward(x, net):
    """Run a Conv1d(k=1) [-> TimeDistributedLayerNorm -> LeakyReLU] ... stack (or a bare Conv1d) on (B, C, T)."""
    convs, ws, bs, gs, ls, eps, slope, _, _ = _td_mlp_stack(net)
    sa.no_autograd(params=[p for c in convs for p in (c.weight, c.bias)])
    return sa.call("td_mlp", x, ws, bs, gs, ls, eps, slope)


def td_mlp_vjp(x, net, grad_y, want_params=True):
    """The backward of ``td_mlp_forward(x, net)`` for grad_y = dL/dy (B, out, T): ``(grad_x, {state-dict key relative to net:
    gradient})`` (an empty dict without ``want_params``), from one call of the ``td_mlp_grad`` op (csrc/td_mlp_grad.hip).  The
    forward saved nothing: the op recomputes it from ``x``.  Autograd is not involved and the results carry no graph."""
    with torch.no_grad():
        convs, ws, bs, gs, ls, eps, slope, cpre, npre = _td_mlp_stack(net)
        x = sa.contiguous(x.detach(), "x")
        g = sa.contiguous(grad_y.detach(), "grad_y")
        if x.dim() != 3 or x.shape[1] != ws[0].shape[1]:
            raise RuntimeError(f"td_mlp_vjp: expected x (B, {ws[0].shape[1]}, T), got {tuple(x.shape)}")
        if tuple(g.shape) != (x.shape[0], ws[-1].shape[0], x.shape[2]):
            raise RuntimeError(f"td_mlp_vjp: expected grad_y {(x.shape[0], ws[-1].shape[0], x.shape[2])}, got {tuple(g.shape)}")
        if g.device != x.device:
            raise RuntimeError(f"x is on {x.device} but grad_y is on {g.device}")
        out = sa.binding().td_mlp_grad(x, g, ws, bs, gs, ls, eps, slope, bool(want_params))
        if not want_params:
            return out[0], {}
        d, nl = len(ws), len(gs)
        keys = ([p + "weight" for p in cpre] + [p + "bias" for p in cpre] + [p + "weight" for p in npre] + [p + "bias" for p in npre])
        assert len(out) == 1 + 2 * d + 2 * nl
        return out[0], dict(zip(keys, out[1:]))
