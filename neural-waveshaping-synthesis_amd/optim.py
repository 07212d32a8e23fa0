"""``Adam``: gradient-norm clipping and the Adam update of every parameter in one operator call - two kernel launches where
``clip_grad_norm_`` + ``torch.optim.Adam`` take dozens over the model's 48 small tensors (csrc/adam_step.hip).

The arithmetic is ``torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm, 2.0)`` followed by ``torch.optim.Adam`` with
``weight_decay = 0``, no amsgrad and no maximize; sums run in a fixed order, so equal inputs give equal bits.  One difference from
Lightning's ``gradient_clip_val``: ``clip_grad_norm_`` scales ``.grad`` in place, this step reads ``.grad`` and leaves it as it is.
"""
import math

import torch

from . import _lib


class Adam(torch.optim.Optimizer):
    """``Adam(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None)``

    ``step()`` is one call of the ``adam_step`` operator over every parameter whose ``.grad`` is not ``None``; the norm that
    ``max_grad_norm`` bounds (``None``: no clipping) is taken over all parameter groups together, as Lightning's clip does.  The
    norm comes back as ``last_grad_norm``, a 0-dim device tensor that is never synchronised here.  ``.grad`` is NOT rewritten
    (``clip_grad_norm_`` scales it in place).  ``lr`` is read from ``param_groups`` at every step, so ``torch.optim.lr_scheduler``
    classes drive it; parameter groups with different ``lr``, ``betas`` or ``eps`` are refused, and so are weight decay, amsgrad
    and maximize.  The operator takes one step count: the parameters of one call must have seen the same number of steps.

    The state has ``torch.optim.Adam``'s layout - ``state[p] = {step, exp_avg, exp_avg_sq}`` - so ``state_dict()`` moves to that
    class and back; ``step`` is kept as torch keeps it (a float32 CPU tensor) and read as an int or a tensor.  Fresh state is two
    views per parameter into one zeroed buffer.  CUDA float32 contiguous parameters only: there is no CPU fallback."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None):
        if not 0.0 <= float(lr):
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= float(eps):
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid betas: {betas}")
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError(f"Invalid max_grad_norm: {max_grad_norm}")
        # weight_decay / amsgrad / maximize: constants, present so that a state dict moves to torch.optim.Adam and back
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0, amsgrad=False, maximize=False))
        self.max_grad_norm = max_grad_norm
        self.last_grad_norm = None

    def _hyper_parameters(self):
        groups = self.param_groups
        first = (float(groups[0]["lr"]), float(groups[0]["betas"][0]), float(groups[0]["betas"][1]), float(groups[0]["eps"]))
        for g in groups:
            if (float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"])) != first:
                raise RuntimeError("nws.optim.Adam: parameter groups with different lr, betas or eps are not supported (one "
                                   "operator call steps every parameter)")
            if g.get("weight_decay", 0) != 0 or g.get("amsgrad", False) or g.get("maximize", False):
                raise RuntimeError("nws.optim.Adam: weight_decay, amsgrad and maximize are not supported")
        return first

    def load_state_dict(self, state_dict):
        """``torch.optim.Adam``'s layout; ``step`` as an int (checkpoints of older torch versions, the reference's among them) or a
        tensor, kept from here on as torch keeps it: a float32 CPU tensor"""
        super().load_state_dict(state_dict)
        for s in self.state.values():
            if "step" in s:
                s["step"] = torch.tensor(float(s["step"]), dtype=torch.float32)

    def _fresh_state(self, params):
        total = sum(p.numel() for p in params)
        flat = torch.zeros(2 * total, dtype=torch.float32, device=params[0].device)
        off = 0
        for p in params:
            n = p.numel()
            self.state[p] = {"step": torch.tensor(0.0, dtype=torch.float32), "exp_avg": flat[off:off + n].view(p.shape),
                             "exp_avg_sq": flat[total + off:total + off + n].view(p.shape)}
            off += n

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lr, beta1, beta2, eps = self._hyper_parameters()
        params = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
        if not params:
            return loss
        for p in params:
            if p.device.type != "cuda" or p.grad.device.type != "cuda":
                raise _lib.NwsError(f"nws.optim.Adam: a parameter lives on {p.device}: the optimiser step only runs as HIP kernels "
                                    "on an AMD GPU (move the model with .to('cuda')); there is no CPU fallback.")
        by_device = {}
        for p in params:
            if len(self.state[p]) == 0:
                by_device.setdefault(p.device, []).append(p)
        for fresh in by_device.values():
            self._fresh_state(fresh)
        states = [self.state[p] for p in params]
        steps = {int(s["step"]) for s in states}
        if len(steps) != 1:
            raise RuntimeError(f"nws.optim.Adam: the parameters of one step have seen different numbers of steps {sorted(steps)}: "
                               "one operator call takes one step count")
        t = steps.pop() + 1
        from .engine import binding

        max_norm = math.inf if self.max_grad_norm is None else float(self.max_grad_norm)
        self.last_grad_norm = binding().adam_step(params, [p.grad for p in params], [s["exp_avg"] for s in states],
                                                  [s["exp_avg_sq"] for s in states], t, lr, beta1, beta2, eps, max_norm)
        for s in states:
            s["step"] = torch.tensor(float(t), dtype=torch.float32)
        return loss
