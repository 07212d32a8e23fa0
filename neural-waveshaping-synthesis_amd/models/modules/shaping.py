"""Waveshaper bank and reverb (reference: models/modules/shaping.py:10-173).

Constructor signatures, attribute names and state-dict keys follow the reference so that
``model.newt = FastNEWT(model.newt)`` (scripts/time_forward_pass.py:42-43, colab cell 17) and
checkpoint loading work unchanged.  Inside ``NeuralWaveshaping.forward`` the arithmetic lives in csrc/exciter_newt.hip
(FiLM -> shaper LUT / sin-MLP -> FiLM -> 64->1 mix, fused with the exciter) and csrc/reverb_fft.hip; called on their own,
``NEWT.forward(exciter, control_embedding)``, ``TrainableNonlinearity.forward``, ``FastNEWT.shaping_fn``, ``Sine`` and
``Reverb.forward`` each run one stand-alone stage kernel.
"""
import ctypes as C

import torch
import torch.nn as nn

from ... import ginlite as gin
from . import _standalone as sa
from .dynamic import Conv1x1, FiLM, TimeDistributedMLP, td_mlp_vjp, upsample_linear


class Sine(nn.Module):
    def forward(self, x):
        """sin(x) on a CUDA tensor with the engine's full-range sine (nws_sin: <= 1.5e-7 absolute)."""
        x = sa.contiguous(x, "x")
        return sa.call("sine", x)


class _GShaperCache:
    """NwsShaperDesc of a TrainableNonlinearity or a FastNEWT table as the byte tensor the binding takes (`sdesc`), cached until a
    tensor changes"""

    def __init__(self):
        self._key = None
        self._val = None

    def get(self, sh=None, *, lut=None, lut_min=0.0, lut_max=0.0):
        from ...generic import desc_bytes, shaper_desc

        ts = [lut] if lut is not None else list(sh.parameters())
        key = tuple((t.data_ptr(), t._version) for t in ts) + (float(lut_min), float(lut_max))
        if key != self._key:
            sa.no_autograd(params=ts)
            keep = []
            d = shaper_desc(sh, lut=lut, lut_min=lut_min, lut_max=lut_max, keep=keep)
            self._val = (desc_bytes(d), keep)
            self._key = key
        return self._val[0]


@gin.configurable
class TrainableNonlinearity(nn.Module):
    """64 independent scalar sin-MLPs stored as grouped 1x1 convs (reference shaping.py:15-37)."""

    def __init__(self, channels, width, nonlinearity=nn.ReLU, final_nonlinearity=Sine, depth=3):
        super().__init__()
        self.input_scale = nn.Parameter(torch.randn(1, channels, 1) * 10)
        stack = []
        for i in range(depth):
            last = i == depth - 1
            stack.append(nn.Conv1d(channels if i == 0 else channels * width,
                                   channels if last else channels * width, 1, groups=channels))
            stack.append(final_nonlinearity() if last else nonlinearity())
        self.net = nn.Sequential(*stack)
        self.channels, self.width, self.depth = channels, width, depth
        self._desc = sa.Desc()
        self._gdesc = _GShaperCache()

    def __getstate__(self):
        d = self.__dict__.copy()
        d["_desc"] = sa.Desc()
        d["_gdesc"] = _GShaperCache()
        return d

    def forward(self, x):
        """Exact shapers on a (B, 64, N) CUDA tensor - one HIP kernel (nws_shaper_apply)."""
        x = sa.contiguous(x, "x")
        if x.dim() != 3 or x.shape[1] != self.channels:
            raise RuntimeError(f"expected (B, {self.channels}, N), got {tuple(x.shape)}")
        if not all(isinstance(m, Sine) for m in list(self.net)[1::2]):
            raise RuntimeError("kernels implement the sine activations NEWT configures (nonlinearity=Sine)")
        if (self.channels, self.width, self.depth) != (sa._lib.N_SHAPERS, sa._lib.SHAPER_WIDTH, 4):
            return sa.call("g_shaper_apply", self._gdesc.get(self), x)          # any channels / width / depth (csrc/generic.hip)
        return sa.call("shaper_apply", self._desc.get(sa.shaper_fields(self)), x)


def _newt_grad_keys(depth):
    """the 2 depth + 3 keys of the sample-rate part's parameter gradients, in the order of the newt_grad / g_newt_grad ops"""
    return ("shaping_fn.input_scale", *(f"shaping_fn.net.{2 * l}.{k}" for l in range(depth) for k in ("weight", "bias")),
            "mixer.0.weight", "mixer.0.bias")


class _NEWTFunction(torch.autograd.Function):
    """NEWT.forward with its backward attached (csrc/newt_grad.hip; any other bank size csrc/g_newt_grad.hip,
    DESIGN.md 3.20): saves the two inputs; backward is
    ``NEWT.vjp`` and hands gradients to the exciter, the control embedding and every parameter that requires grad"""

    @staticmethod
    def forward(ctx, exciter, control_embedding, module, *params):
        with torch.no_grad():
            y = module._forward_detached(exciter.detach(), control_embedding.detach())
        ctx.module = module
        ctx.save_for_backward(exciter, control_embedding)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        exciter, emb = ctx.saved_tensors
        need = ctx.needs_input_grad
        want = any(need[3:])
        ge, gemb, grads = ctx.module.vjp(grad_out, exciter, emb, want_params=want, want_exciter=need[0])
        named = list(ctx.module.named_parameters())
        out = [grads[k].view_as(p) if n else None for (k, p), n in zip(named, need[3:])] if want else [None] * len(named)
        return (ge, gemb if need[1] else None, None, *out)


@gin.configurable
class NEWT(nn.Module):
    """``differentiable`` (a plain attribute, default False): forward only, as the stage kernels are.  Set to True (hop 128,
    one output channel, sine activations; up to 64 shapers of width up to 16 and depth up to 4), a forward under grad mode whose
    exciter, control embedding or parameters require grad returns the same bits with a ``torch.autograd.Function`` attached that
    saves the two inputs; its backward hands gradients to both and to each of the parameters that requires grad (25 at depth 4).
    ``vjp`` is the same gradient without autograd.  The packaged size set (64 shapers of width 8 and depth 4) runs
    csrc/newt_grad.hip, every other one csrc/g_newt_grad.hip."""

    differentiable = False      # also the value of a module unpickled from before the flag existed

    def __init__(self, n_waveshapers: int, control_embedding_size: int, shaping_fn_size: int = 16,
                 out_channels: int = 1):
        super().__init__()
        self.n_waveshapers = n_waveshapers
        self.mlp = TimeDistributedMLP(control_embedding_size, control_embedding_size, n_waveshapers * 4, depth=4)
        self.waveshaping_index = FiLM()
        self.shaping_fn = TrainableNonlinearity(n_waveshapers, shaping_fn_size, nonlinearity=Sine)
        self.normalising_coeff = FiLM()
        self.mixer = nn.Sequential(Conv1x1(n_waveshapers, out_channels, 1))
        self._newt_desc = sa.Desc()
        self._g_newt = _GShaperCache()

    def __getstate__(self):
        d = self.__dict__.copy()
        d["_newt_desc"] = sa.Desc()
        d["_g_newt"] = _GShaperCache()
        return d

    def _apply_fields(self):
        return sa.shaper_fields(self._modules["shaping_fn"]), {}

    def _specialised(self, hop):
        sh = self._modules["shaping_fn"]
        return (self.n_waveshapers == sa._lib.N_SHAPERS and self.mixer[0].out_channels == 1 and hop == sa._lib.HOP
                and (sh.channels, sh.width, sh.depth) == (sa._lib.N_SHAPERS, sa._lib.SHAPER_WIDTH, 4))

    def _g_shaper(self):
        return self._g_newt.get(self._modules["shaping_fn"])

    def _forward_generic(self, exciter, film):
        """any n_waveshapers / shaping_fn_size / depth / out_channels / hop: FiLM -> shaper -> FiLM (g_film_shaper_kernel) then
        the Conv1d(S -> out_channels) mixer (g_conv1x1_kernel), csrc/generic.hip"""
        mw = sa._req(self.mixer[0].weight.detach(), "newt.mixer.0.weight")
        mb = sa._req(self.mixer[0].bias.detach(), "newt.mixer.0.bias")
        return sa.call("g_newt_apply", self._g_shaper(), exciter, film, mw, mb)

    def _need_backward(self, hop=None, device=None):
        """True for the packaged size set (csrc/newt_grad.hip), False for another one the runtime-size backward serves
        (csrc/g_newt_grad.hip); raises for everything else.  A forward that carries a backward never calls the inner modules.
        ``device``: of the exciter - on the runtime-size path the refusal of a CPU tensor names the size set."""
        sh = self._modules["shaping_fn"]
        hop = sa._lib.HOP if hop is None else hop
        sizes = f"this is {self.n_waveshapers} shapers of width {sh.width} and depth {sh.depth}"
        packaged = NEWT._specialised(self, sa._lib.HOP)
        if not all(isinstance(m, Sine) for m in list(sh.net)[1::2]):
            raise RuntimeError("NEWT: the backward implements the sine activations NEWT configures (nonlinearity=Sine)")
        if hop != sa._lib.HOP or self.mixer[0].out_channels != 1:
            raise RuntimeError(f"NEWT: the backward exists for hop {sa._lib.HOP} and one output channel only (the noise branch and the "
                               f"GRU fix the hop: their runtime-size forms have no backward); {sizes}, hop {hop}, "
                               f"{self.mixer[0].out_channels} output channel(s)")
        if not packaged and device is not None and device.type != "cuda":
            raise RuntimeError(f"NEWT: the backward needs tensors on an AMD GPU (no CPU fallback), the exciter is on {device}; {sizes}, "
                               "which runs on the runtime-size path (csrc/g_newt_grad.hip)")
        if not packaged and not (1 <= self.n_waveshapers <= 64 and 1 <= sh.width <= 16 and 1 <= sh.depth <= 4):
            raise RuntimeError("NEWT: the runtime-size backward (csrc/g_newt_grad.hip) exists for at most 64 shapers of width at most 16 "
                               f"and depth at most 4; {sizes}")
        return packaged

    def _need_backward_for(self, exciter, control_embedding):
        """``_need_backward`` on the unchecked pair: the hop where the shapes give one, and the exciter's device"""
        hop = None
        if getattr(exciter, "ndim", 0) == 3 and getattr(control_embedding, "ndim", 0) == 3 and control_embedding.shape[2] >= 1:
            hop = exciter.shape[2] // control_embedding.shape[2]
        return self._need_backward(hop, exciter.device if isinstance(exciter, torch.Tensor) else None)

    def _checked_pair(self, exciter, control_embedding):
        exciter = sa.contiguous(exciter, "exciter")
        emb = sa.contiguous(control_embedding, "control_embedding")
        if exciter.dim() != 3 or exciter.shape[1] != self.n_waveshapers:
            raise RuntimeError(f"NEWT: expected an exciter of shape (B, {self.n_waveshapers}, N), got {tuple(exciter.shape)}")
        if emb.dim() != 3 or emb.shape[0] != exciter.shape[0] or emb.shape[2] < 1 or exciter.shape[2] % emb.shape[2]:
            raise RuntimeError(f"NEWT: exciter {tuple(exciter.shape)} does not match a control embedding {tuple(emb.shape)}")
        if emb.device != exciter.device:
            raise RuntimeError(f"exciter is on {exciter.device} but the control embedding is on {emb.device}")
        return exciter, emb

    def _wdesc(self):
        tensors, scalars = NEWT._apply_fields(self)
        tensors = dict(tensors, newt_out_w=self.mixer[0].weight, newt_out_b=self.mixer[0].bias)
        return self._newt_desc.get(tensors, scalars)

    def _forward_detached(self, exciter, control_embedding):
        """the forward on checked, detached inputs (callers hold no_grad): the launches of ``forward`` for the module's size set"""
        film = self.mlp(control_embedding)
        if not NEWT._specialised(self, exciter.shape[2] // film.shape[2]):
            return self._forward_generic(exciter, film)
        return sa.call("newt_apply", self._wdesc(), exciter, film)

    def vjp(self, grad_out, exciter, control_embedding, want_params=True, want_exciter=True):
        """(dL/d(exciter) (B, S, N) | None, dL/d(control_embedding) (B, 128, T), {state-dict key relative to this module:
        gradient}) of ``forward`` at (exciter, control_embedding) for grad_out = dL/d(out) (B, 1, N); the keys ``mlp.net.*``,
        ``shaping_fn.*`` and ``mixer.0.*`` (25 at depth 4), an empty dict without ``want_params``.  Reruns ``self.mlp`` for the FiLM
        parameters, takes their gradient and the sample-rate part from the ``newt_grad`` op (csrc/newt_grad.hip, DESIGN.md 3.18;
        the packaged size set) or the ``g_newt_grad`` op (csrc/g_newt_grad.hip; any other) and the MLP's part from
        ``td_mlp_vjp``.  Whatever ``differentiable`` and the grad mode say; autograd is not involved and the results carry no
        graph."""
        with torch.no_grad():
            self._need_backward_for(exciter, control_embedding)
            exciter, emb = self._checked_pair(exciter.detach(), control_embedding.detach())
            g = sa.contiguous(grad_out.detach(), "grad_out")
            packaged = self._need_backward(exciter.shape[2] // emb.shape[2])
            if g.numel() != exciter.shape[0] * exciter.shape[2] or g.shape[0] != exciter.shape[0]:
                raise RuntimeError(f"NEWT: grad_out {tuple(g.shape)} is not ({exciter.shape[0]}, 1, {exciter.shape[2]})")
            if g.device != exciter.device:
                raise RuntimeError(f"exciter is on {exciter.device} but grad_out is on {g.device}")
            film = self.mlp(emb)
            if packaged:
                out = sa.binding().newt_grad(self._wdesc(), exciter, film, g, bool(want_exciter), bool(want_params))
            else:
                mw = sa._req(self.mixer[0].weight.detach(), "newt.mixer.0.weight")
                mb = sa._req(self.mixer[0].bias.detach(), "newt.mixer.0.bias")
                out = sa.binding().g_newt_grad(self._g_shaper(), exciter, film, g, mw, mb, bool(want_exciter), bool(want_params))
            g_emb, mg = td_mlp_vjp(emb, self.mlp.net, out[0], want_params)
            g_exc = out[1] if want_exciter else None
            if not want_params:
                return g_exc, g_emb, {}
            keys = _newt_grad_keys(self._modules["shaping_fn"].depth)
            grads = {"mlp.net." + k: v for k, v in mg.items()}
            grads.update(zip(keys, out[-len(keys):]))
            return g_exc, g_emb, grads

    def forward(self, exciter, control_embedding):
        """(B, 64, N) exciter, (B, 128, T) control embedding -> (B, 1, N) (reference shaping.py:67-79): the FiLM-parameter
        MLP (one launch) then FiLM -> shaper -> FiLM -> Conv1d(64 -> 1) on the materialised exciter (one launch)."""
        if self.differentiable and torch.is_grad_enabled():
            params = list(self.parameters())
            if any(isinstance(t, torch.Tensor) and t.requires_grad for t in (exciter, control_embedding, *params)):
                self._need_backward_for(exciter, control_embedding)
                e, c = self._checked_pair(exciter.detach(), control_embedding.detach())
                self._need_backward(e.shape[2] // c.shape[2])
                if sa.has_hooks(self.waveshaping_index, self.normalising_coeff, self.mixer, self.mixer[0], self._modules.get("shaping_fn")):
                    raise RuntimeError("NEWT.differentiable: forward hooks on the inner modules (waveshaping_index, shaping_fn, "
                                       "normalising_coeff, mixer) make the forward run them one by one, and that sequence has no "
                                       "backward; remove the hooks or clear the flag")
                return _NEWTFunction.apply(exciter if exciter.is_contiguous() else exciter.contiguous(),
                                           control_embedding if control_embedding.is_contiguous() else control_embedding.contiguous(),
                                           self, *params)
        exciter = sa.contiguous(exciter, "exciter")
        if exciter.dim() != 3 or exciter.shape[1] != self.n_waveshapers:
            raise RuntimeError(f"NEWT: expected an exciter of shape (B, {self.n_waveshapers}, N), got {tuple(exciter.shape)}")
        film = self.mlp(control_embedding)                       # (B, 256, T), channel-major like the reference's Conv1d stack
        T = film.shape[2]
        if exciter.shape[0] != film.shape[0] or exciter.shape[2] % T:
            raise RuntimeError(f"NEWT: exciter {tuple(exciter.shape)} does not match {T} control frames")
        if sa.has_hooks(self.waveshaping_index, self.normalising_coeff, self.mixer, self.mixer[0], self._modules.get("shaping_fn")):
            # somebody listens on the inner modules: run them one by one, exactly the reference's sequence (shaping.py:69-79)
            fp = upsample_linear(film, exciter.shape[2] // T)
            g_i, b_i, g_n, b_n = torch.split(fp, self.n_waveshapers, 1)
            x = self.waveshaping_index(exciter, g_i, b_i)
            x = self.shaping_fn(x)
            x = self.normalising_coeff(x, g_n, b_n)
            return self.mixer(x)
        if not self._specialised(exciter.shape[2] // T):
            return self._forward_generic(exciter, film)
        tensors, scalars = self._apply_fields()
        tensors = dict(tensors, newt_out_w=self.mixer[0].weight, newt_out_b=self.mixer[0].bias)
        return sa.call("newt_apply", self._newt_desc.get(tensors, scalars), exciter, film)


class FastNEWT(NEWT):
    """Lookup-table replacement of the shaper MLPs (reference shaping.py:82-151).

    ``lookup_table[s, i] = shaper_s(linspace(table_min, table_max, table_size)[i])`` is evaluated by the
    HIP kernel ``shaper_table_kernel``.  Like the reference it shares ``mlp``, the FiLM modules and
    ``mixer`` with the wrapped NEWT.  The wrapped NEWT's trained ``shaping_fn`` stays registered as a
    sub-module (the reference keeps a dangling re-initialised one there).
    """

    def __init__(self, newt: NEWT, table_size: int = 4096, table_min: float = -3.0, table_max: float = 3.0):
        super().__init__()
        self.table_size = table_size
        self.table_min = table_min
        self.table_max = table_max
        self.n_waveshapers = newt.n_waveshapers
        self.mlp = newt.mlp
        self.waveshaping_index = newt.waveshaping_index
        self.normalising_coeff = newt.normalising_coeff
        self.mixer = newt.mixer
        self._modules["shaping_fn"] = newt._modules["shaping_fn"]
        self.lookup_table = self._init_lookup_table(newt, table_size, self.n_waveshapers, table_min, table_max)
        self._lut_desc = sa.Desc()
        self._g_lut = _GShaperCache()

    def __getstate__(self):
        d = super().__getstate__()
        d["_lut_desc"] = sa.Desc()
        d["_g_lut"] = _GShaperCache()
        return d

    def _specialised(self, hop):
        return self.n_waveshapers == sa._lib.N_SHAPERS and self.mixer[0].out_channels == 1 and hop == sa._lib.HOP

    _NO_BACKWARD = ("FastNEWT: the lookup table has no backward (a table lookup has no gradient with respect to the shapers' "
                    "parameters); training uses the exact NEWT, as the reference does, and the table is built from it afterwards")

    @property
    def differentiable(self):
        return False

    @differentiable.setter
    def differentiable(self, value):
        if value:
            raise RuntimeError(self._NO_BACKWARD)

    def vjp(self, grad_out, exciter, control_embedding, want_params=True, want_exciter=True):
        raise RuntimeError(self._NO_BACKWARD)

    def _g_shaper(self):
        return self._g_lut.get(lut=self.lookup_table, lut_min=self.table_min, lut_max=self.table_max)

    @staticmethod
    def _init_lookup_table(newt, table_size, n_waveshapers, table_min, table_max):
        sh = newt._modules["shaping_fn"]
        home = sh.input_scale.device
        if home.type == "cuda":
            dev = home
        elif torch.cuda.is_available():
            # the reference builds FastNEWT before .to(device) (scripts/time_forward_pass.py:42-45);
            # the table is still computed by the HIP kernel, then parked next to the module
            dev = torch.device("cuda", torch.cuda.current_device())
        else:
            raise sa._lib.NwsError("FastNEWT needs an AMD GPU to evaluate its lookup table (no CPU fallback)")
        if (sh.channels, sh.width, sh.depth) != (sa._lib.N_SHAPERS, sa._lib.SHAPER_WIDTH, 4):
            # any channels / width / depth: runtime-size table kernel (csrc/generic.hip: g_shaper_table_kernel)
            import copy

            from ...generic import desc_bytes, shaper_desc

            sh_dev = sh if home == dev else copy.deepcopy(sh).to(dev)
            keep = []
            d = shaper_desc(sh_dev, keep=keep)
            with torch.no_grad():
                table = sa.call("g_shaper_table", desc_bytes(d), keep[0], int(table_size), float(table_min), float(table_max))
            torch.cuda.current_stream(dev).synchronize()
            return nn.Parameter(table.to(home))
        fields = {k: v.detach().to(dev).contiguous() for k, v in sa.shaper_fields(sh).items()}
        table = sa.call("shaper_table", sa.Desc().get(fields), fields["shaper_in_scale"], int(table_size), float(table_min), float(table_max))
        torch.cuda.current_stream(dev).synchronize()
        return nn.Parameter(table.to(home))

    def _lut_fields(self):
        return {"lut": self.lookup_table}, {"lut_size": int(self.table_size), "lut_min": float(self.table_min),
                                            "lut_max": float(self.table_max)}

    def _apply_fields(self):
        return self._lut_fields()

    def shaping_fn(self, x):
        """LUT lookup with the reference's index quirks, on a (B, 64, N) CUDA tensor (nws_shaper_apply)."""
        x = sa.contiguous(x, "x")
        if x.dim() != 3 or x.shape[1] != self.n_waveshapers:
            raise RuntimeError(f"expected (B, {self.n_waveshapers}, N), got {tuple(x.shape)}")
        if self.lookup_table.numel() != self.n_waveshapers * self.table_size:
            raise RuntimeError("lookup_table does not match table_size")
        if self.n_waveshapers != sa._lib.N_SHAPERS:
            return sa.call("g_shaper_apply", self._g_shaper(), x)
        return sa.call("shaper_apply", self._lut_desc.get(*self._lut_fields()), x)


class _ReverbFunction(torch.autograd.Function):
    """Reverb.forward with its transpose attached (csrc/reverb_fft.hip): backward runs reverb_grad_x and
    reverb_grad_ir, each only when its gradient is needed"""

    @staticmethod
    def forward(ctx, x, ir, module):
        xd = x.detach()
        y = module._forward_detached(xd)
        ctx.module = module
        ctx.save_for_backward(xd, ir)          # ir itself: an in-place change before backward is autograd's to refuse
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        xd, ir = ctx.saved_tensors
        dx, dir_ = ctx.module.vjp(xd, grad_out, need_x=ctx.needs_input_grad[0], need_ir=ctx.needs_input_grad[1])
        return dx, dir_, None


@gin.configurable
class Reverb(nn.Module):
    """x + circular_conv(x, [0, ir]) of length max(N, len(ir)+1) (reference shaping.py:154-173).

    ``differentiable`` (a plain attribute, default False): forward only, the result carries no graph.  Set to True, a forward
    under grad mode whose x or ir requires grad returns the same bits with a ``torch.autograd.Function`` attached that gives
    dL/dx and dL/d(ir) (``initial_zero`` is a buffer).  ``vjp`` is the same pair of gradients without autograd."""

    differentiable = False      # also the value of a module unpickled from before the flag existed

    def __init__(self, length_in_seconds, sr):
        super().__init__()
        self.ir = nn.Parameter(torch.randn(1, sr * length_in_seconds - 1) * 1e-6)
        self.register_buffer("initial_zero", torch.zeros(1, 1))
        self.differentiable = False
        self._tables = {}

    def __getstate__(self):
        d = self.__dict__.copy()
        d["_tables"] = {}
        return d

    def _plan_and_spectrum(self, x, ir, need_plan=False):
        """(plan tensor, tables, IR spectrum) of a (B, N) call, or None when the circular length is odd and has no plan; the
        spectrum is cached until ir changes (in place: ir._version)"""
        from ..._lib import NwsReverbPlan
        from ...engine import reverb_plan_and_tables

        N = x.shape[1]
        probe = NwsReverbPlan()
        if sa._lib.lib().nws_reverb_plan(int(N), int(ir.numel()) + 1, C.byref(probe)) != 0:
            if need_plan:
                raise RuntimeError(f"Reverb: no gradient for an odd circular length (max(N, len(ir) + 1) = {max(N, ir.numel() + 1)}): "
                                   "the reference's rfft / irfft pair is not a circular convolution there, and the transform "
                                   "kernels that carry the backward have a plan for even lengths only")
            return None
        plan, tables, plan_t = reverb_plan_and_tables(x.device, N, ir.numel() + 1)
        L = sa._lib.lib()
        key = (plan.L, ir.data_ptr(), ir._version)
        spec = self._tables.get(key)
        if spec is None:
            self._tables.clear()
            with torch.cuda.device(x.device):
                spec = torch.empty(L.nws_reverb_spectrum_bytes(C.byref(plan)) // 4, dtype=torch.float32, device=x.device)
                nb = L.nws_reverb_workspace_bytes(C.byref(plan), 1)
                ws1 = torch.empty(nb, dtype=torch.uint8, device=x.device)
                sa.checked(L.nws_reverb_ir_spectrum(C.byref(plan), tables.data_ptr(), ir.data_ptr(), ir.numel(),
                                                    spec.data_ptr(), ws1.data_ptr(), nb, sa.stream_ptr(x.device)),
                           "nws_reverb_ir_spectrum")
            self._tables[key] = spec
        return plan_t, tables, spec

    def _checked_input(self, x, name="x"):
        x = sa.contiguous(x, name)
        if x.dim() != 2:
            raise RuntimeError(f"{name}: expected (B, N), got {tuple(x.shape)}")
        ir = sa._req(self.ir.detach(), "reverb.ir")
        if ir.device != x.device:
            raise RuntimeError(f"{name} is on {x.device} but reverb.ir is on {ir.device}")
        return x, ir

    def _forward_detached(self, x):
        x, ir = self._checked_input(x)
        aux = self._plan_and_spectrum(x, ir)
        if aux is None:
            # odd circular length (every even one has a plan): the reference's own rfft / irfft expression (csrc/generic.hip)
            return sa.call("g_reverb_direct", x, ir.reshape(-1))
        plan_t, tables, spec = aux
        return sa.call("reverb", plan_t, tables, spec, x)

    def forward(self, x):
        """Stand-alone reverb on a (B, N) CUDA tensor: four-step FFT kernels of csrc/reverb_fft.hip."""
        if self.differentiable and torch.is_grad_enabled() and isinstance(x, torch.Tensor) and (x.requires_grad or self.ir.requires_grad):
            xc, ir = self._checked_input(x.detach())
            self._plan_and_spectrum(xc, ir, need_plan=True)       # refusals before autograd is involved
            return _ReverbFunction.apply(x, self.ir, self)
        return self._forward_detached(x)

    def vjp(self, x, grad_out, need_x=True, need_ir=True):
        """(dL/dx | None, dL/d(ir) | None) of ``forward`` at x for grad_out = dL/dy: dx in the shape of x, dir in the shape of
        ir, (1, ir_len), summed over the batch.  Whatever ``differentiable`` and the grad mode say; autograd is not involved
        and the results carry no graph."""
        with torch.no_grad():
            x, ir = self._checked_input(x.detach())
            g, _ = self._checked_input(grad_out.detach(), "grad_out")
            if g.shape != x.shape:
                raise RuntimeError(f"grad_out {tuple(g.shape)} is not in the shape of x {tuple(x.shape)}")
            if not (need_x or need_ir):
                return None, None
            plan_t, tables, spec = self._plan_and_spectrum(x, ir, need_plan=True)
            dx = sa.call("reverb_grad_x", plan_t, tables, spec, g) if need_x else None
            dir_ = sa.call("reverb_grad_ir", plan_t, tables, x, g, int(ir.numel())).reshape(self.ir.shape) if need_ir else None
            return dx, dir_
