"""``NeuralWaveshaping`` - the drop-in module surface of the MI355X NEWT engine.

Mirrors the reference's ``NeuralWaveshaping`` (models/neural_waveshaping.py:29-90): same constructor
(gin-configurable), sub-module / attribute names, state-dict keys, ``forward(f0, control)``,
``render_exciter`` and ``get_embedding``.  ``forward`` is ONE call into the C-ABI (``nws_forward``),
which enqueues the hand-written HIP kernels on torch's current stream.

Of the reference's Lightning hooks (:92-165) the two that need no backward pass are here: ``validation_step``
and ``test_step`` return ``stft_loss(recon, audio)`` - ``losses.MultiResolutionSTFTLoss``, the HIP restatement
of the ``auraloss`` loss the reference logs as ``val/loss`` / ``test/loss`` - through the
reference's ``_run_step``.  ``stft_loss`` is made on first use (in the reference ``configure_optimizers`` makes
it).  ``training_step`` and ``configure_optimizers`` raise on a model as constructed; they are behind the opt-in flag
``NeuralWaveshaping.differentiable``, which sets the links' own flags: the loss, the reverb and the noise
branch's filter have a backward pass, and so have a frame MLP and the control encoder (3.16, 3.17:
``ControlModule.differentiable``, ``.vjp``) and the oscillator branch (3.18: ``NEWT.differentiable``, ``.vjp``,
``Conv1x1.differentiable``); ``pre_reverb_graph`` composes them, for the flagged forward and for ``scripts/fit_newt.py``, and
``scripts/train.py`` is the training loop.  ``pre_reverb`` renders the reverb's input, which is what fitting ``reverb.ir`` alone needs;
``pre_reverb_parts`` renders it in two parts with the noise filter's input, which is what fitting the noise colour
needs.  Logging (``self.log``, wandb) is left to the caller.

Hidden inputs, exactly like the reference: every forward draws ``rand_like(osc.rand_phase)`` and then
``rand(control_hop*T - 1)`` from the default generator of the module's device, in that order
(generators.py:55, :30).  For parity testing the two draws can be injected with the keyword-only
arguments ``phase_u`` and ``noise``.
"""
import os

import torch
import torch.nn as nn

from .. import _lib
from .. import ginlite as gin
from ..engine import Engine, _req
from .modules import _standalone as sa
from .modules.dynamic import Conv1x1, TimeDistributedMLP, td_mlp_forward, td_mlp_vjp, upsample_linear
from .modules.generators import FIRNoiseSynth, HarmonicOscillator
from .modules.shaping import NEWT, Reverb

gin.external_configurable(nn.GRU, module="torch.nn")
gin.external_configurable(nn.Conv1d, module="torch.nn")

_DEFAULT_GIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gin", "models", "newt.gin")


_GRU_KEYS = ("gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0", "gru.bias_hh_l0")


class _ControlFunction(torch.autograd.Function):
    """ControlModule.forward with its backward attached (csrc/control_gru_grad.hip): saves x and gru_out; backward
    runs proj's part through td_mlp_vjp and the recurrence's through control_gru_grad and hands gradients to x and to every
    parameter that requires grad"""

    @staticmethod
    def forward(ctx, x, module, *params):
        with torch.no_grad():
            xd = x.detach()
            h = module._gru_out(xd)
            y = td_mlp_forward(h.transpose(1, 2).contiguous(), module.proj)
        ctx.module = module
        ctx.save_for_backward(xd, h)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_emb):
        x, h = ctx.saved_tensors
        want = any(ctx.needs_input_grad[2:])
        gx, grads = ctx.module._vjp(grad_emb, x, h, want)
        keys = _GRU_KEYS + ("proj.weight", "proj.bias")
        named = dict(ctx.module.named_parameters())
        out = [grads[k].view_as(named[k]) if need else None for k, need in zip(keys, ctx.needs_input_grad[2:])] if want else [None] * 6
        return (gx if ctx.needs_input_grad[0] else None, None, *out)


@gin.configurable
class ControlModule(nn.Module):
    """GRU(control_size -> hidden) + Conv1d(hidden -> embedding, 1) (reference :17-26).

    ``differentiable`` (a plain attribute, default False): forward only, as the stage kernels are.  Set to True (GRU(2 -> 128)
    only: the runtime-size recurrence has no backward), a forward under grad mode whose ``x`` or parameters require grad returns
    the same bits with a ``torch.autograd.Function`` attached that saves ``x`` and ``gru_out``; its backward hands gradients to
    ``x`` and to each of the six parameters that requires grad.  ``vjp`` is the same gradient without autograd."""

    differentiable = False      # also the value of a module unpickled from before the flag existed

    def __init__(self, control_size: int, hidden_size: int, embedding_size: int):
        super().__init__()
        self.gru = nn.GRU(control_size, hidden_size, batch_first=True)
        self.proj = nn.Conv1d(hidden_size, embedding_size, 1)
        self.differentiable = False

        self._desc = sa.Desc()

    def __getstate__(self):
        d = self.__dict__.copy()
        d["_desc"] = sa.Desc()
        return d

    def _checked(self, x):
        g = self.gru
        if g.num_layers != 1 or g.bidirectional or not g.batch_first:
            raise RuntimeError("the HIP path implements nn.GRU(control_size, hidden_size, batch_first=True), one layer")
        if x.dim() != 3 or x.shape[1] != g.input_size:
            raise RuntimeError(f"ControlModule: expected (B, {g.input_size}, T), got {tuple(x.shape)}")
        return g.input_size == 2 and g.hidden_size == sa._lib.HIDDEN

    def _wdesc(self):
        g = self.gru
        return self._desc.get({"gru_w_ih": g.weight_ih_l0, "gru_w_hh": g.weight_hh_l0, "gru_b_ih": g.bias_ih_l0,
                               "gru_b_hh": g.bias_hh_l0})

    def _gru_out(self, x):
        """(B, 2, T) -> gru_out (B, T, 128): the persistent GRU kernel on a checked, contiguous x"""
        return sa.binding().control_gru(self._wdesc(), x, None, False)[0]

    def _need_backward_sizes(self, x):
        if not self._checked(x):
            raise RuntimeError("ControlModule: the recurrence's backward (csrc/control_gru_grad.hip) exists for GRU(2 -> 128) only; "
                               f"this is GRU({self.gru.input_size} -> {self.gru.hidden_size}), which runs on the runtime-size path "
                               "and has no backward")

    def forward(self, x):
        """(B, control_size, T) -> (B, embedding_size, T): persistent GRU kernel (csrc/control_gru.hip) + Conv1d(k=1).
        Stand-alone form of what NeuralWaveshaping.forward runs fused (GRU, then proj inside frame_mlps16_kernel)."""
        if self.differentiable:
            xc = sa.contiguous(x.detach(), "x")
            self._need_backward_sizes(xc)
            if torch.is_grad_enabled():
                params = [dict(self.named_parameters())[k] for k in _GRU_KEYS + ("proj.weight", "proj.bias")]
                if x.requires_grad or any(p.requires_grad for p in params):
                    return _ControlFunction.apply(x if x.is_contiguous() else x.contiguous(), self, *params)
            return td_mlp_forward(self._gru_out(xc).transpose(1, 2).contiguous(), self.proj)
        x = sa.contiguous(x, "x")
        g = self.gru
        sa.no_autograd(inputs=(x,))
        if not self._checked(x):
            # any control_size / hidden_size: runtime-size recurrence (csrc/generic.hip: g_gru_kernel)
            ps = [sa._req(p.detach(), "gru parameter") for p in (g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0)]
            sa.no_autograd(params=[g.weight_ih_l0])
            h = sa.call("g_gru", ps[0], ps[1], ps[2], ps[3], x, None)[0]
        else:
            h = self._gru_out(x)                                        # (B, T, 128)
        return td_mlp_forward(h.transpose(1, 2).contiguous(), self.proj)

    def _vjp(self, grad_emb, x, gru_out, want_params):
        with torch.no_grad():
            g_h, pg = td_mlp_vjp(gru_out.transpose(1, 2).contiguous(), self.proj, grad_emb, want_params)      # dL/d(gru_out) (B, 128, T)
            out = sa.binding().control_gru_grad(self._wdesc(), x, None, gru_out, g_h.transpose(1, 2).contiguous(), None,
                                                bool(want_params))
            if not want_params:
                return out[0], {}
            grads = dict(zip(_GRU_KEYS, out[2:]))
            grads["proj.weight"], grads["proj.bias"] = pg["weight"], pg["bias"]
            return out[0], grads

    def vjp(self, grad_emb, x, want_params=True):
        """(dL/dx (B, 2, T), {state-dict key: gradient}) of ``forward`` at ``x`` for grad_emb = dL/d(emb) (B, embedding_size, T);
        keys ``gru.weight_ih_l0``, ``gru.weight_hh_l0``, ``gru.bias_ih_l0``, ``gru.bias_hh_l0``, ``proj.weight``, ``proj.bias``, an
        empty dict without ``want_params``.  Reruns the forward GRU kernel for gru_out, takes proj's part from ``td_mlp_vjp`` and the
        recurrence's from ``control_gru_grad``.  Whatever ``differentiable`` and the grad mode say; autograd is not
        involved and the results carry no graph."""
        with torch.no_grad():
            x = sa.contiguous(x.detach(), "x")
            self._need_backward_sizes(x)
            return self._vjp(grad_emb, x, self._gru_out(x), want_params)


@gin.configurable
class NeuralWaveshaping(nn.Module):
    def __init__(self, n_waveshapers: int, control_hop: int, sample_rate: float = 16000,
                 learning_rate: float = 1e-3, lr_decay: float = 0.9, lr_decay_interval: int = 10000,
                 log_audio: bool = False):
        super().__init__()
        self.hparams = dict(n_waveshapers=n_waveshapers, control_hop=control_hop, sample_rate=sample_rate,
                            learning_rate=learning_rate, lr_decay=lr_decay, lr_decay_interval=lr_decay_interval,
                            log_audio=log_audio)
        self.learning_rate = learning_rate
        self.lr_decay = lr_decay
        self.lr_decay_interval = lr_decay_interval
        self.control_hop = control_hop
        self.log_audio = log_audio
        self.sample_rate = sample_rate

        self.embedding = ControlModule()
        self.osc = HarmonicOscillator()
        self.harmonic_mixer = Conv1x1(self.osc.n_harmonics, n_waveshapers, 1)
        self.newt = NEWT()
        with gin.config_scope("noise_synth"):
            self.h_generator = TimeDistributedMLP()
            self.noise_synth = FIRNoiseSynth()
        self.reverb = Reverb()
        object.__setattr__(self, "_engine", Engine(self))

    # ---- cache hygiene: any re-homing / re-loading of parameters drops the pointer cache ----------
    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self._engine.invalidate()
        return out

    def load_state_dict(self, *a, **k):
        out = super().load_state_dict(*a, **k)
        self._engine.invalidate()
        return out

    def __setattr__(self, name, value):
        if name == "differentiable":
            value = bool(value)
            self._set_differentiable(value)
        super().__setattr__(name, value)
        if name == "newt" and "_engine" in self.__dict__:
            self._engine.invalidate()

    def invalidate_cache(self):
        """Drop the engine's cached pointer struct and derived tables.  In-place parameter updates are noticed on their own
        (Engine._fingerprint); needed only after writes through `p.data` or after changing `exciter_opts`."""
        self._engine.invalidate()

    # a copy / an unpickled model gets its own engine (the cache holds raw device pointers of THIS model's tensors)
    def __getstate__(self):
        d = self.__dict__.copy()
        d.pop("_engine", None)
        return d

    def __setstate__(self, state):
        super().__setstate__(state)
        object.__setattr__(self, "_engine", Engine(self))

    # ---- public surface ----------------------------------------------------------------------------
    def render_exciter(self, f0):
        """(B, 1, N) upsampled F0 in Hz -> (B, n_waveshapers, N) exciter (reference :64-67)."""
        f0 = _req(f0 if f0.is_contiguous() else f0.contiguous(), "f0")
        if f0.dim() != 3 or f0.shape[1] != 1:
            raise RuntimeError(f"expected (B, 1, N), got {tuple(f0.shape)}")
        if not self._engine.specialised() or f0.shape[-1] % _lib.HOP:
            # any n_harmonics / n_waveshapers / length: oscillator bank + Conv1d(k=1), runtime-size kernels (csrc/generic.hip)
            with torch.no_grad():
                osc = self.osc(f0[:, 0])
                mw = _req(self.harmonic_mixer.weight.detach(), "harmonic_mixer.weight")
                mb = _req(self.harmonic_mixer.bias.detach(), "harmonic_mixer.bias")
                return sa.call("g_conv1x1", osc, mw, mb)
        eng = self._engine
        f0_up = f0[:, 0]
        u = torch.rand_like(self.osc.rand_phase).reshape(-1)
        carry = eng.phase_carry(f0_up=f0_up)
        exc, _ = eng.exciter_newt(None, f0_up.contiguous(), carry, u, None, want_exciter=True, want_newt=False)
        return exc

    def get_embedding(self, control):
        """(B, C>=2, T) normalised control -> (B, 128, T) embedding (reference :69-72)."""
        control = _req(control if control.is_contiguous() else control.contiguous(), "control")
        if not self._engine.specialised():
            return self.embedding(control[:, 0:2].contiguous())       # (reference :70-72: f0 and loudness channels only)
        gru = self._engine.control_gru(control)
        emb, _, _, _ = self._engine.frame_mlps(gru, want_emb=True)
        return emb

    def _checked_inputs(self, f0, control, phase_u, noise):
        # strided views (control[:, :2], expand()) are accepted like in the reference: compacted by torch
        f0 = _req(f0 if f0.is_contiguous() else f0.contiguous(), "f0")
        control = _req(control if control.is_contiguous() else control.contiguous(), "control")
        if f0.dim() != 3 or f0.shape[1] != 1:
            raise RuntimeError(f"f0: expected (B, 1, T), got {tuple(f0.shape)}")
        if control.dim() != 3 or control.shape[1] < 2:
            raise RuntimeError(f"control: expected (B, C>=2, T), got {tuple(control.shape)}")
        B, _, T = f0.shape
        if control.shape[0] != B or control.shape[2] != T:
            raise RuntimeError(f"f0 {tuple(f0.shape)} and control {tuple(control.shape)} disagree on batch / frames")
        if T < 2:
            raise RuntimeError("need at least 2 control frames (reflect padding of the noise STFT, generators.py:31)")
        dev = f0.device
        sa.no_autograd(inputs=(f0, control))     # inference-only kernels: never hand back a graph-less result for grad inputs
        if phase_u is None:
            phase_u = torch.rand_like(self.osc.rand_phase)          # RNG draw #1 (generators.py:55)
        phase_u = _req(phase_u.reshape(-1), "phase_u", int(self.osc.n_harmonics))
        if noise is None:
            noise = torch.rand(self.control_hop * T - 1, device=dev)  # RNG draw #2 (generators.py:30)
        noise = _req(noise, "noise", self.control_hop * T - 1)
        return f0, control, phase_u, noise

    # ---- training (opt-in) ------------------------------------------------------------------------
    _TRAINED = ("newt", "embedding", "harmonic_mixer", "h_generator", "noise_synth", "reverb")

    # ``differentiable`` (default False, also the value of a model unpickled from before the flag existed): nothing carries a
    # graph and ``training_step`` and ``configure_optimizers`` raise.  Assigning it (``__setattr__``) sets ``differentiable`` of
    # ``embedding``, ``harmonic_mixer``, ``newt``, ``h_generator``, ``noise_synth``, ``reverb`` and ``stft_loss`` (a ``FastNEWT``
    # refuses: the lookup table has no backward, and then nothing is changed); False clears them.  Set to True, a forward under
    # grad mode with some parameter that requires grad runs the links one by one with their backwards attached
    # (``pre_reverb_graph(self, ..., "model")``, then ``reverb``) with the same two hidden draws in the same order; under
    # ``no_grad`` it is the fused forward as before, so validation during training stays on the fast path.  The two hooks then
    # are the reference's (models/neural_waveshaping.py:92-118).
    differentiable = False

    def _set_differentiable(self, value):
        for name in self._TRAINED:             # newt first: FastNEWT refuses True before anything has been changed
            getattr(self, name).differentiable = value
        self.stft_loss.differentiable = value

    def _wants_graph(self):
        return self.differentiable and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())

    def forward(self, f0, control, *, phase_u=None, noise=None):
        if self._wants_graph():
            return self.reverb(pre_reverb_graph(self, f0, control, "model", phase_u=phase_u, noise=noise))
        f0, control, phase_u, noise = self._checked_inputs(f0, control, phase_u, noise)
        if self._sub_module_hooks():
            return self._forward_module_by_module(f0, control, phase_u, noise)
        return self._engine.forward(f0, control, phase_u, noise)

    def pre_reverb(self, f0, control, phase_u=None, noise=None):
        """(B, N) input of ``self.reverb`` for the same draws as ``forward`` (reference :74-86: everything before :88), so that
        ``self.reverb(self.pre_reverb(...))`` is the forward within the parity bar.  Runs the stage kernels one module after
        the other under ``no_grad``: nothing upstream of the reverb has a backward, and the result carries no graph - it is
        what ``Reverb.vjp`` and a differentiable ``Reverb`` take as x (scripts/fit_reverb.py)."""
        f0, control, phase_u, noise = self._checked_inputs(f0, control, phase_u, noise)
        return self._pre_reverb_module_by_module(f0, control, phase_u, noise)

    def pre_reverb_parts(self, f0, control, phase_u=None, noise=None, want_emb=False):
        """``pre_reverb`` taken apart where the noise branch's backward starts: (newt_sum (B, N), H (B, 129, T), noise (N - 1)) -
        the summed oscillator branch, the noise filter magnitudes ``h_generator(emb)`` and the excitation draw, so that
        ``newt_sum + self.noise_synth(H, noise=noise)[:, 0]`` is ``pre_reverb`` for the same draws (the sum of the channels in
        another order: within the parity bar, not to the bit).  Same module-by-module kernels, under ``no_grad``; nothing
        carries a graph.  With ``noise_synth.differentiable`` a gradient reaches H (scripts/fit_noise.py).  ``want_emb``: also
        the control embedding (B, 128, T) that ``h_generator`` turned into H, as a fourth value - with
        ``h_generator.differentiable`` the gradient goes on from H to the MLP's parameters."""
        f0, control, phase_u, noise = self._checked_inputs(f0, control, phase_u, noise)
        with torch.no_grad():
            f0_up = upsample_linear(f0, int(self.control_hop))                    # :75
            sig = self.osc(f0_up[:, 0], phase_u=phase_u)                          # :65   (draw #1 injected / made above)
            x = self.harmonic_mixer(sig)                                          # :66
            emb = self.embedding(control[:, 0:2].contiguous())                    # :69-72
            x = self.newt(x, emb)                                                 # :80
            H = self.h_generator(emb)                                             # :82
            parts = (sa.sum_channels(x), H, noise)                                # :86 without the noise channel
            return parts + (emb,) if want_emb else parts

    # ---- evaluation hooks (reference :104-112, :136-165): inference + loss, no backward ----------------
    @property
    def stft_loss(self):
        """losses.MultiResolutionSTFTLoss() with the reference's (auraloss's default) resolutions, made on first use"""
        loss = self.__dict__.get("_stft_loss")
        if loss is None:
            from ..losses import MultiResolutionSTFTLoss

            loss = MultiResolutionSTFTLoss()
            self.__dict__["_stft_loss"] = loss       # not a sub-module: it holds no state and must not enter the state dict
        return loss

    def _run_step(self, batch):
        """reference :104-112 -> (loss, recon, audio)"""
        audio = batch["audio"].float()
        f0 = batch["f0"].float()
        control = batch["control"].float()

        recon = self(f0, control)

        if recon.shape[-1] != audio.shape[-1] or recon.shape[0] != audio.shape[0]:
            raise RuntimeError(f"the model rendered {tuple(recon.shape)} ({int(self.control_hop)} samples per control frame) but the "
                               f"batch's audio is {tuple(audio.shape)}: the loss compares signals of one length")
        loss = self.stft_loss(recon, audio.reshape(recon.shape))
        return loss, recon, audio

    def validation_step(self, batch, batch_idx):
        """reference :136-150 without the logging: the loss as a 0-dim tensor on the device (nothing is read back)"""
        with torch.no_grad():
            return self._run_step(batch)[0]

    def test_step(self, batch, batch_idx):
        """reference :152-165 without the logging; unlike there, the loss is returned"""
        with torch.no_grad():
            return self._run_step(batch)[0]

    def training_step(self, batch, batch_idx):
        """Under ``differentiable``: reference :114-118 without the logging - the loss of ``_run_step`` with its graph"""
        if self.differentiable:
            return self._run_step(batch)[0]
        raise NotImplementedError("training_step: there is no backward pass in this package behind this hook yet - every link has "
                                  "one when called on its own: the loss (losses.MultiResolutionSTFTLoss(differentiable=True)), the "
                                  "reverb (Reverb.differentiable, Reverb.vjp), the noise branch's filter "
                                  "(FIRNoiseSynth.differentiable, FIRNoiseSynth.vjp: dL/dH), a frame MLP "
                                  "(TimeDistributedMLP.differentiable, .vjp, td_mlp_vjp), the control encoder "
                                  "(ControlModule.differentiable, .vjp: the recurrence and proj) and the oscillator branch "
                                  "(NEWT.differentiable, NEWT.vjp, Conv1x1.differentiable for harmonic_mixer; DESIGN.md 3.18).  "
                                  "scripts/fit_newt.py --params model composes them into a step over every parameter; "
                                  "validation_step and test_step give the reference's loss, scripts/fit_reverb.py fits reverb.ir "
                                  "and scripts/fit_noise.py the noise colour.  The hook itself is behind an opt-in flag: set "
                                  "NeuralWaveshaping.differentiable = True (scripts/train.py does)")

    def configure_optimizers(self):
        """Under ``differentiable``: the reference's dictionary (:92-102) - Adam(lr) and StepLR(lr_decay_interval, lr_decay) stepped
        every optimiser step - with ``optim.Adam``, which also clips (set its ``max_grad_norm``)"""
        if self.differentiable:
            from ..optim import Adam

            optimizer = Adam(self.parameters(), lr=self.learning_rate)
            scheduler = torch.optim.lr_scheduler.StepLR(optimizer, self.lr_decay_interval, self.lr_decay)
            return {"optimizer": optimizer, "lr_scheduler": {"scheduler": scheduler, "interval": "step"}}
        raise NotImplementedError("configure_optimizers: there is no backward pass in this package behind the Lightning hooks yet "
                                  "(the loss, the reverb, the noise branch's filter, a frame MLP, the control encoder and the "
                                  "oscillator branch - NEWT.differentiable, NEWT.vjp - each have one when called on their own); "
                                  "scripts/fit_newt.py --params model builds the reference's Adam + StepLR from the model's hparams "
                                  "and steps every parameter, scripts/fit_reverb.py and scripts/fit_noise.py fit reverb.ir and the "
                                  "noise colour; model.stft_loss is made on first use instead.  The hook itself is behind an opt-in "
                                  "flag: set NeuralWaveshaping.differentiable = True (scripts/train.py does)")

    def _sub_module_hooks(self) -> bool:
        """Forward hooks on sub-modules (the reference's users tap stages that way, and so does tests/golden/make_golden.py on
        the reference itself): the fused forward never calls the sub-modules, so with hooks present the forward runs them one
        by one instead - the reference's own sequence (models/neural_waveshaping.py:74-90), one HIP stage kernel per module."""
        hit = self.__dict__.get("_hook_mods")
        if hit is None or hit[0] != _engine_epoch():
            # the hook registries themselves (one OrderedDict per module and kind, created once in Module.__init__): checking
            # ~90 dicts for emptiness is ~2 us per forward
            hit = (_engine_epoch(), [d for m in self.modules() if m is not self for d in (m._forward_hooks, m._forward_pre_hooks)])
            self.__dict__["_hook_mods"] = hit
        for d in hit[1]:
            if d:
                return True
        return False

    def _forward_module_by_module(self, f0, control, phase_u, noise):
        x = self._pre_reverb_module_by_module(f0, control, phase_u, noise)
        with torch.no_grad():
            return self.reverb(x)                                                 # :88

    def _pre_reverb_module_by_module(self, f0, control, phase_u, noise):
        with torch.no_grad():
            f0_up = upsample_linear(f0, int(self.control_hop))                    # :75
            sig = self.osc(f0_up[:, 0], phase_u=phase_u)                          # :65   (draw #1 injected / made above)
            x = self.harmonic_mixer(sig)                                          # :66
            emb = self.embedding(control[:, 0:2].contiguous())                    # :69-72
            x = self.newt(x, emb)                                                 # :80
            H = self.h_generator(emb)                                             # :82
            nz = self.noise_synth(H, noise=noise)                                 # :83   (draw #2)
            return sa.sum_channels(torch.cat((x, nz), dim=1))                     # :85-86 (cat: plumbing; the sum: a HIP kernel)

    # ---- checkpoints (Lightning .ckpt as shipped by the reference, or flat .npz fixtures) -------------
    @classmethod
    def load_from_checkpoint(cls, checkpoint_path, map_location=None, strict=True, **kwargs):
        from ..checkpoint import read_checkpoint

        ensure_default_config()
        state, hparams = read_checkpoint(checkpoint_path)
        hparams.update(kwargs)
        model = cls(**hparams)
        model.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()}, strict=strict)
        if map_location is not None:
            model = model.to(map_location)
        return model


def pre_reverb_graph(model, f0, control, mode, phase_u=None, noise=None):
    """The reverb's input (B, N) with the graph a mode needs, the links called one by one with whatever ``differentiable`` flags
    the caller has set; draws the two hidden inputs in the forward's order unless they are given.  ``mode`` "model": the control
    embedding carries its graph into both branches; anything else (scripts/fit_newt.py's "shapers" and "branch"): the embedding and
    the noise channel are rendered without one and only oscillator bank -> ``harmonic_mixer`` -> ``newt`` carries the gradient."""
    f0, control, phase_u, noise = model._checked_inputs(f0, control, phase_u, noise)
    with torch.no_grad():
        f0_up = upsample_linear(f0, int(model.control_hop))
        sig = model.osc(f0_up[:, 0], phase_u=phase_u)         # no parameters, and F0 is data: nothing goes further back
    ctl = control[:, 0:2].contiguous()
    if mode == "model":
        emb = model.embedding(ctl)
        nz = model.noise_synth(model.h_generator(emb), noise=noise)
    else:
        with torch.no_grad():
            emb = model.embedding(ctl)
            nz = model.noise_synth(model.h_generator(emb), noise=noise)
    x = model.newt(model.harmonic_mixer(sig), emb)
    return x[:, 0] + nz[:, 0]


def _engine_epoch():
    from ..engine import _EPOCH

    return _EPOCH[0]


def ensure_default_config():
    """Parse the packaged newt.gin if the caller has not parsed a model gin file yet."""
    try:
        gin.query_parameter("NeuralWaveshaping.control_hop")
    except ValueError:
        gin.parse_config_file(_DEFAULT_GIN)


def _stream(self, batch_size: int = 1, *, phase_u=None, noise=None, slots: bool = False, **kw):
    """Stateful streaming synthesiser bound to this model (see streaming.NewtStream; kw: max_chunk_frames, graph).  A model of
    another architecture than gin/models/newt.gin gets the same stream on the runtime-size kernels (streaming.GenericNewtStream).
    slots=True: B voice slots that start and stop on their own (streaming.VoiceStream; kw: graph; the packaged architecture only -
    `model.voices(B)` gives the slot stream of any architecture)."""
    from ..streaming import GenericNewtStream, NewtStream, VoiceStream

    if slots:
        return VoiceStream(self, batch_size, phase_u=phase_u, noise=noise, **kw)
    cls = NewtStream if self._engine.specialised() else GenericNewtStream
    return cls(self, batch_size, phase_u=phase_u, noise=noise, **kw)


def _voices(self, batch_size: int = 1, **kw):
    """B voice slots that start and stop on their own, for this model whatever its architecture (kw: phase_u, noise, graph):
    streaming.VoiceStream on the fused kernels for gin/models/newt.gin, streaming.GenericVoiceStream on the runtime-size kernels
     for every other configuration."""
    from ..streaming import voice_stream

    return voice_stream(self, batch_size, **kw)


def _player(self, voices: int, **kw):
    """Polyphonic note player bound to this model (see streaming.NotePlayer; kw: hop_frames, channels, the envelope and vibrato
    parameters, normalisation=(mean, std), phase_u, noise, graph): note_on / note_off in, one mixed signal out, hop by hop.  Any
    architecture with a two-channel control input: the player's stream is `model.voices(voices)`."""
    from ..streaming import NotePlayer

    return NotePlayer(self, voices, **kw)


NeuralWaveshaping.stream = _stream
NeuralWaveshaping.voices = _voices
NeuralWaveshaping.player = _player
