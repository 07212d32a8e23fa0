"""Stateful streaming synthesis: host side of csrc/stream.hip.

The reference's buffer benchmark (scripts/time_buffer_sizes.py) is stateless: every buffer restarts the GRU, the
oscillator phase and the reverb.  `NewtStream` carries that state so that the concatenation of the chunks it emits
equals the reference's ONE-SHOT forward over the whole signal up to the reverb input (`pre_reverb`), and applies the
learned reverb as a linear convolution of the stream instead of the one-shot path's wrap-around.

One `push` = ONE call of the binding (`engine.binding().stream_step` -> `nws_stream_step`): the one-shot kernels plus small streaming
kernels on a window = [last frame of the previous chunk] + [K new frames] - four launches for a hop of <= 256 samples (whatever
depends on nothing the hop computes, and the frame MLPs of its one or two frames, ride on the recurrence launch: DESIGN.md 3.8),
seven for longer chunks; every piece of state
(GRU h, previous frame, float64 phase sum, noise residue and window, reverb-input ring, position counters) lives in one
device blob behind fixed pointers.  Nothing is computed by torch.  Because the pointers and launch arguments of a
steady-state hop (same K as the previous push, not first, not final) never change, such hops are captured ONCE into a
hipGraph and replayed (`graph=True`, the default): a 256-sample hop is then one graph launch.

  * the stream emits audio 64 samples (4 ms) behind the control frames it has seen (linear upsampling looks one frame
    ahead); `push(..., final=True)` releases the remainder exactly like the one-shot forward's right edge;
  * the phase offsets are drawn once per stream and the noise chunk by chunk from the device generator (or both are
    injected for parity testing), mirroring the reference's two hidden draws;
  * chunk size changes bits at the 1e-6 level: the same frames pushed in other chunk sizes give the same signal to 1e-5 of its
    RMS, not bit for bit (hops of one or two frames take another frame-MLP kernel than longer chunks, chunks beyond 2048
    samples sum the reverb in another order).

`VoiceStream` (`model.stream(B, slots=True)`, `nws_stream_step_slots`) is the slot mode: B voices that start and stop on their
own in one batched stream, with per-slot events as device data; its docstring states the contract.

Which kernel family serves a stream is one object, its path: `_FusedPath` (the packaged architecture) or `_GenericPath` (any other
bank, harmonic count, layer sizes, sample rate, reverb length: `nws_g_stream_step` / `nws_g_stream_step_slots`, the runtime-size
kernels).  `GenericNewtStream` and `GenericVoiceStream` are the two streams with the second path and nothing
else of their own; `model.stream` and `model.voices(B)` pick the class.

`NotePlayer` (`model.player(voices)`) plays notes on that slot stream: `nws_note_control` writes every slot's controls
of a hop from the notes, `nws_voice_mix` sums the slots into one signal; `NoteBook` is its host-side scheduling.
"""
from __future__ import annotations

import ctypes as C
import math
import time
import warnings

import numpy as np
import torch

from . import _lib
from .engine import _req, binding, stream_ptr

HOP = _lib.HOP
_MAX_CHUNK_FRAMES = 249   # 16 kHz: (K+1) * 128 + 31999 <= 64000, the FFT reverb of a long chunk inside the L = 64000 plan
_RING = 65536             # kRing of csrc/stream.hip: reverb-input ring per utterance; the impulse response must fit half of it
_GRAPH_AFTER = 2          # consecutive steady-state pushes of one (K, channels) before that hop is captured


class _FusedPath:
    """What a stream asks of the kernel family that serves its model; here the fused kernels (the architecture of
    gin/models/newt.gin), in _GenericPath the same calls for the runtime-size kernels.  Construction refuses a model the family does
    not serve and reads `dev`, `ir_len`, `n_harmonics` and `control_size` from the family's own record of the model; a call that
    needs the stream's state takes the stream `s`.  The two path classes are this module's only code that touches engine privates."""

    def __init__(self, model, slots: bool):
        self.eng = eng = model._engine
        if not eng.specialised():
            raise RuntimeError("stateful streaming runs on the fused kernels: the model must have the architecture of "
                               "gin/models/newt.gin" + (" - model.voices(B) gives the slot stream of any architecture" if slots else ""))
        _, _, self.dev = eng.weights()
        self.ir_len = int(eng.ir().numel())
        self.n_harmonics, self.control_size = _lib.N_HARMONICS, 2

    # ---- the watch on the weights -------------------------------------------------------------------------------------
    def record(self):
        """The engine's current record of pointers and derived tables (replaced, never edited, on a rebuild)."""
        return self.eng.record()

    def rewalk(self):
        """One fingerprint walk over an existing record; rebuilds it if a parameter changed (drains the device first)."""
        if self.eng.record() is not None:
            self.eng._wd()

    def settle(self):
        """In front of a capture.  Nothing to do here: a step that finds the record stale inside a capture raises (Engine._wd), the
        capture fails and the stream goes on with eager pushes."""

    def reverb_aux(self, plan_n):
        """(plan, tables, IR spectrum, plan tensor) of the FFT reverb length `plan_n`, for the current weights."""
        return self.eng.reverb_aux(plan_n)

    # ---- sizing ---------------------------------------------------------------------------------------------------------
    def state_bytes(self, B, max_frames, plan):
        return _lib.lib().nws_stream_state_bytes(B, max_frames, self.ir_len, C.byref(plan) if plan is not None else None)

    def slot_state_bytes(self, B, max_frames):
        """(bytes of a slot stream's state, offset of its counters: where `gave_up` reads the flag)"""
        L = _lib.lib()
        return L.nws_stream_slot_state_bytes(B, max_frames, self.ir_len), int(L.nws_stream_counters_offset(B, max_frames, self.ir_len))

    # ---- one call of the binding ------------------------------------------------------------------------------------
    def step(self, s, f0_2d, control, first, final, noise_new, out, pre):
        eng = self.eng
        r = eng._wd()
        _, tables, spec, plan_t = eng._reverb_aux(s._plan_n) if s._need_fft else (None, None, None, None)
        binding().stream_step(r.wdesc, r.fir_design, plan_t, tables, spec, s._state, s.max_frames, f0_2d, control, bool(first),
                              bool(final), int(s.frames_seen), int(s._nz_prev_start), eng.osc_sample_rate(), s.phase_u,
                              r.rand_phase, noise_new, s._noise_all, r.ir.reshape(-1), out, pre)

    def step_slots(self, s, f0_2d, control, noise_new, out, pre):
        eng = self.eng
        r = eng._wd()
        binding().stream_step_slots(r.wdesc, r.fir_design, s._state, s.max_frames, f0_2d, control, int(s.frames_seen),
                                    int(s._nz_prev_start), eng.osc_sample_rate(), s.phase_u, r.rand_phase, noise_new,
                                    s._noise_all, r.ir.reshape(-1), s._ev, out, pre)

    def reverb_tail(self, s, plan, tables, spec, tail, ws, nb):
        _lib.check(_lib.lib().nws_stream_reverb_tail(C.byref(plan), tables.data_ptr(), spec.data_ptr(), s._state.data_ptr(),
                                                     s._state.numel(), s.B, s.max_frames, self.ir_len, tail.data_ptr(),
                                                     ws.data_ptr(), nb, stream_ptr(self.dev)), "nws_stream_reverb_tail")

    def gave_up(self, s) -> bool:
        """Did a slot hop's device work report that it gave up waiting (counters[5])?  Synchronises."""
        return int(s._state[s._counters_at + 40: s._counters_at + 48].cpu().view(torch.int64)[0]) != 0


class _GenericPath:
    """_FusedPath for a model that `Engine.specialised()` turns down (another bank, harmonic count, GRU / MLP size, sample rate,
    reverb length, several NEWT output channels): the runtime-size stage kernels of csrc/generic.hip on the window, the noise
    branch, ring and reverb of csrc/stream.hip.  The noise branch, the ring and the 64-sample emission delay
    are the packaged stream's, so three sizes are fixed: control hop 128, 256 noise taps, a window symmetric about tap 128.  What it
    watches for weight updates is the GenericEngine's descriptor record."""

    def __init__(self, model, slots: bool):
        self.eng = eng = model._engine
        m, ns = model, model.noise_synth
        if int(m.control_hop) != HOP or int(ns.hop_length) != HOP:
            raise RuntimeError(f"stateful streaming runs at a control hop of {HOP} samples: this model has control_hop = "
                               f"{int(m.control_hop)}, FIRNoiseSynth.hop_length = {int(ns.hop_length)} - render it with the one-shot "
                               f"forward, which serves every hop")
        if int(ns.ir_length) != _lib.FIR_LEN:
            raise RuntimeError(f"stateful streaming filters the noise with {_lib.FIR_LEN} taps per frame: this model has "
                               f"FIRNoiseSynth.ir_length = {int(ns.ir_length)} - render it with the one-shot forward, which serves "
                               f"every even length")
        if not eng._window_symmetric():
            w = ns.window.detach().float().cpu()
            asym = float((w[1:HOP] - w[HOP + 1:].flip(0)).abs().max())
            raise RuntimeError(f"stateful streaming hands half of every frame's noise taps on: the window must be symmetric about tap "
                               f"{HOP} with window[0] = 0, this model's has window[0] = {float(w[0]):.6g} and differs by up to "
                               f"{asym:.3g} between mirrored taps - render it with the one-shot forward, which serves every window")
        r = eng.generic.model_desc()
        self.dev, self.ir_len = r.device, int(r.ir.numel())
        self.n_harmonics, self.control_size = int(r.struct.n_harmonics), int(r.struct.control_size)

    def record(self):
        return self.eng.generic.record()

    def rewalk(self):
        self.eng.generic.model_desc()

    settle = rewalk     # a rebuild synchronises: in front of the capture, never inside it

    def reverb_aux(self, plan_n):
        g = self.eng.generic
        r = g.model_desc()
        return g._reverb_aux(plan_n, r.device, r.ir)

    def _served(self, nbytes):
        if nbytes == 0:
            raise RuntimeError("stateful streaming: the runtime-size kernels do not serve this model's layer sizes - render it "
                               "with the one-shot forward")
        return nbytes

    def state_bytes(self, B, max_frames, plan):
        r = self.eng.generic.model_desc()
        return self._served(_lib.lib().nws_g_stream_state_bytes(C.byref(r.struct), B, max_frames, self.ir_len,
                                                                C.byref(plan) if plan is not None else None))

    def slot_state_bytes(self, B, max_frames):
        r = self.eng.generic.model_desc()
        return self._served(_lib.lib().nws_g_stream_slot_state_bytes(C.byref(r.struct), B, max_frames, self.ir_len)), None

    def step(self, s, f0_2d, control, first, final, noise_new, out, pre):
        g = self.eng.generic
        r = g.model_desc()
        _, tables, spec, plan_t = g._reverb_aux(s._plan_n, r.device, r.ir) if s._need_fft else (None, None, None, None)
        binding().g_stream_step(r.gdesc, plan_t, tables, spec, s._state, s.max_frames, f0_2d, control, bool(first), bool(final),
                                int(s.frames_seen), int(s._nz_prev_start), self.eng.osc_sample_rate(), s.phase_u,
                                r.rand_phase, noise_new, s._noise_all, out, pre)

    def step_slots(self, s, f0_2d, control, noise_new, out, pre):
        r = self.eng.generic.model_desc()
        binding().g_stream_step_slots(r.gdesc, s._state, s.max_frames, f0_2d, control, int(s.frames_seen),
                                      int(s._nz_prev_start), self.eng.osc_sample_rate(), s.phase_u, r.rand_phase, noise_new,
                                      s._noise_all, s._ev, out, pre)

    def reverb_tail(self, s, plan, tables, spec, tail, ws, nb):
        r = self.eng.generic.model_desc()
        _lib.check(_lib.lib().nws_g_stream_reverb_tail(C.byref(r.struct), C.byref(plan), tables.data_ptr(), spec.data_ptr(),
                                                       s._state.data_ptr(), s._state.numel(), s.B, s.max_frames, tail.data_ptr(),
                                                       ws.data_ptr(), nb, stream_ptr(self.dev)), "nws_g_stream_reverb_tail")

    def gave_up(self, s) -> bool:
        """Synchronises; the runtime-size hop has no wait inside a launch and so nothing it could have given up on."""
        torch.cuda.synchronize(self.dev)
        return False


class _StreamBase:
    """What NewtStream and VoiceStream share: the opening of a stream, the captured steady-state hop and its fall-back to eager
    pushes, the watch on the engine's weights record, and the reverb tail.  Whatever depends on the kernel family goes through
    `self._path`, an object of the class `_PATH` names (the one thing the Generic* subclasses change).  A subclass provides
    `_steady_step(f0_2d, control, noise_new, out, pre)`: one steady-state hop through the binding."""

    _PATH = _FusedPath

    def _open(self, model, batch_size, phase_u, slots):
        """The opening, before the subclass sizes its state: the path with its refusals, the ring refusal, the FFT reverb length
        and the stream's one phase draw."""
        self.model, self.eng = model, model._engine
        self._path = p = self._PATH(model, slots)
        self.dev, self._ir_len, self.B = p.dev, p.ir_len, int(batch_size)
        if slots and self.B < 1:
            raise RuntimeError("VoiceStream: at least one slot")
        self.tail_len = self._ir_len + 1
        if self._ir_len >= _RING // 2:
            span = "" if slots else f" ({self._ir_len / float(model.sample_rate):.2f} s at {model.sample_rate} Hz)"
            raise RuntimeError(f"stateful streaming keeps {_RING // 2 - 1} samples of reverb history per {'slot' if slots else 'utterance'}; "
                               f"this model's impulse response has {self._ir_len} taps{span} - render it with the one-shot forward")
        # the FFT reverb of a long chunk is one direct transform of [ir_len samples of history | chunk]: the smallest standard
        # length that holds twice the tail (64000 at 16 kHz, 32000 at 8 kHz) bounds the chunk
        self._plan_n = next(n for n in (32000, 64000, 128000, 256000) if n >= 2 * self.tail_len)
        self.phase_u = _req((phase_u if phase_u is not None else torch.rand_like(model.osc.rand_phase)).reshape(-1),
                            "phase_u", p.n_harmonics)

    def _alloc(self, nbytes, graph):
        """The rest of the opening: the state blob, reset, and the bookkeeping of positions and captured hops."""
        with torch.cuda.device(self.dev):
            self._state = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
            _lib.check(_lib.lib().nws_stream_reset(self._state.data_ptr(), nbytes, stream_ptr(self.dev)), "nws_stream_reset")
        self._use_graph = bool(graph)
        self._graphs = {}          # (K, channels) -> (graph, f0_in, control_in, noise_new, out, pre)
        self._steady_runs = {}     # (K, channels) -> CONSECUTIVE steady-state pushes seen
        self.frames_seen = 0       # (the slot stream counts its pre-roll in)
        self._nz_prev_start = 0
        self._last_K = None
        self._last_pre = None
        self.finished = False

    def _capture(self, K, C_in):
        """hipGraph of one steady-state hop of K frames: static input / output buffers, the fresh noise draws inside."""
        dev = self.dev
        self._path.settle()
        with torch.cuda.device(dev):
            f0_in = torch.zeros((self.B, K), dtype=torch.float32, device=dev)
            c_in = torch.zeros((self.B, C_in, K), dtype=torch.float32, device=dev)
            nz = torch.empty(HOP * K, dtype=torch.float32, device=dev) if self._noise_all is None else None
            out = torch.empty((self.B, HOP * K), dtype=torch.float32, device=dev)
            pre = torch.empty((self.B, HOP * K), dtype=torch.float32, device=dev)
            g = torch.cuda.CUDAGraph()
            torch.cuda.synchronize(dev)
            with torch.cuda.graph(g):
                if nz is not None:
                    nz.uniform_()                                  # the reference's torch.rand draw, chunk by chunk
                self._steady_step(f0_in, c_in, nz, out, pre)
        # capture records, it does not run: the state has not advanced
        return g, f0_in, c_in, nz, out, pre

    def _captured_hop(self, key, may_capture):
        """The captured hop of key = (K, channels), or None.  With `may_capture` a missing one is captured now; where that is not
        possible (e.g. a foreign capture in progress) the stream stays eager from now on, and says so."""
        hit = self._graphs.get(key)
        if hit is None and may_capture:
            try:
                hit = self._graphs[key] = self._capture(*key)
            except Exception as e:
                warnings.warn(f"{type(self).__name__}: hipGraph capture of the {key[0]}-frame hop failed ({type(e).__name__}: {e}); this "
                              f"stream continues with eager pushes", RuntimeWarning, stacklevel=3)
                self._use_graph = False
        return hit

    def refresh(self):
        """Pick up a weight update NOW: re-derive the engine's tables if any parameter changed and drop the captured hops that
        point into the old ones.  Call it after an optimizer step / load_state_dict / in-place edit when the very next hop must
        see the new weights; without it a captured hop (`graph=True`) keeps replaying the old tables for up to 250 ms (eager
        pushes notice at once), see _check_weights."""
        self.__dict__["_last_walk"] = 0.0
        self._check_weights()

    def _check_weights(self):
        """A captured hop holds raw pointers into the engine's derived tables (fragment tables, LUT pairs, FIR design, IR
        spectrum).  If the engine has rebuilt them (somebody ran a forward after a weight update, `.to()`, `invalidate_cache`)
        the graphs are dropped and re-captured; in-place updates nobody has told the engine about are looked for at most every
        250 ms of wall-clock (a full fingerprint walk costs ~12 us of host time: too much for every 256-sample hop, nothing once
        per sixteen 16 ms hops).  So for up to 250 ms after such an update graph=True and graph=False streams differ; `refresh()`
        closes that window on demand."""
        now = time.monotonic()
        if now - self.__dict__.get("_last_walk", 0.0) >= 0.25:
            self._last_walk = now
            self._path.rewalk()
        rec = self._path.record()
        if rec is not self.__dict__.get("_w_seen"):
            if self._graphs:
                torch.cuda.synchronize(self.dev)
                self._graphs.clear()
                self._steady_runs.clear()
            self._w_seen = rec

    def reverb_tail(self) -> torch.Tensor:
        """The remaining (B, ir_len + 1) reverb tail of every row after the last chunk (what a linear reverb still rings out)."""
        plan, tables, spec, _ = self._path.reverb_aux(self._plan_n)
        with torch.cuda.device(self.dev):
            tail = torch.empty((self.B, self.tail_len), dtype=torch.float32, device=self.dev)
            nb = 2 * ((self.B * (2 * self._ir_len + 1) * 4 + 255) // 256 * 256) + _lib.lib().nws_reverb_workspace_bytes(C.byref(plan), self.B)
            ws = torch.empty(nb, dtype=torch.uint8, device=self.dev)
            self._path.reverb_tail(self, plan, tables, spec, tail, ws, nb)
        return tail


class NewtStream(_StreamBase):
    def __init__(self, model, batch_size: int, phase_u: torch.Tensor | None = None, noise: torch.Tensor | None = None,
                 max_chunk_frames: int = _MAX_CHUNK_FRAMES, graph: bool = True):
        self._open(model, batch_size, phase_u, slots=False)
        fit = (self._plan_n - self._ir_len) // HOP - 1
        self.max_frames = int(min(max(1, max_chunk_frames), fit))
        self._noise_all = _req(noise, "noise") if noise is not None else None    # parity mode: the reference's whole draw
        self.samples_emitted = 0
        self._need_fft = HOP * (self.max_frames + 1) > 2048
        plan = self._path.reverb_aux(self._plan_n)[0] if self._need_fft else None
        self._alloc(self._path.state_bytes(self.B, self.max_frames, plan), graph)

    # ---- one call of the binding ------------------------------------------------------------------------------------
    def _step(self, f0_2d, control, first, final, noise_new, out, pre):
        self._path.step(self, f0_2d, control, first, final, noise_new, out, pre)

    def _steady_step(self, f0_2d, control, noise_new, out, pre):
        self._path.step(self, f0_2d, control, False, False, noise_new, out, pre)

    # ---- one chunk ----------------------------------------------------------------------------------------------------
    def push(self, f0: torch.Tensor, control: torch.Tensor, final: bool = False) -> torch.Tensor:
        """f0 (B,1,K) Hz, control (B,C>=2,K) normalised  ->  (B, 128K) audio (128K-64 for the first chunk, 128K+64
        for the chunk marked `final`, which ends the stream exactly like the one-shot forward's right edge)."""
        if self.finished:
            raise RuntimeError("stream already finished")
        f0 = _req(f0 if f0.is_contiguous() else f0.contiguous(), "f0")
        control = _req(control if control.is_contiguous() else control.contiguous(), "control")
        B, _, K = f0.shape
        if B != self.B or control.shape[0] != B or control.shape[2] != K or control.shape[1] < 2:
            raise RuntimeError(f"expected f0 ({self.B},1,K) and control ({self.B},C>=2,K)")
        if K < 1:
            raise RuntimeError("empty chunk")
        if K > self.max_frames:                          # long chunks: process in pieces (state makes that exact)
            outs = []
            for k0 in range(0, K, self.max_frames):
                k1 = min(K, k0 + self.max_frames)
                outs.append(self.push(f0[:, :, k0:k1], control[:, :, k0:k1], final and k1 == K))
            return torch.cat(outs, dim=1)
        first = self.frames_seen == 0
        L = _lib.lib()
        M = L.nws_stream_out_samples(K, int(first), int(final))
        if M <= 0:
            raise RuntimeError("a first chunk of one frame that is also not final emits 64 samples; nothing smaller exists")
        steady = (not first) and (not final) and self._last_K == K and self.frames_seen >= K + 2
        f0_2d = f0[:, 0, :]
        self._check_weights()
        key = (K, control.shape[1])
        if not steady:
            self._steady_runs.clear()      # the count is of CONSECUTIVE steady hops of one shape
        if steady and self._use_graph:
            runs = self._steady_runs.get(key, 0) + 1
            self._steady_runs = {key: runs}
            hit = self._captured_hop(key, runs > _GRAPH_AFTER and not torch.cuda.is_current_stream_capturing())
            if hit is not None:
                g, f0_in, c_in, _, out, pre = hit
                torch._foreach_copy_([f0_in, c_in], [f0_2d, control])      # one multi-tensor launch for both inputs
                g.replay()
                self._advance(K, M, first, final)
                self._last_pre = pre
                return out.clone()
        with torch.cuda.device(self.dev):
            out = torch.empty((B, M), dtype=torch.float32, device=self.dev)
            pre = torch.empty((B, M), dtype=torch.float32, device=self.dev)
            nz = None
            if self._noise_all is None:
                nz = torch.rand(L.nws_stream_noise_draws(K, int(first), self.frames_seen), device=self.dev)   # RNG draw #2, chunk-wise
            self._step(f0_2d.contiguous(), control, first, final, nz, out, pre)
        self._advance(K, M, first, final)
        self._last_pre = pre
        return out

    # ---- zero-copy hops: the caller writes into the captured hop's own input buffers and reads its output buffer ----------
    def static_io(self, K: int, channels: int = 2):
        """(f0_in (B, K), control_in (B, channels, K), out (B, 128 K)) of the captured steady-state hop of K frames - the
        buffers `hop()` consumes and fills, for callers that produce control frames in place (an audio callback): no input
        copies, no output copy.  Needs the stream in steady state for this K (two pushes of K frames behind it)."""
        if not (self.frames_seen >= K + 2 and self._last_K == K and not self.finished):
            raise RuntimeError(f"static_io({K}): push at least two chunks of {K} frames first (the captured hop is the steady-state one)")
        hit = self._graphs.get((K, channels))
        if hit is None:
            hit = self._graphs[(K, channels)] = self._capture(K, channels)
        return hit[1], hit[2], hit[4]

    def hop(self, K: int, channels: int = 2) -> torch.Tensor:
        """Replay the captured hop on whatever the caller left in static_io(K)'s input buffers; returns the static output
        buffer (overwritten by the next hop)."""
        self._check_weights()
        hit = self._graphs.get((K, channels))
        if hit is None or self._last_K != K or self.finished or self.frames_seen < K + 2:
            raise RuntimeError("hop(): call static_io(K) first (again after a weight update), and do not interleave other chunk sizes")
        hit[0].replay()
        self._advance(K, HOP * K, False, False)
        self._last_pre = hit[5]
        return hit[4]

    def _advance(self, K, M, first, final):
        self._nz_prev_start = int(_lib.lib().nws_stream_noise_start(int(first), self.frames_seen))
        self.frames_seen += K
        self.samples_emitted += M
        self._last_K = K
        self.finished = bool(final)


class GenericNewtStream(NewtStream):
    """NewtStream for a model that `Engine.specialised()` turns down: the same contract and methods on the runtime-size kernels,
    one push = one `g_stream_step` of the binding (`nws_g_stream_step`).  _GenericPath states what it needs."""

    _PATH = _GenericPath


# ---- slot mode: B voices with their own lifetimes in one batched stream ------------------------------------------------
SLOT_START, SLOT_STOP, SLOT_RELEASE, SLOT_ACTIVE = 1, 2, 4, 8   # include/nws_hip.h NWS_SLOT_*
IDLE, ACTIVE, RELEASING = "idle", "active", "releasing"
_SLOT_MAX_FRAMES = 16     # hops of up to 2048 samples: the time-domain reverb
_PREROLL = 2              # internal all-idle frames in front of the first hop (the first user hop is then an ordinary one)


def _slot_set(sel, B: int, what: str) -> set:
    """A bool mask of B entries or a list of slot indices -> set of slot indices."""
    if sel is None:
        return set()
    if isinstance(sel, torch.Tensor):
        sel = sel.detach().cpu()
        if sel.dtype == torch.bool:
            if sel.numel() != B:
                raise RuntimeError(f"{what}: a bool mask needs {B} entries, got {sel.numel()}")
            return set(int(i) for i in torch.nonzero(sel.reshape(-1)).reshape(-1).tolist())
        sel = sel.reshape(-1).tolist()
    elif hasattr(sel, "dtype") and str(getattr(sel, "dtype")) == "bool":     # numpy bool mask
        sel = list(sel)
        if len(sel) != B:
            raise RuntimeError(f"{what}: a bool mask needs {B} entries, got {len(sel)}")
        return {i for i, v in enumerate(sel) if v}
    sel = list(sel)
    if sel and all(isinstance(v, bool) for v in sel):
        if len(sel) != B:
            raise RuntimeError(f"{what}: a bool mask needs {B} entries, got {len(sel)}")
        return {i for i, v in enumerate(sel) if v}
    out = set()
    for v in sel:
        i = int(v)
        if not 0 <= i < B:
            raise RuntimeError(f"{what}: slot {i} outside 0 .. {B - 1}")
        out.add(i)
    return out


class SlotBook:
    """Host-side slot state machine of a VoiceStream (no GPU): idle -> active on start, active -> releasing for the one hop after
    the stop hop, releasing -> idle after it.  `plan` validates one hop's events and returns the per-slot event words without
    changing anything; `commit` applies them once the hop has been issued."""

    def __init__(self, B: int):
        self.B = int(B)
        self.states = [IDLE] * self.B

    def plan(self, start=None, stop=None) -> list:
        st, sp = _slot_set(start, self.B, "start"), _slot_set(stop, self.B, "stop")
        for i in sorted(st):
            if self.states[i] != IDLE:
                raise RuntimeError(f"start on slot {i}: it is {self.states[i]} (a start is accepted on an idle slot only)")
        for i in sorted(sp - st):
            if self.states[i] != ACTIVE:
                raise RuntimeError(f"stop on slot {i}: it is {self.states[i]} (a stop is accepted on an active slot, or with a start)")
        words = []
        for i, s in enumerate(self.states):
            if i in st:
                w = SLOT_ACTIVE | SLOT_START | (SLOT_STOP if i in sp else 0)
            elif s == ACTIVE:
                w = SLOT_ACTIVE | (SLOT_STOP if i in sp else 0)
            elif s == RELEASING:
                w = SLOT_RELEASE
            else:
                w = 0
            words.append(w)
        return words

    def commit(self, words) -> None:
        for i, w in enumerate(words):
            if w & SLOT_STOP:
                self.states[i] = RELEASING
            elif w & SLOT_ACTIVE:
                self.states[i] = ACTIVE
            else:
                self.states[i] = IDLE


class VoiceStream(_StreamBase):
    """B voice slots in one batched stream, each starting and stopping on its own (`model.stream(B, slots=True)`).

    One hop = K frames (1 <= K <= 16) for every slot, `push(f0, control, start=, stop=)` -> (B, 128 K), every hop the same shape.
    Events per slot and hop (`start` / `stop`: bool masks of B entries or lists of slot indices):
      * start: this hop's frames are a new voice's first frames; accepted on an IDLE slot only;
      * stop: this hop's frames are the voice's last frames; accepted on an ACTIVE slot, or together with a start;
      * a slot is RELEASING for the one hop after its stop hop (its voice's last 64 samples come out), then IDLE again.
    A violation raises RuntimeError before anything is launched; the stream stays usable.

    Output: slot b's output is one continuous signal o_b; the hop covering frames [a, a+K) (a = 0 for the first hop) returns
    o_b[128 a : 128 a + 128 K].  A voice v of slot b starting at frame a_v with T_v frames has the dry signal pre_v = the
    one-shot forward's `pre_reverb` of its own (f0, control), with the stream's single phase draw (shared by all voices, as the
    reference shares it over a batch) and the noise samples noise[128 a_v : 128 a_v + 128 T_v - 1] of the stream's noise sequence
    (reflect-padded at both ends exactly like the one-shot).  pre_v sits at o-indices [128 a_v + 64, 128 (a_v + T_v) + 64) - the
    64-sample latency of every stream.  The slot's dry signal is the sum of its placed voices and exactly 0 everywhere else, and
    o_b = dry_b + linear_conv(dry_b, [0, ir]): reverb tails of ended voices keep ringing, also under a later voice of the slot.
    Idle and releasing slots' f0 / control are never read into an output (NaN there is harmless).

    Draws: phase_u once per stream; in drawn mode every hop draws 128 K noise samples whatever its events, so one captured hop per
    K stays valid.  Parity mode (`noise=`): the stream's whole noise sequence, at least 128 F - 1 samples for F frames pushed in
    all (samples past its end read as 0).

    `static_io(K)` -> (f0_in, control_in, events, out): the captured hop's own buffers; `hop(K, start=, stop=)` writes the
    events and replays ONE graph per K whatever they are.  `check()` raises if the device reported a hop it had to give up on.
    """

    def __init__(self, model, batch_size: int, phase_u: torch.Tensor | None = None, noise: torch.Tensor | None = None,
                 graph: bool = True):
        self._open(model, batch_size, phase_u, slots=True)
        dev = self.dev
        self.max_frames = _SLOT_MAX_FRAMES
        self._noise_all = None
        if noise is not None:
            nz = _req(noise, "noise").reshape(-1)
            # the pre-roll's frames come first in the device's noise positions: its samples are never read into an output
            self._noise_all = torch.cat([torch.zeros(HOP * _PREROLL, dtype=nz.dtype, device=nz.device), nz])
        nbytes, self._counters_at = self._path.slot_state_bytes(self.B, self.max_frames)   # (no counters offset: no give-up flag)
        self._alloc(nbytes, graph)
        self.book = SlotBook(self.B)
        self._ev_words = [0] * self.B
        self.hops = 0
        L = _lib.lib()
        # pre-roll: every slot idle, output dropped; afterwards each hop is an ordinary (not first) one of the same shape
        with torch.cuda.device(dev):
            self._ev = torch.zeros(self.B, dtype=torch.int32, device=dev)     # the hop's event words, read by its launches
            f0 = torch.zeros((self.B, _PREROLL), dtype=torch.float32, device=dev)
            c = torch.zeros((self.B, self._path.control_size, _PREROLL), dtype=torch.float32, device=dev)
            M = L.nws_stream_out_samples(_PREROLL, 1, 0)
            out = torch.empty((self.B, M), dtype=torch.float32, device=dev)
            nz = torch.rand(L.nws_stream_noise_draws(_PREROLL, 1, 0), device=dev) if self._noise_all is None else None
            self._step(f0, c, nz, out, None)
        self._advance(_PREROLL)
        self._last_K = None

    # ---- one call of the binding ------------------------------------------------------------------------------------
    def _step(self, f0_2d, control, noise_new, out, pre):
        self._path.step_slots(self, f0_2d, control, noise_new, out, pre)

    _steady_step = _step

    def _set_events(self, words):
        # one host-to-device copy per hop whose words differ from the last ones written (a copy costs a few us of the hop's
        # latency; a hop without events and without a release repeats the previous words)
        if words == self._ev_words:
            return
        host = torch.tensor(words, dtype=torch.int32).pin_memory()
        self._ev.copy_(host, non_blocking=True)
        self._ev_words = list(words)

    def _steady(self, K):
        return self._last_K == K and self.hops >= 1

    def _check_shape(self, f0, control):
        f0 = _req(f0 if f0.is_contiguous() else f0.contiguous(), "f0")
        control = _req(control if control.is_contiguous() else control.contiguous(), "control")
        if f0.dim() != 3 or control.dim() != 3:
            raise RuntimeError(f"expected f0 ({self.B},1,K) and control ({self.B},C>=2,K)")
        B, one, K = f0.shape
        if B != self.B or one != 1 or control.shape[0] != B or control.shape[2] != K or control.shape[1] < 2:
            raise RuntimeError(f"expected f0 ({self.B},1,K) and control ({self.B},C>=2,K), got {tuple(f0.shape)} / {tuple(control.shape)}")
        if not 1 <= K <= _SLOT_MAX_FRAMES:
            raise RuntimeError(f"slot mode serves hops of 1 .. {_SLOT_MAX_FRAMES} frames (up to 2048 samples); got {K}")
        return f0, control, K

    # ---- one hop ---------------------------------------------------------------------------------------------------------
    def push(self, f0: torch.Tensor, control: torch.Tensor, start=None, stop=None) -> torch.Tensor:
        """f0 (B,1,K) Hz, control (B,C>=2,K) normalised, this hop's events -> (B, 128 K) audio."""
        if self.finished:
            raise RuntimeError("VoiceStream: closed")
        f0, control, K = self._check_shape(f0, control)
        words = self.book.plan(start, stop)        # raises before anything is launched
        self._check_weights()
        f0_2d = f0[:, 0, :]
        self._set_events(words)
        key = (K, control.shape[1])
        if self._use_graph and self._steady(K) and not torch.cuda.is_current_stream_capturing():
            hit = self._captured_hop(key, True)
            if hit is not None:
                g, f0_in, c_in, _, out, pre = hit
                torch._foreach_copy_([f0_in, c_in], [f0_2d, control])
                g.replay()
                self._done(words, K, pre)
                return out.clone()
        L = _lib.lib()
        with torch.cuda.device(self.dev):
            out = torch.empty((self.B, HOP * K), dtype=torch.float32, device=self.dev)
            pre = torch.empty((self.B, HOP * K), dtype=torch.float32, device=self.dev)
            nz = torch.rand(L.nws_stream_noise_draws(K, 0, self.frames_seen), device=self.dev) if self._noise_all is None else None
            self._step(f0_2d.contiguous(), control, nz, out, pre)
        self._done(words, K, pre)
        return out

    def _done(self, words, K, pre):
        self.book.commit(words)
        self._advance(K)
        self.hops += 1
        self._last_pre = pre

    def _advance(self, K):
        self._nz_prev_start = int(_lib.lib().nws_stream_noise_start(int(self.frames_seen == 0), self.frames_seen))
        self.frames_seen += K
        self._last_K = K

    # ---- zero-copy hops ----------------------------------------------------------------------------------------------
    def static_io(self, K: int, channels: int = 2):
        """(f0_in (B, K), control_in (B, channels, K), events (B) int32, out (B, 128 K)) of the captured hop of K frames: the
        buffers `hop()` consumes and fills (`hop` writes `events` from its start / stop arguments).  Needs one push of K frames
        behind it."""
        if self.finished:
            raise RuntimeError("VoiceStream: closed")
        if not self._steady(K):
            raise RuntimeError(f"static_io({K}): push a hop of {K} frames first")
        if not 1 <= K <= _SLOT_MAX_FRAMES:
            raise RuntimeError(f"slot mode serves hops of 1 .. {_SLOT_MAX_FRAMES} frames; got {K}")
        hit = self._graphs.get((K, channels))
        if hit is None:
            hit = self._graphs[(K, channels)] = self._capture(K, channels)
        return hit[1], hit[2], self._ev, hit[4]

    def hop(self, K: int, start=None, stop=None, channels: int = 2) -> torch.Tensor:
        """Replay the captured hop on static_io(K)'s inputs with this hop's events; returns the static output buffer (overwritten
        by the next hop)."""
        if self.finished:
            raise RuntimeError("VoiceStream: closed")
        self._check_weights()
        hit = self._graphs.get((K, channels))
        if hit is None or not self._steady(K):
            raise RuntimeError("hop(): call static_io(K) first (again after a weight update), and do not interleave other hop sizes")
        words = self.book.plan(start, stop)
        self._set_events(words)
        hit[0].replay()
        self._done(words, K, hit[5])
        return hit[4]

    # ---- state ---------------------------------------------------------------------------------------------------------
    def slot_states(self) -> list:
        """'idle' / 'active' / 'releasing' per slot, as of the next hop."""
        return list(self.book.states)

    def idle_slots(self) -> list:
        return [i for i, s in enumerate(self.book.states) if s == IDLE]

    def check(self) -> None:
        """Raise if a hop's device work reported that it gave up waiting (counters[5]; synchronises).  The flag belongs to the
        four-launch hop (K <= 2 frames, at most 512 slots), whose frame-MLP workgroups wait inside the launch for their slot's
        recurrence with a bounded wait; the seven-launch form of every other hop has no such wait and never sets it, and on the
        runtime-size kernels no hop has one: there the call only synchronises."""
        if self._path.gave_up(self):
            raise RuntimeError("VoiceStream: a hop's frame-MLP work gave up waiting for its recurrence rows (its output is NaN)")

    def close(self) -> None:
        """check(), then release the captured hops; push / hop / static_io raise afterwards."""
        self.check()
        self._graphs.clear()
        self.finished = True


class GenericVoiceStream(VoiceStream):
    """VoiceStream for a model that `Engine.specialised()` turns down (what GenericNewtStream is to NewtStream): the same contract
    and methods, one hop = one `g_stream_step_slots` of the binding (`nws_g_stream_step_slots`, csrc/generic.hip).
    The hop is a chain of launches in which nothing waits, so `check()` has no give-up flag to read.  _GenericPath states what it
    needs."""

    _PATH = _GenericPath


def voice_stream(model, batch_size: int, **kw):
    """The slot stream of `model` whatever its architecture (`model.voices`): VoiceStream on the fused kernels when
    `Engine.specialised()`, GenericVoiceStream on the runtime-size kernels otherwise."""
    cls = VoiceStream if model._engine.specialised() else GenericVoiceStream
    return cls(model, batch_size, **kw)


# ---- note player: notes -> frame-rate controls -> slot stream -> one mixed signal -----------------------
NOTE_HELD = _lib.NOTE_HELD


def pan_gains(pan: float, channels: int) -> tuple:
    """Constant-power law: pan in [-1, 1] -> (left, right) = (cos, sin) of (pan + 1) pi / 4.  One channel: gain 1."""
    if not -1.0 <= float(pan) <= 1.0:
        raise RuntimeError(f"pan {pan} outside [-1, 1]")
    if channels == 1:
        return (1.0,)
    a = (float(pan) + 1.0) * math.pi / 4.0
    return (math.cos(a), math.sin(a))


class NoteBook:
    """Host-side scheduling of a NotePlayer (no GPU), beside SlotBook: notes to slots, events to hop boundaries, a voice's frame
    count, and the hop that carries its slot `stop`.

    `note_on` hands the idle slot of lowest index to the note at once (a slot that is `releasing`, or taken by an earlier note-on
    of the same interval, is not idle) and queues the start; `note_off` queues the release.  `plan()` applies the queue at the hop
    boundary - a note-off finds j_off = the frames its voice has had, 0 when the voice has not had a hop yet - and returns the
    hop's (start, stop) slot lists; `commit()` books the hop.  A voice's slot `stop` goes on the hop that contains its frame
    j_off + R - 1: voice hop (j_off + R - 1) // K.  `notes` (pitch, velocity, j_off) and `gains` per slot are what the device
    tables must hold for the planned hop; `notes_dirty` / `gains_dirty` say that they changed since `clean()`."""

    def __init__(self, voices: int, hop_frames: int, release_frames: int, channels: int = 1):
        self.B, self.K, self.R, self.C = int(voices), int(hop_frames), int(release_frames), int(channels)
        if self.B < 1 or not 1 <= self.K <= _SLOT_MAX_FRAMES or self.R < 1 or self.C not in (1, 2):
            raise RuntimeError(f"NoteBook: voices >= 1, 1 <= hop_frames <= {_SLOT_MAX_FRAMES}, release_frames >= 1, channels 1 or 2")
        self.slots = SlotBook(self.B)
        self.frames = [0] * self.B                       # frames the slot's voice has had: the device counter's mirror
        self.notes = [(0.0, 0.0, NOTE_HELD)] * self.B
        self.gains = [(0.0,) * self.C] * self.B
        self.notes_dirty = self.gains_dirty = True
        self.hops = 0
        self.dropped = 0
        self._slot_of = {}                               # live handle -> slot, from note_on until the stop hop is booked
        self._start_hop = [None] * self.B
        self._on, self._off = [], []
        self._next = 0
        self._planned = None

    # ---- between hops --------------------------------------------------------------------------------------------------
    def note_on(self, pitch: float, velocity: float = 0.8, gains=None):
        if not 0.0 < float(velocity) <= 1.0:
            raise RuntimeError(f"velocity {velocity} outside (0, 1]")
        gains = tuple(float(g) for g in (gains if gains is not None else (1.0,) * self.C))
        if len(gains) != self.C:
            raise RuntimeError(f"expected {self.C} gains, got {len(gains)}")
        taken = set(self._slot_of.values())
        for b in range(self.B):
            if self.slots.states[b] == IDLE and b not in taken:
                handle = self._next
                self._next += 1
                self._slot_of[handle] = b
                self._on.append((b, float(pitch), float(velocity), gains))
                return handle
        self.dropped += 1
        return None

    def note_off(self, handle) -> None:
        """Release the note; a handle whose voice has ended (or None) is ignored."""
        if handle in self._slot_of:
            self._off.append(handle)

    def active(self) -> list:
        """handles of the notes that sound or wait for their first hop, released ones included"""
        return sorted(self._slot_of)

    def stop_hop(self, handle):
        """the hop (counted from the book's first) that carries the voice's slot `stop`; None while the note is held"""
        b = self._slot_of.get(handle)
        if b is None or self.notes[b][2] == NOTE_HELD or self._start_hop[b] is None:
            return None
        return self._start_hop[b] + (self.notes[b][2] + self.R - 1) // self.K

    # ---- at the hop boundary -----------------------------------------------------------------------------------------------
    def plan(self):
        if self._planned is not None:
            raise RuntimeError("NoteBook: plan() twice without commit()")
        start = []
        for b, pitch, velocity, gains in self._on:
            self.notes = self.notes[:b] + [(pitch, velocity, NOTE_HELD)] + self.notes[b + 1:]
            if self.gains[b] != gains:
                self.gains = self.gains[:b] + [gains] + self.gains[b + 1:]
                self.gains_dirty = True
            self.notes_dirty = True
            self.frames[b] = 0
            self._start_hop[b] = self.hops
            start.append(b)
        for handle in self._off:
            b = self._slot_of.get(handle)
            if b is not None and self.notes[b][2] == NOTE_HELD:
                self.notes = self.notes[:b] + [(self.notes[b][0], self.notes[b][1], self.frames[b])] + self.notes[b + 1:]
                self.notes_dirty = True
        self._on, self._off = [], []
        stop = [b for b in sorted(self._slot_of.values())
                if self.notes[b][2] != NOTE_HELD and self.frames[b] <= self.notes[b][2] + self.R - 1 < self.frames[b] + self.K]
        words = self.slots.plan(start, stop)
        self._planned = words
        return start, stop

    def commit(self) -> None:
        words, self._planned = self._planned, None
        self.slots.commit(words)
        for b, w in enumerate(words):
            if w & SLOT_ACTIVE:
                self.frames[b] += self.K
            if w & SLOT_STOP:
                self._slot_of = {h: s for h, s in self._slot_of.items() if s != b}
        self.hops += 1

    def clean(self) -> None:
        self.notes_dirty = self.gains_dirty = False


class NotePlayer:
    """A polyphonic instrument on a trained model (`model.player(voices, **kw)`): notes in, one mixed signal out.

    One `hop()` = `hop_frames` control frames (128 samples each) = three pieces on torch's current stream:
      * `note_control` (nws_note_control): every slot's F0 and normalised controls of this hop's frames, from the hop's event words,
        the note table and the per-slot frame counters - closed forms in the voice's frame index, so a note's
        controls do not depend on the hop size;
      * the hop of the `VoiceStream` / `GenericVoiceStream` the player owns (used as it is: its captured hop once it exists, on that hop's own input
        buffers, which the control launch fills in place);
      * `voice_mix` (nws_voice_mix): out[c] = sum over the slots of gain[slot, c] * slot output.
    The three are two launches around the stream's replayed graph, not one graph of their own.  Nothing is read back; the host
    keeps a `NoteBook` and copies the event words, the note table or the gains to the device only when they change.

    Envelope per note: a linear attack of `attack` frames from `silence` to the peak p = peak_lo + velocity (peak_hi - peak_lo), a
    linear decay of `decay` frames by `drop`, the sustain at p - drop, and from `note_off` a linear release of `release` frames to
    `silence`; loudness in the feature's units (dB + 80) / 80.  Vibrato: `vib_depth` cents at `vib_rate` Hz, faded in over
    `vib_ramp` frames after `vib_delay`.  `peak_hi`, `peak_lo` and `silence` default to min(1, mean1 + 2 std1), mean1 - std1 and
    max(0, mean1 - 4 std1) of the checkpoint's loudness statistics: these defaults, like those of the envelope times and the
    vibrato, come from the statistics' meaning alone - nobody has listened to them.

    `note_on` returns a handle, or None (and counts `dropped`) when no slot is idle: no voice is stolen.  A slot's gains are its
    latest note's, so the reverb tail of an earlier voice of the slot follows a new note's pan.  Events take effect at the next
    hop boundary.  `normalisation=(mean, std)` is the checkpoint's (checkpoint.load_normalisation); `phase_u`, `noise` and `graph`
    go to the stream.  Any architecture: the stream is `voice_stream(model, voices)` - VoiceStream on the packaged one,
    GenericVoiceStream otherwise; the model's control input must have 2 channels (F0 and loudness)."""

    def __init__(self, model, voices: int, hop_frames: int = 1, channels: int = 1, *, attack: int = 3, decay: int = 12,
                 release: int = 25, drop: float = 0.075, silence: float | None = None, peak_lo: float | None = None,
                 peak_hi: float | None = None, vib_rate: float = 5.5, vib_depth: float = 15.0, vib_delay: int = 38,
                 vib_ramp: int = 25, normalisation=None, phase_u: torch.Tensor | None = None, noise: torch.Tensor | None = None,
                 graph: bool = True):
        if normalisation is None:
            raise RuntimeError("NotePlayer: pass normalisation=(mean, std), the checkpoint's data_mean / data_std "
                               "(checkpoint.load_normalisation)")
        mean, std = ([float(v) for v in list(x)[:2]] for x in normalisation)
        n_control = int(model.embedding.gru.input_size)
        if n_control != 2:
            raise RuntimeError(f"NotePlayer: ControlModule.control_size = {n_control}: note_control writes two control channels, F0 and "
                               f"loudness, so the model's control input must have 2")
        self.book = NoteBook(voices, hop_frames, release, channels)          # validates voices, hop_frames, release, channels
        self.B, self.K, self.C = self.book.B, self.book.K, self.book.C
        hi = min(1.0, mean[1] + 2.0 * std[1]) if peak_hi is None else float(peak_hi)
        lo = mean[1] - std[1] if peak_lo is None else float(peak_lo)
        q = max(0.0, mean[1] - 4.0 * std[1]) if silence is None else float(silence)
        self.params = dict(zip(_lib.NOTE_PARAMS, (int(attack), int(decay), int(release), int(vib_delay), int(vib_ramp), float(drop), q,
                                                  lo, hi, float(vib_rate), float(vib_depth), float(model.sample_rate), mean[0], std[0],
                                                  mean[1], std[1])))
        p = self.params
        if (p["attack"] < 0 or p["decay"] < 0 or p["vib_delay"] < 0 or p["vib_ramp"] < 1 or p["drop"] < 0 or p["vib_rate"] < 0
                or not p["std0"] > 0 or not p["std1"] > 0 or max(p["attack"], p["decay"], p["release"], p["vib_delay"], p["vib_ramp"]) > 2 ** 24):
            raise RuntimeError("NotePlayer: attack, decay, vib_delay >= 0, release, vib_ramp >= 1 (all at most 2^24 frames), drop >= 0, "
                               "vib_rate >= 0 and positive standard deviations")
        self.stream = voice_stream(model, self.B, phase_u=phase_u, noise=noise, graph=graph)
        self.dev = dev = self.stream.dev
        self._params = torch.tensor([float(p[k]) for k in _lib.NOTE_PARAMS], dtype=torch.float64)
        nbytes = _lib.lib().nws_note_control_state_bytes(self.B)
        if nbytes == 0:
            raise RuntimeError(f"NotePlayer: {self.B} voices: 1 <= voices <= 65535")
        with torch.cuda.device(dev):
            self._state = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            binding().note_control_reset(self._state, self.B)
            self._notes = torch.zeros((self.B, 4), dtype=torch.int32, device=dev)
            self._gain = torch.zeros((self.B, self.C), dtype=torch.float32, device=dev)
            self._f0 = torch.zeros((self.B, self.K), dtype=torch.float32, device=dev)         # a hop before the captured one exists
            self._control = torch.zeros((self.B, 2, self.K), dtype=torch.float32, device=dev)
            self._out = torch.zeros((self.C, HOP * self.K), dtype=torch.float32, device=dev)
        self.finished = False
        self.last_hop = None

    # ---- notes --------------------------------------------------------------------------------------------------------------
    @property
    def dropped(self) -> int:
        return self.book.dropped

    def note_on(self, pitch: float, velocity: float = 0.8, pan: float = 0.0):
        """Start a note at the next hop: MIDI note number, velocity in (0, 1], pan in [-1, 1] (left .. right; two channels only).
        -> a handle for `note_off`, or None when every slot is taken (counted in `dropped`)."""
        return self.book.note_on(pitch, velocity, pan_gains(pan, self.C))

    def note_off(self, handle) -> None:
        """Release the note from the next hop on; its slot is free again two hops after the release has ended."""
        self.book.note_off(handle)

    def active(self) -> list:
        """handles of the notes that still sound (released ones until their release has ended)"""
        return self.book.active()

    # ---- one hop --------------------------------------------------------------------------------------------------------------
    def _upload(self):
        book = self.book
        if book.notes_dirty:
            table = np.zeros((self.B, 4), dtype=np.int32)
            table[:, 0] = np.array([n[0] for n in book.notes], dtype=np.float32).view(np.int32)
            table[:, 1] = np.array([n[1] for n in book.notes], dtype=np.float32).view(np.int32)
            table[:, 2] = [n[2] for n in book.notes]
            self._notes.copy_(torch.from_numpy(table).pin_memory(), non_blocking=True)
        if book.gains_dirty:
            self._gain.copy_(torch.tensor(book.gains, dtype=torch.float32).pin_memory(), non_blocking=True)
        book.clean()

    def hop(self) -> torch.Tensor:
        """One hop -> (channels, 128 hop_frames): the player's own output buffer, overwritten by the next hop."""
        if self.finished:
            raise RuntimeError("NotePlayer: closed")
        vs, K = self.stream, self.K
        start, stop = self.book.plan()
        vs._check_weights()
        vs._set_events(vs.book.plan(start, stop))          # the control launch reads the words the stream's hop will read
        self._upload()
        ops = binding()
        if vs._use_graph and vs._steady(K) and not torch.cuda.is_current_stream_capturing():
            f0_in, control_in, ev, _ = vs.static_io(K)
            ops.note_control(self._params, ev, self._notes, self._state, f0_in, control_in)
            o = vs.hop(K, start=start, stop=stop)
        else:
            f0_in, control_in = self._f0, self._control
            ops.note_control(self._params, vs._ev, self._notes, self._state, f0_in, control_in)
            o = vs.push(f0_in.unsqueeze(1), control_in, start=start, stop=stop)
        ops.voice_mix(o, self._gain, self._out)
        self.book.commit()
        self.last_hop = (f0_in, control_in, start, stop, o)    # what the hop fed the stream and got from it: for tests and debugging
        return self._out

    def render(self, n_hops: int) -> torch.Tensor:
        """n_hops hops -> (channels, 128 hop_frames n_hops)"""
        with torch.cuda.device(self.dev):
            out = torch.empty((self.C, HOP * self.K * int(n_hops)), dtype=torch.float32, device=self.dev)
        for h in range(int(n_hops)):
            out[:, h * HOP * self.K:(h + 1) * HOP * self.K].copy_(self.hop())
        return out

    # ---- state ----------------------------------------------------------------------------------------------------------------
    def check(self) -> None:
        """VoiceStream.check(), and the device's frame counters against the host's mirror for every sounding slot (synchronises)."""
        self.stream.check()
        cnt = self._state[:4 * self.B].cpu().view(torch.int32).tolist()
        for b, s in enumerate(self.book.slots.states):
            if s == ACTIVE and cnt[b] != self.book.frames[b]:
                raise RuntimeError(f"NotePlayer: slot {b}: device frame counter {cnt[b]}, host mirror {self.book.frames[b]}")
        if self.book.slots.states != self.stream.book.states:
            raise RuntimeError("NotePlayer: the note book and the stream's slot book disagree")

    def close(self) -> None:
        """check(), then close the stream; hop raises afterwards."""
        self.check()
        self.stream.close()
        self.finished = True


# ---- streaming sample-rate converter: a stream at one rate feeds, or is fed by, a device at another ----------------------
class StreamResampler:
    """Band-limited sample-rate conversion of a stream, chunk by chunk (`binding().resample_stream_step` ->
    `nws_resample_stream_step`, csrc/resample_stream.hip): the concatenation of everything `push` and `flush`
    return is `resample_audio` of the concatenated input - to the converter's accuracy, and bit for bit the same whatever the
    chunk sizes.  The stream runs `latency_samples` (= right, 4 ms) input samples behind its input; the chunk marked `final`
    (or `flush()`) releases the remainder against a zero extension, like the offline converter's right edge.

    The two counters of every row (samples consumed, outputs emitted) live in the device state blob, so a step's launch has no
    changing argument: `static_io(n)` captures the step of n samples ONCE into a hipGraph and `hop()` replays it.  How many of a
    step's output columns are new (705 or 706 per 256 samples at 16 -> 44.1 kHz) comes from the host's own mirror of the
    counters, plain Python ints, never from a read-back; `check()` compares mirror and device on demand."""

    def __init__(self, sr_in, sr_out, batch_size: int, device=None, max_chunk: int = 4096, graph: bool = True):
        from .data.utils.preprocess_audio import _bank, _rate

        self.sr_in, self.sr_out = _rate(sr_in, "sr_in"), _rate(sr_out, "sr_out")
        self.B = int(batch_size)
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise _lib.NwsError(f"StreamResampler on {dev}: the converter only runs as a HIP kernel on an AMD GPU; there is no CPU fallback.")
        self.dev = torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)
        L = _lib.lib()
        in_range = max(self.sr_in, self.sr_out) < 2 ** 31 and 1 <= self.B <= 65535
        nbytes = L.nws_resample_stream_state_bytes(self.B, self.sr_in, self.sr_out) if in_range else 0
        if nbytes == 0:
            raise RuntimeError(f"StreamResampler: unsupported stream (B {self.B}, {self.sr_in} -> {self.sr_out} Hz): 1 <= B <= 65535, "
                               "rates the offline converter serves, and a filter whose history and look-ahead leave room for a chunk "
                               "in 64 KB of LDS")
        dims = (C.c_int32 * 6)()
        _lib.check(L.nws_resample_dims(self.sr_in, self.sr_out, dims), "nws_resample_dims")
        self.taps, self._right = int(dims[2]), int(dims[4])
        self.max_chunk = int(min(max(1, int(max_chunk)), L.nws_resample_stream_max_chunk(self.sr_in, self.sr_out)))
        self._bank = _bank(self.sr_in, self.sr_out, self.dev)
        with torch.cuda.device(self.dev):
            self._state = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        self._use_graph = bool(graph)
        self._graphs = {}          # n -> (graph or None, x_in, out)
        self._static_n = None
        self.reset()

    # ---- the host's mirror of the device counters ---------------------------------------------------------------------
    @property
    def latency_samples(self) -> int:
        return self._right

    @property
    def samples_in(self) -> int:
        return self._n_seen

    @property
    def samples_out(self) -> int:
        return self._t_next

    def _emits(self, n: int, final: bool) -> int:
        """columns a step of n samples adds: E(n_seen + n) - t_next, with `final` up to the offline length"""
        return int(_lib.lib().nws_resample_stream_emitted(self._n_seen + n, self.sr_in, self.sr_out, int(final))) - self._t_next

    def _advance(self, n: int, m: int, final: bool):
        self._n_seen += n
        self._t_next += m
        self.finished = bool(final)

    def reset(self):
        """Back to the initial state: nothing consumed, nothing emitted, a history of zeros (the captured steps stay valid)."""
        binding().resample_stream_reset(self._state, self.B, self.sr_in, self.sr_out)
        self._n_seen = 0
        self._t_next = 0
        self.finished = False

    # ---- one chunk ----------------------------------------------------------------------------------------------------
    def _step(self, x, final, out):
        binding().resample_stream_step(self._state, self._bank, self.sr_in, self.sr_out, x, bool(final), out)

    def push(self, x: torch.Tensor, final: bool = False) -> torch.Tensor:
        """x (B, n) float32 at sr_in -> (B, m) at sr_out: the outputs whose last tap this chunk delivered (m may be 0).  `final`
        ends the stream (n may be 0 then): the remaining outputs up to (samples_in L) // M, against zeros beyond the end."""
        if self.finished:
            raise RuntimeError("stream already finished")
        if isinstance(x, torch.Tensor) and x.is_cuda and not x.is_contiguous():
            x = x.contiguous()
        if not isinstance(x, torch.Tensor) or x.dim() != 2:
            raise RuntimeError(f"expected a ({self.B}, n) chunk, got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
        n = int(x.shape[1])
        if n < 1 and not final:
            raise RuntimeError("empty chunk")
        if n > self.max_chunk:                           # long chunks: process in pieces (state makes that exact)
            outs = []
            for k0 in range(0, n, self.max_chunk):
                k1 = min(n, k0 + self.max_chunk)
                outs.append(self.push(x[:, k0:k1], final and k1 == n))
            return torch.cat(outs, dim=1)
        m = self._emits(n, final)
        width = int(_lib.lib().nws_resample_stream_max_out(n, self.sr_in, self.sr_out, int(final)))
        with torch.cuda.device(self.dev):
            out = torch.empty((self.B, width), dtype=torch.float32, device=self.dev)
        self._step(x, final, out)                        # the binding checks device, dtype and sizes, and raises before a launch
        self._advance(n, m, final)
        return out[:, :m]

    def flush(self) -> torch.Tensor:
        """The stream's remaining outputs: `push` of an empty chunk with final=True."""
        with torch.cuda.device(self.dev):
            return self.push(torch.empty((self.B, 0), dtype=torch.float32, device=self.dev), final=True)

    # ---- zero-copy hops: the caller writes into the captured step's own input buffer and reads its output buffer -----------
    def static_io(self, n: int):
        """(x_in (B, n), out (B, max_out)) of the captured step of n samples - the buffers `hop()` consumes and fills.  One
        kernel, no parallel branches, no changing argument: captured once, valid for the life of the stream (across reset())."""
        n = int(n)
        if self.finished:
            raise RuntimeError("stream already finished")
        if not 1 <= n <= self.max_chunk:
            raise RuntimeError(f"static_io({n}): a captured step takes 1 .. {self.max_chunk} samples")
        hit = self._graphs.get(n)
        if hit is None:
            width = int(_lib.lib().nws_resample_stream_max_out(n, self.sr_in, self.sr_out, 0))
            with torch.cuda.device(self.dev):
                x_in = torch.zeros((self.B, n), dtype=torch.float32, device=self.dev)
                out = torch.zeros((self.B, width), dtype=torch.float32, device=self.dev)
                g = None
                if self._use_graph:
                    g = torch.cuda.CUDAGraph()
                    torch.cuda.synchronize(self.dev)
                    with torch.cuda.graph(g):
                        self._step(x_in, False, out)     # capture records, it does not run: the state has not advanced
            hit = self._graphs[n] = (g, x_in, out)
        self._static_n = n
        return hit[1], hit[2]

    def hop(self) -> torch.Tensor:
        """Run the captured step on whatever the caller left in static_io(n)'s input buffer; returns the new columns
        out[:, :m] of the static output buffer (overwritten by the next hop)."""
        hit = self._graphs.get(self._static_n)
        if hit is None:
            raise RuntimeError("hop(): call static_io(n) first")
        if self.finished:
            raise RuntimeError("stream already finished")
        n = self._static_n
        m = self._emits(n, False)
        if hit[0] is not None:
            hit[0].replay()
        else:
            self._step(hit[1], False, hit[2])
        self._advance(n, m, False)
        return hit[2][:, :m]

    def check(self) -> None:
        """Read the device counters back once (synchronises) and compare them with the host's mirror; for tests and debugging."""
        cnt = self._state[:16 * self.B].cpu().view(torch.int64).reshape(self.B, 2)
        want = torch.tensor([self._n_seen, self._t_next], dtype=torch.int64).expand(self.B, 2)
        if not torch.equal(cnt, want):
            raise RuntimeError(f"StreamResampler: device counters {cnt.tolist()} differ from the host's mirror "
                               f"(n_seen {self._n_seen}, t_next {self._t_next})")


# ---- analysis streams: frame-rate features from chunked audio with a bounded delay -----------------------------------------
class _FrameStream:
    """What `StreamF0` and `StreamLoudness` share: frames of 2 W samples every hop_length, frame e released once frame e + lag
    exists (DESIGN.md 3.24 has the arithmetic), the counters in the device state blob with a mirror of plain ints on the host
    that is handed to every step, so nothing is read back; `check()` compares mirror and device on demand.
    A subclass sets B, dev, frame_length, hop_length, lag, max_chunk, _state and _half (its name for 2 W in messages), and has
    `reset()`, `_emitted_after`, `_frames_after` and `_step(x, final, m) -> its output tensors, (B, >= m) each`."""

    def _device(self, device):
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise _lib.NwsError(f"{type(self).__name__} on {dev}: the extractor only runs as HIP kernels on an AMD GPU; there is no CPU fallback.")
        return torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)

    @property
    def latency_samples(self) -> int:
        return self.frame_length // 2 + self.lag * self.hop_length

    @property
    def samples_in(self) -> int:
        return self._n_seen

    @property
    def frames_out(self) -> int:
        return self._emitted

    def _rows_bytes(self) -> int:
        """bytes of the B rows of the state blob (all of it, unless a subclass keeps more behind them)"""
        return self._state.numel()

    def _restart(self):
        self._n_seen = 0
        self._emitted = 0
        self.finished = False

    def push(self, x: torch.Tensor, final: bool = False):
        """x (B, n) or (n,) float32 CUDA -> the subclass's outputs, (B, m) each: the m >= 0 frames this chunk released.
        `final` ends the stream (n may be 0 then): the remaining frames up to 1 + samples_in // hop_length."""
        if self.finished:
            raise RuntimeError("stream already finished")
        if isinstance(x, torch.Tensor) and x.dim() == 1 and self.B == 1:
            x = x.unsqueeze(0)
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[0] != self.B:
            raise RuntimeError(f"expected a ({self.B}, n) chunk, got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
        if not x.is_cuda:
            raise _lib.NwsError(f"chunk lives on {x.device}: the extractor only runs as HIP kernels on an AMD GPU; there is no CPU fallback.")
        if not x.is_contiguous():
            x = x.contiguous()
        n = int(x.shape[1])
        if n < 1 and not final:
            raise RuntimeError("empty chunk")
        if n > self.max_chunk:                           # long chunks: process in pieces (state makes that exact)
            outs = []
            for k0 in range(0, n, self.max_chunk):
                k1 = min(n, k0 + self.max_chunk)
                outs.append(self.push(x[:, k0:k1], final and k1 == n))
            return tuple(torch.cat(o, dim=1) for o in zip(*outs))
        if final and self._n_seen + n <= self.frame_length // 2:
            raise RuntimeError(f"a stream of {self._n_seen + n} samples cannot end: the reflect padding needs more than "
                               f"{self._half} / 2 = {self.frame_length // 2}")
        after = self._emitted_after(self._n_seen + n, final)
        if after < 0:
            raise RuntimeError(f"{type(self).__name__}: the stream is limited to 2^21 hops; reset() it")
        m = after - self._emitted
        with torch.cuda.device(self.dev):
            outs = self._step(x, bool(final), m)
        self._n_seen += n
        self._emitted = after
        self.finished = bool(final)
        return tuple(o[:, :m] for o in outs)

    def flush(self):
        """The stream's remaining frames: `push` of an empty chunk with final=True."""
        with torch.cuda.device(self.dev):
            return self.push(torch.empty((self.B, 0), dtype=torch.float32, device=self.dev), final=True)

    def check(self) -> None:
        """Read the device counters back once (synchronises) and compare them with the host's mirror; for tests and debugging."""
        row = self._rows_bytes() // self.B
        cnt = self._state[:self.B * row].view(self.B, row)[:, :32].cpu().contiguous().view(torch.int64)
        frames = -1 if self._n_seen <= self.frame_length // 2 and self.finished else self._frames_after(self._n_seen, self.finished)
        want = torch.tensor([self._n_seen, frames, self._emitted, int(self.finished)], dtype=torch.int64).expand(self.B, 4)
        if not torch.equal(cnt, want):
            raise RuntimeError(f"{type(self).__name__}: device counters {cnt.tolist()} differ from the host's mirror {want[0].tolist()}")


class StreamF0(_FrameStream):
    """pYIN F0 of a stream, chunk by chunk (`binding().pyin_stream_step` -> `nws_pyin_stream_step`, csrc/pyin_stream.hip;
    DESIGN.md 3.24), with the offline extractor's names and defaults.  The stream runs the offline forward pass as the samples
    arrive and emits frame e once frame e + lag exists, as the state at e of the best path that ends in frame e + lag;
    `final` (or `flush()`) computes the last frames against the reflected right edge and releases the rest.  With a lag of
    at least the clip's frame count the result is `pyin_frames` of the whole clip, bit for bit; at lag 4 it agreed with it
    on every frame of the project's test signals (DESIGN.md 3.24 has the table).  The output runs `latency_samples` =
    frame_length / 2 + lag hop_length samples behind the input.

    The counters live in the device state blob; the host keeps a mirror (plain ints) and hands its sample count to every
    step, so nothing is read back; `check()` compares mirror and device on demand."""

    def __init__(self, batch_size: int, sample_rate: float = 16000, minimum_frequency: float = 65.0,
                 maximum_frequency: float = 2093.0, frame_length: int = 1024, hop_length: int = 128, lag: int = 8,
                 fill_unvoiced=None, device=None):
        from .data.utils.f0_extraction import _config, _table

        self.B = int(batch_size)
        self.cfg = _config(sample_rate, minimum_frequency, maximum_frequency, frame_length, hop_length)
        self.frame_length, self.hop_length, self.lag = self.cfg[3], self.cfg[4], int(lag)
        self.fill_unvoiced = None if fill_unvoiced is None else float(fill_unvoiced)
        self.dev = self._device(device)
        if not 0 <= self.lag <= 255:
            raise RuntimeError(f"StreamF0: lag {self.lag} outside 0 .. 255")
        L = _lib.lib()
        nbytes = L.nws_pyin_stream_state_bytes(self.B, *self.cfg) if 1 <= self.B <= 65535 else 0
        if nbytes == 0:
            raise RuntimeError(f"StreamF0: unsupported stream (B {self.B}, configuration {self.cfg}): 1 <= B <= 65535, a "
                               "configuration the offline extractor serves, and at most 256 hops in half a frame")
        self.max_chunk = int(L.nws_pyin_stream_max_chunk(*self.cfg))
        self._table = _table(self.cfg, self.dev)
        with torch.cuda.device(self.dev):
            self._state = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        self.reset()

    _half = "frame_length"

    def _emitted_after(self, n_seen: int, final: bool) -> int:
        return int(_lib.lib().nws_pyin_stream_emitted(n_seen, *self.cfg, self.lag, int(final)))

    def _frames_after(self, n_seen: int, final: bool) -> int:
        return int(_lib.lib().nws_pyin_stream_frames(n_seen, *self.cfg, int(final)))

    def reset(self):
        """Back to the initial state: nothing consumed, nothing emitted."""
        binding().pyin_stream_reset(self._state, self.B, *self.cfg)
        self._restart()

    def _step(self, x, final, m):
        """-> (f0 fp32, voiced_prob fp64, states int32)"""
        f0 = torch.empty((self.B, max(m, 1)), dtype=torch.float32, device=self.dev)
        voiced_prob = torch.empty((self.B, max(m, 1)), dtype=torch.float64, device=self.dev)
        states = torch.empty((self.B, max(m, 1)), dtype=torch.int32, device=self.dev)
        binding().pyin_stream_step(self._state, self._table, *self.cfg, self.lag, x, self._n_seen, final,
                                   self.fill_unvoiced is not None, self.fill_unvoiced if self.fill_unvoiced is not None else 0.0,
                                   f0, voiced_prob, states)
        return f0, voiced_prob, states


# ---- loudness stream: the loudness feature with a causal reference level ----------------------------------------------------
class StreamLoudness(_FrameStream):
    """Perceptual loudness of a stream, chunk by chunk (`binding().loudness_stream_step` -> `nws_loudness_stream_step`,
    csrc/loudness_stream.hip), with the offline extractor's names and the pipeline's defaults
    (gin/data/urmp_4second_pyin.gin), which pair it with a `StreamF0`: both emit the same number of frames on every push.

    The offline feature is measured against the loudest bin of the WHOLE clip, which a stream does not know.  Here frame e
    leaves once frame e + lag exists and is measured against a reference power that depends on e, the lag and the signal alone,
    never on the chunking:
      * reference="running": the largest power heard up to frame e + lag (at the flush: up to the last frame).  Quiet starts
        are rendered too loud until the signal's peak has been heard; from then on the frames are the offline ones, bit for bit.
        Without a release the maximum does not decay: one click pins the reference until `reset()`.
      * release_db_per_s (with "running"): the tracked level falls by this many dB per second, never below
        floor_power, so the reference recovers after a click; frame e is then measured against the largest level between
        frames e and e + lag.  `sample_rate` turns the rate into the factor per hop.  0 (the default): no release, the stream above.
      * reference=a float or a (B,) tensor of powers: fixed, a calibration - `loudness_extraction.peak_power` of a sound check,
        for example.  With the clip's own peak power the stream is `loudness_frames` of the clip, bit for bit.  A signal louder
        than its reference gives values above 1 (above 0 dB without `normalise`); they are not clipped.
      * floor_power (with "running"): the running maximum starts at this power instead of 0, so that the room noise in front of
        the first note is not rendered at 0 dB.
    `push` returns (loudness (B, m) fp32, reference_power (B, m) fp32): the frames released and the reference each was measured
    against.  `final` (or `flush()`) computes the last frames against the reflected right edge and releases the rest.  The
    output runs `latency_samples` = n_fft / 2 + lag hop_length samples behind the input."""

    _half = "n_fft"

    def __init__(self, batch_size: int, n_fft: int = 1024, hop_length: int = 128, lag: int = 8, reference="running",
                 floor_power=None, epsilon: float = 1e-5, normalise: bool = True, device=None, release_db_per_s: float = 0.0,
                 sample_rate: float = 16000):
        from .data.utils.loudness_extraction import _dft_operand, release_factor

        self.B = int(batch_size)
        self.n_fft = self.frame_length = int(n_fft)
        self.hop_length, self.lag = int(hop_length), int(lag)
        self.epsilon, self.normalise = float(epsilon), bool(normalise)
        self.dev = self._device(device)
        if not 0 <= self.lag <= 255:
            raise RuntimeError(f"StreamLoudness: lag {self.lag} outside 0 .. 255")
        if not self.epsilon > 0.0:
            raise RuntimeError(f"StreamLoudness: epsilon {self.epsilon} must be positive")
        L = _lib.lib()
        nbytes = L.nws_loudness_stream_state_bytes(self.B, self.n_fft, self.hop_length) if 1 <= self.B <= 65535 else 0
        if nbytes == 0:
            raise RuntimeError(f"StreamLoudness: unsupported stream (B {self.B}, n_fft {self.n_fft}, hop_length {self.hop_length}): "
                               "1 <= B <= 65535, sizes the offline extractor serves (n_fft a power of two in [64, 2048], "
                               "1 <= hop_length <= n_fft, 31 hop_length + n_fft samples within 160 KB of LDS), and at most 256 hops "
                               "in half a frame")
        self.max_chunk = int(L.nws_loudness_stream_max_chunk(self.n_fft, self.hop_length))
        self.track = isinstance(reference, str)
        self.release_db_per_s = float(release_db_per_s)
        self.release_factor = release_factor(release_db_per_s, self.hop_length, sample_rate)
        if self.release_factor < 1.0:
            if not self.track:
                raise RuntimeError("StreamLoudness: release_db_per_s belongs to reference='running'; a fixed reference does not move")
            nbytes = L.nws_loudness_stream_release_state_bytes(self.B, self.n_fft, self.hop_length)      # the rows, then the floors
        if self.track:
            if reference != "running":
                raise RuntimeError(f"StreamLoudness: reference {reference!r}: expected 'running', a power or a (B,) tensor of powers")
            self._initial = self._powers(0.0 if floor_power is None else floor_power, "floor_power")
        else:
            if floor_power is not None:
                raise RuntimeError("StreamLoudness: floor_power belongs to reference='running'; a fixed reference has no floor")
            self._initial = self._powers(reference, "reference")
        self._dft = _dft_operand(self.n_fft, self.dev)
        with torch.cuda.device(self.dev):
            self._state = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        self.reset()

    def _powers(self, value, name) -> torch.Tensor:
        """a power or a (B,) tensor of powers -> (B,) fp32 on the stream's GPU; checked once, here (this reads a tensor back)"""
        if isinstance(value, torch.Tensor):
            p = value.detach().to(device=self.dev, dtype=torch.float32).reshape(-1).contiguous()
            if p.numel() != self.B:
                raise RuntimeError(f"StreamLoudness: {name}: expected ({self.B},) powers, got {tuple(value.shape)}")
        else:
            p = torch.full((self.B,), float(value), dtype=torch.float32, device=self.dev)
        if not bool((torch.isfinite(p) & (p >= 0)).all()):
            raise RuntimeError(f"StreamLoudness: {name}: powers must be finite and >= 0")
        return p

    def _rows_bytes(self) -> int:
        return int(_lib.lib().nws_loudness_stream_state_bytes(self.B, self.n_fft, self.hop_length))      # a release keeps floors behind

    def _emitted_after(self, n_seen: int, final: bool) -> int:
        return int(_lib.lib().nws_loudness_stream_emitted(n_seen, self.n_fft, self.hop_length, self.lag, int(final)))

    def _frames_after(self, n_seen: int, final: bool) -> int:
        return int(_lib.lib().nws_loudness_stream_frames(n_seen, self.n_fft, self.hop_length, int(final)))

    def reset(self):
        """Back to the initial state: nothing consumed, nothing emitted, the reference level at its initial power."""
        if self.release_factor < 1.0:
            binding().loudness_stream_reset_release(self._state, self.B, self.n_fft, self.hop_length, self._initial)
        else:
            binding().loudness_stream_reset(self._state, self.B, self.n_fft, self.hop_length, self._initial, self.track)
        self._restart()

    def _step(self, x, final, m):
        """-> (loudness fp32, reference_power fp32)"""
        loudness = torch.empty((self.B, max(m, 1)), dtype=torch.float32, device=self.dev)
        reference_power = torch.empty((self.B, max(m, 1)), dtype=torch.float32, device=self.dev)
        if self.release_factor < 1.0:
            binding().loudness_stream_step_release(self._state, self._dft, self.n_fft, self.hop_length, self.lag, self.release_factor,
                                                   True, x, self._n_seen, final, self.epsilon, 80.0, self.normalise, loudness,
                                                   reference_power)
        else:
            binding().loudness_stream_step(self._state, self._dft, self.n_fft, self.hop_length, self.lag, x, self._n_seen, final,
                                           self.epsilon, 80.0, self.normalise, loudness, reference_power)
        return loudness, reference_power


class StreamControl:
    """Chunked audio -> the model's two inputs: one `StreamF0` and one `StreamLoudness` on the model's sample rate and control
    hop (frames of 1024 samples, the same lag), and `checkpoint.make_control` on what they release - in float64 on the device,
    cast to fp32 at the end, so the values are the bits of `make_control` on the two streams' frames.  `reference`,
    `floor_power` and `release_db_per_s` (at the model's sample rate) are `StreamLoudness`'s, `fill_unvoiced` is `StreamF0`'s; `mean` / `std` are the dataset statistics of the
    checkpoint ((f0, loudness) each; None: the features as they are); `octave_shift` transposes F0 by whole octaves.
    `push(x, final=False)` -> (f0 (B, 1, m) Hz, control (B, 2, m)), ready for `model.stream(B).push` whenever m > 0."""

    def __init__(self, model, batch_size: int, lag: int = 8, reference="running", floor_power=None, mean=None, std=None,
                 octave_shift: int = 0, fill_unvoiced=None, release_db_per_s: float = 0.0):
        dev = next(model.parameters()).device
        sr, hop = float(model.sample_rate), int(model.control_hop)
        self.f0 = StreamF0(batch_size, sample_rate=sr, frame_length=1024, hop_length=hop, lag=lag, fill_unvoiced=fill_unvoiced,
                           device=dev)
        self.loudness = StreamLoudness(batch_size, n_fft=1024, hop_length=hop, lag=lag, reference=reference,
                                       floor_power=floor_power, device=dev, release_db_per_s=release_db_per_s, sample_rate=sr)
        self.mean = (0.0, 0.0) if mean is None else (float(mean[0]), float(mean[1]))
        self.std = (1.0, 1.0) if std is None else (float(std[0]), float(std[1]))
        self.scale = 2.0 ** int(octave_shift)

    @property
    def latency_samples(self) -> int:
        return self.f0.latency_samples

    @property
    def finished(self) -> bool:
        return self.f0.finished

    def push(self, x: torch.Tensor, final: bool = False):
        f0 = self.f0.push(x, final)[0]
        loudness = self.loudness.push(x, final)[0]
        if f0.shape != loudness.shape:
            raise RuntimeError(f"StreamControl: the two streams released {f0.shape[1]} and {loudness.shape[1]} frames")
        f0 = f0.double() * self.scale
        control = torch.stack([(f0 - self.mean[0]) / self.std[0], (loudness.double() - self.mean[1]) / self.std[1]], dim=-2)
        return f0.float().unsqueeze(-2), control.float()

    def flush(self):
        """The remaining frames of both streams."""
        with torch.cuda.device(self.f0.dev):
            return self.push(torch.empty((self.f0.B, 0), dtype=torch.float32, device=self.f0.dev), final=True)

    def reset(self):
        self.f0.reset()
        self.loudness.reset()

    def check(self) -> None:
        self.f0.check()
        self.loudness.check()
