"""The ctypes binding with the op layer's surface: `CtypesOps` has one method per operator of the TORCH_LIBRARY(newt_hip)
block of csrc/torch_ops.cpp - same name, same positional parameters, same return arity - and each method is the call of
the `extern "C"` launcher(s) of libnws_hip.so that the op of that name makes (tests/test_cpu_cops_surface.py holds the two
surfaces together).  `engine.binding()` hands out either this object or `torch.ops.newt_hip`, so a call site is written once.

Like the ops, every method takes contiguous fp32 CUDA tensors, allocates its outputs on the tensors' device, enqueues on
torch's current stream of that device and raises (`_lib.check`) when the launcher reports an error.  `wdesc` / `gdesc` /
`sdesc` arrive as the CPU uint8 tensor of the struct, `plan` as the CPU int32 tensor of `NwsReverbPlan.as_tensor()`, event
handles as ints.  This module is the only place in the package that marshals a launcher call through ctypes.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import NwsForwardAux, NwsGenericModel, NwsReverbPlan, NwsShaperDesc, NwsWeights, check, ptr

HOP = _lib.HOP


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _struct(desc: torch.Tensor, cls):
    """the CPU uint8 tensor of a struct (engine.py / generic.desc_bytes) back as the ctypes struct"""
    return cls.from_buffer_copy(desc.numpy())


def _plan(plan: torch.Tensor | None):
    return NwsReverbPlan(*plan.tolist()[:6]) if plan is not None else None


def _ref(struct):
    return C.byref(struct) if struct is not None else None


def _aux(fir_design, plan, tables, spectrum) -> NwsForwardAux:
    aux = NwsForwardAux()
    aux.fir_design = ptr(fir_design)
    aux.plan = C.pointer(_plan(plan))
    aux.reverb_tables = ptr(tables)
    aux.reverb_spectrum = ptr(spectrum)
    return aux


def _new(like: torch.Tensor, *shape, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device=like.device)


def _ptrs(tensors):
    return (C.c_void_p * max(1, len(tensors)))(*[t.data_ptr() for t in tensors])


def _pyin_dims(cfg, table=None):
    """nws_pyin_dims of a configuration + the table's length in doubles; `table`: a device table to check against it"""
    dims = (C.c_int32 * 8)()
    L = _lib.lib()
    if L.nws_pyin_dims(*cfg, dims) != 0:
        raise RuntimeError(f"pyin: unsupported configuration (sample_rate, fmin, fmax, frame_length, hop) = {cfg}: at most 512 "
                           "lags (frame_length <= 1024), 1024 pitch bins and a transition window of 127; hop <= frame_length")
    n = L.nws_pyin_table_bytes(*cfg) // 8
    if isinstance(table, torch.Tensor) and (not table.is_cuda or table.dtype != torch.float64 or table.numel() != n):
        raise RuntimeError("pyin: table does not belong to this configuration (expected a float64 CUDA tensor of nws_pyin_table)")
    return (*dims, n)


def _resample_dims(sr_in, sr_out):
    """nws_resample_dims of a pair of rates: (L, M, taps, left, right, step)"""
    dims = (C.c_int32 * 6)()
    if not (1 <= sr_in < 2 ** 31 and 1 <= sr_out < 2 ** 31) or _lib.lib().nws_resample_dims(sr_in, sr_out, dims) != 0:
        raise RuntimeError(f"resample: unsupported rates {sr_in} -> {sr_out}: integers >= 1 whose weight bank (sr_out / gcd rows) "
                           "stays below 64 MB")
    return tuple(dims)


def _mfcc_dims(sample_rate, n_fft, n_mfcc, n_mels):
    """nws_mfcc_dims of a configuration: (bins, n_mels, n_mfcc, jpad, nnz, off_w, off_dct, words)"""
    dims = (C.c_int32 * 8)()
    ok = all(0 <= v < 2 ** 31 for v in (n_fft, n_mfcc, n_mels))
    if not ok or _lib.lib().nws_mfcc_dims(sample_rate, n_fft, n_mfcc, n_mels, dims) != 0:
        raise RuntimeError(f"mfcc: unsupported configuration (sample_rate {sample_rate}, n_fft {n_fft}, n_mfcc {n_mfcc}, n_mels "
                           f"{n_mels}): sample_rate > 0, n_fft a power of two in [64, 2048], 1 <= n_mfcc <= n_mels <= 1024")
    return tuple(dims)


def _check_dev(name, t, like=None, like_name="out"):
    if not t.is_cuda:
        raise RuntimeError(f"{name} lives on {t.device}: the NEWT forward path only runs as HIP kernels on an AMD GPU "
                           "(there is no CPU fallback)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name}: expected Float, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name}: expected a contiguous tensor")
    if like is not None and t.device != like.device:
        raise RuntimeError(f"{like_name} is on {like.device} but {name} is on {t.device}: all tensors of one call must live on "
                           "the same GPU")


def _check_state(t, like=None):
    """a state blob: a contiguous uint8 tensor on the GPU (of `like`, the call's chunk)"""
    if not t.is_cuda:
        raise RuntimeError(f"state lives on {t.device}: the NEWT forward path only runs as HIP kernels on an AMD GPU "
                           "(there is no CPU fallback)")
    if t.dtype != torch.uint8:
        raise RuntimeError(f"state: expected Byte, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError("state: expected a contiguous tensor")
    if like is not None and t.device != like.device:
        raise RuntimeError(f"chunk is on {like.device} but state is on {t.device}: all tensors of one call must live on the same GPU")


class CtypesOps:
    def abi_version(self):
        return int(_lib.lib().nws_abi_version())

    # ---- whole forward and its halves ----------------------------------------------------------------------------------
    def forward(self, wdesc, f0, control, phase_u, rand_phase, noise, fir_design, plan, reverb_tables, reverb_spectrum,
                workspace, sample_rate):
        B, Cc, T = control.shape
        aux = _aux(fir_design, plan, reverb_tables, reverb_spectrum)
        with torch.cuda.device(f0.device):
            out = _new(f0, B, T * HOP)
            check(_lib.lib().nws_forward(C.byref(_struct(wdesc, NwsWeights)), C.byref(aux), ptr(f0), ptr(control), B, Cc, T,
                                         sample_rate, ptr(phase_u), ptr(rand_phase), ptr(noise), ptr(out), ptr(workspace),
                                         workspace.numel(), _stream(f0.device)), "nws_forward")
        return out

    def forward_control(self, wdesc, f0, control, workspace, batched_gru):
        B, Cc, T = control.shape
        with torch.cuda.device(f0.device):
            check(_lib.lib().nws_forward_control(C.byref(_struct(wdesc, NwsWeights)), ptr(f0), ptr(control), B, Cc, T,
                                                 1 if batched_gru else 0, ptr(workspace), workspace.numel(), _stream(f0.device)),
                  "nws_forward_control")

    def forward_audio(self, wdesc, f0, phase_u, rand_phase, noise, fir_design, plan, reverb_tables, reverb_spectrum, workspace,
                      sample_rate, out, wait_event, record_event):
        B, _, T = f0.shape
        aux = _aux(fir_design, plan, reverb_tables, reverb_spectrum)
        with torch.cuda.device(f0.device):
            if out is None:
                out = _new(f0, B, T * HOP)
            check(_lib.lib().nws_forward_audio_ev(C.byref(_struct(wdesc, NwsWeights)), C.byref(aux), ptr(f0), B, T, sample_rate,
                                                  ptr(phase_u), ptr(rand_phase), ptr(noise), ptr(out), ptr(workspace),
                                                  workspace.numel(), _stream(f0.device), wait_event or None, record_event or None),
                  "nws_forward_audio_ev")
        return out

    def forward_audio_pre(self, wdesc, f0, phase_u, rand_phase, noise, fir_design, plan, reverb_tables, reverb_spectrum,
                          workspace, sample_rate):
        B, _, T = f0.shape
        aux = _aux(fir_design, plan, reverb_tables, reverb_spectrum)
        with torch.cuda.device(f0.device):
            check(_lib.lib().nws_forward_audio_pre(C.byref(_struct(wdesc, NwsWeights)), C.byref(aux), ptr(f0), B, T, sample_rate,
                                                   ptr(phase_u), ptr(rand_phase), ptr(noise), ptr(workspace), workspace.numel(),
                                                   _stream(f0.device)), "nws_forward_audio_pre")

    def forward_audio_blocks(self, wdesc, f0, phase_u, rand_phase, noise, fir_design, plan, reverb_tables, reverb_spectrum,
                             workspace, sample_rate, out, row0, nrows, events):
        B, _, T = f0.shape
        n = len(row0)
        aux = _aux(fir_design, plan, reverb_tables, reverb_spectrum)
        with torch.cuda.device(f0.device):
            check(_lib.lib().nws_forward_audio_blocks(C.byref(_struct(wdesc, NwsWeights)), C.byref(aux), ptr(f0), B, T, sample_rate,
                                                      ptr(phase_u), ptr(rand_phase), ptr(noise), ptr(out), ptr(workspace),
                                                      workspace.numel(), _stream(f0.device), (C.c_int32 * n)(*row0),
                                                      (C.c_int32 * n)(*nrows), (C.c_void_p * n)(*events) if events else None, n),
                  "nws_forward_audio_blocks")

    def forward_reverb_rows(self, fir_design, plan, reverb_tables, reverb_spectrum, workspace, T, row0, nrows, out):
        aux = _aux(fir_design, plan, reverb_tables, reverb_spectrum)
        with torch.cuda.device(out.device):
            check(_lib.lib().nws_forward_reverb_rows(C.byref(aux), out.shape[0], T, row0, nrows, ptr(out), ptr(workspace),
                                                     workspace.numel(), _stream(out.device)), "nws_forward_reverb_rows")

    # ---- stages of the fused path ----------------------------------------------------------------------------------------
    def phase_carry(self, f0, f0_up):
        src = f0 if f0 is not None else f0_up
        B = src.shape[0]
        T = src.shape[-1] if f0 is not None else src.shape[-1] // HOP
        with torch.cuda.device(src.device):
            carry = _new(src, B, T * HOP // 32, dtype=torch.float64)
            check(_lib.lib().nws_phase_carry(ptr(f0), ptr(f0_up), B, T, ptr(carry), _stream(src.device)), "nws_phase_carry")
        return carry

    def exciter_newt(self, wdesc, f0, f0_up, carry, phase_u, rand_phase, film, sample_rate, want_exciter, want_newt):
        src = f0 if f0 is not None else f0_up
        B = src.shape[0]
        T = src.shape[-1] if f0 is not None else src.shape[-1] // HOP
        with torch.cuda.device(src.device):
            exc = _new(src, B, _lib.N_SHAPERS, T * HOP) if want_exciter else None
            out = _new(src, B, T * HOP) if want_newt else None
            check(_lib.lib().nws_exciter_newt(C.byref(_struct(wdesc, NwsWeights)), ptr(f0), ptr(f0_up), ptr(carry), ptr(phase_u),
                                              ptr(rand_phase), ptr(film), B, T, sample_rate, ptr(exc), ptr(out),
                                              _stream(src.device)), "nws_exciter_newt")
        return exc, out

    def oscillator(self, f0_up, phase_u, rand_phase, sample_rate):
        B, N = f0_up.shape
        with torch.cuda.device(f0_up.device):
            st = _stream(f0_up.device)
            carry = _new(f0_up, B, N // 32, dtype=torch.float64)
            out = _new(f0_up, B, _lib.N_HARMONICS, N)
            check(_lib.lib().nws_phase_carry(None, ptr(f0_up), B, N // HOP, ptr(carry), st), "nws_phase_carry")
            check(_lib.lib().nws_oscillator(ptr(f0_up), ptr(carry), ptr(phase_u), ptr(rand_phase), B, N, sample_rate, ptr(out), st),
                  "nws_oscillator")
        return out

    def control_gru(self, wdesc, control, h0, batched):
        B, Cc, T = control.shape
        fn = _lib.lib().nws_control_gru_batched if batched else _lib.lib().nws_control_gru_state
        with torch.cuda.device(control.device):
            out = _new(control, B, T, _lib.HIDDEN)
            hT = _new(control, B, _lib.HIDDEN)
            check(fn(C.byref(_struct(wdesc, NwsWeights)), ptr(control), B, Cc, T, ptr(h0), ptr(out), ptr(hT),
                     _stream(control.device)), "nws_control_gru")
        return out, hT

    def control_gru_grad(self, wdesc, control, h0, gru_out, grad_out, grad_hT, want_params):
        B, Cc, T = control.shape
        H = _lib.HIDDEN
        if B < 1 or T < 1:
            raise RuntimeError("control: need at least one utterance and one frame")
        for t in (gru_out, grad_out):
            if tuple(t.shape) != (B, T, H):
                raise RuntimeError(f"control_gru_grad: gru_out / grad_out {tuple(t.shape)} is not ({B}, {T}, {H})")
        for t in (h0, grad_hT):
            if t is not None and t.numel() != B * H:
                raise RuntimeError(f"h0 / grad_hT: expected ({B}, {H}), got {tuple(t.shape)}")
        L = _lib.lib()
        with torch.cuda.device(control.device):
            out = [_new(control, B, 2, T), _new(control, B, H)]
            if want_params:
                out += [_new(control, 3 * H, 2), _new(control, 3 * H, H), _new(control, 3 * H), _new(control, 3 * H)]
            gp = out[2:] if want_params else [None] * 4
            nbytes = L.nws_control_gru_grad_workspace_bytes(B, T, 1 if want_params else 0)
            ws = _new(control, max(nbytes, 1), dtype=torch.uint8)
            check(L.nws_control_gru_grad(C.byref(_struct(wdesc, NwsWeights)), ptr(control), B, Cc, T, ptr(h0), ptr(gru_out),
                                         ptr(grad_out), ptr(grad_hT), ptr(out[0]), ptr(out[1]), ptr(gp[0]), ptr(gp[1]), ptr(gp[2]),
                                         ptr(gp[3]), ptr(ws), nbytes, _stream(control.device)), "nws_control_gru_grad")
        return out

    def frame_mlps(self, wdesc, gru_out, fir_design, want_emb, want_H):
        B, T, _ = gru_out.shape
        with torch.cuda.device(gru_out.device):
            emb = _new(gru_out, B, _lib.HIDDEN, T) if want_emb else None
            film = _new(gru_out, B, T, _lib.FILM_CH)
            H = _new(gru_out, B, T, _lib.N_BANDS) if want_H else None
            fir = _new(gru_out, B, T, _lib.FIR_HALF)
            check(_lib.lib().nws_frame_mlps(C.byref(_struct(wdesc, NwsWeights)), ptr(gru_out), ptr(fir_design), B, T, ptr(emb),
                                            ptr(film), ptr(H), ptr(fir), _stream(gru_out.device)), "nws_frame_mlps")
        return emb, film, H, fir

    def fir_noise(self, fir, noise, add_in, origin):
        B, T, _ = fir.shape
        with torch.cuda.device(fir.device):
            out = _new(fir, B, T * HOP)
            if origin < 0:
                check(_lib.lib().nws_fir_noise(ptr(fir), ptr(noise), ptr(add_in), B, T, ptr(out), _stream(fir.device)), "nws_fir_noise")
            else:
                check(_lib.lib().nws_fir_noise_window(ptr(fir), ptr(noise), noise.numel(), origin, ptr(add_in), B, T, ptr(out),
                                                      _stream(fir.device)), "nws_fir_noise_window")
        return out

    def frame_mlps_spec(self, wdesc, gru_out):
        B, T, _ = gru_out.shape
        with torch.cuda.device(gru_out.device):
            film = _new(gru_out, B, T, _lib.FILM_CH)
            spec = torch.zeros((B, T, _lib.SPEC_ROW), dtype=torch.float32, device=gru_out.device)   # (3 floats per row never written)
            check(_lib.lib().nws_frame_mlps_spec(C.byref(_struct(wdesc, NwsWeights)), ptr(gru_out), B, T, ptr(film), ptr(spec),
                                                 _stream(gru_out.device)), "nws_frame_mlps_spec")
        return film, spec

    def fir_noise_spec(self, spec, noise, add_in):
        B, T, row = spec.shape
        if row != _lib.SPEC_ROW or noise.numel() != T * HOP - 1:
            raise RuntimeError(f"fir_noise_spec: spec {tuple(spec.shape)} must be (B, T, {_lib.SPEC_ROW}) and noise {tuple(noise.shape)} "
                               f"its {T * HOP - 1} samples")
        with torch.cuda.device(spec.device):
            out = _new(spec, B, T * HOP)
            check(_lib.lib().nws_fir_noise_spec(ptr(spec), ptr(noise), ptr(add_in), B, T, ptr(out), _stream(spec.device)),
                  "nws_fir_noise_spec")
        return out

    def fir_from_h(self, H, fir_design):
        B, _, T = H.shape
        with torch.cuda.device(H.device):
            fir = _new(H, B, T, _lib.FIR_HALF)
            check(_lib.lib().nws_fir_from_h(ptr(H), ptr(fir_design), B, T, ptr(fir), _stream(H.device)), "nws_fir_from_h")
        return fir

    def fir_noise_grad(self, noise, grad_out):
        B, N = grad_out.shape
        T = N // HOP
        if N != T * HOP or T < 2 or noise.numel() != N - 1:
            raise RuntimeError(f"fir_noise_grad: grad_out {tuple(grad_out.shape)} must be (B, 128 T) with T >= 2 and noise "
                               f"{tuple(noise.shape)} its {N - 1} samples")
        with torch.cuda.device(grad_out.device):
            grad_fir = _new(grad_out, B, T, _lib.FIR_HALF)
            check(_lib.lib().nws_fir_noise_grad(ptr(noise), ptr(grad_out), B, T, ptr(grad_fir), _stream(grad_out.device)),
                  "nws_fir_noise_grad")
        return grad_fir

    def fir_from_h_grad(self, grad_fir, fir_design):
        B, T, _ = grad_fir.shape
        with torch.cuda.device(grad_fir.device):
            grad_H = _new(grad_fir, B, _lib.N_BANDS, T)
            check(_lib.lib().nws_fir_from_h_grad(ptr(grad_fir), ptr(fir_design), B, T, ptr(grad_H), _stream(grad_fir.device)),
                  "nws_fir_from_h_grad")
        return grad_H

    def sum_batch_time(self, x):
        B, Cc, T = x.shape
        with torch.cuda.device(x.device):
            out = _new(x, Cc)
            check(_lib.lib().nws_sum_batch_time(ptr(x), B, Cc, T, ptr(out), _stream(x.device)), "nws_sum_batch_time")
        return out

    def reverb(self, plan, tables, spectrum, x):
        B, N = x.shape
        p = _plan(plan)
        with torch.cuda.device(x.device):
            nbytes = _lib.lib().nws_reverb_workspace_bytes(C.byref(p), B)
            ws = _new(x, nbytes, dtype=torch.uint8)
            y = torch.empty_like(x)
            check(_lib.lib().nws_reverb(C.byref(p), ptr(tables), ptr(spectrum), ptr(x), B, N, ptr(y), ptr(ws), nbytes,
                                        _stream(x.device)), "nws_reverb")
        return y

    def reverb_grad_x(self, plan, tables, spectrum, grad_out):
        B, N = grad_out.shape
        p = _plan(plan)
        with torch.cuda.device(grad_out.device):
            nbytes = _lib.lib().nws_reverb_grad_workspace_bytes(C.byref(p), B, 0)
            ws = _new(grad_out, nbytes, dtype=torch.uint8)
            dx = torch.empty_like(grad_out)
            check(_lib.lib().nws_reverb_grad_x(C.byref(p), ptr(tables), ptr(spectrum), ptr(grad_out), B, N, ptr(dx), ptr(ws), nbytes,
                                               _stream(grad_out.device)), "nws_reverb_grad_x")
        return dx

    def reverb_grad_ir(self, plan, tables, x, grad_out, ir_len):
        B, N = x.shape
        if tuple(grad_out.shape) != (B, N):
            raise RuntimeError(f"reverb_grad_ir: x {tuple(x.shape)} and grad_out {tuple(grad_out.shape)} differ in shape")
        p = _plan(plan)
        with torch.cuda.device(x.device):
            nbytes = _lib.lib().nws_reverb_grad_workspace_bytes(C.byref(p), B, 1)
            ws = _new(x, nbytes, dtype=torch.uint8)
            dir_ = _new(x, ir_len)
            check(_lib.lib().nws_reverb_grad_ir(C.byref(p), ptr(tables), ptr(x), ptr(grad_out), B, N, ir_len, ptr(dir_), ptr(ws),
                                                nbytes, _stream(x.device)), "nws_reverb_grad_ir")
        return dir_

    def reverb_linear_chunk(self, plan, tables, spectrum, x, tail_in):
        B, M = x.shape
        p = _plan(plan)
        with torch.cuda.device(x.device):
            nfl = (2 * ((B + 1) // 2) + B) * p.L
            ws = _new(x, nfl)
            y, tail_out = torch.empty_like(x), torch.empty_like(tail_in)
            check(_lib.lib().nws_reverb_linear_chunk(C.byref(p), ptr(tables), ptr(spectrum), ptr(x), B, M, ptr(tail_in),
                                                     ptr(tail_out), tail_in.shape[1], ptr(y), ptr(ws), nfl * 4, _stream(x.device)),
                  "nws_reverb_linear_chunk")
        return y, tail_out

    def shaper_apply(self, wdesc, x):
        with torch.cuda.device(x.device):
            y = torch.empty_like(x)
            check(_lib.lib().nws_shaper_apply(C.byref(_struct(wdesc, NwsWeights)), ptr(x), x.shape[0], x.shape[2], ptr(y),
                                              _stream(x.device)), "nws_shaper_apply")
        return y

    def shaper_table(self, wdesc, like, size, tmin, tmax):
        with torch.cuda.device(like.device):
            table = _new(like, _lib.N_SHAPERS, size)
            check(_lib.lib().nws_shaper_table(C.byref(_struct(wdesc, NwsWeights)), size, tmin, tmax, ptr(table), _stream(like.device)),
                  "nws_shaper_table")
        return table

    def newt_apply(self, wdesc, exciter, film):
        B, _, N = exciter.shape
        T = film.shape[2]
        if film.shape[1] != _lib.FILM_CH or N != T * HOP:
            raise RuntimeError(f"NEWT: exciter {tuple(exciter.shape)} and FiLM parameters {tuple(film.shape)} disagree")
        with torch.cuda.device(exciter.device):
            out = _new(exciter, B, 1, N)
            check(_lib.lib().nws_newt_apply(C.byref(_struct(wdesc, NwsWeights)), ptr(exciter), ptr(film), B, T, ptr(out),
                                            _stream(exciter.device)), "nws_newt_apply")
        return out

    def newt_grad(self, wdesc, exciter, film, grad_out, want_exciter, want_params):
        B, S, N = exciter.shape
        T = film.shape[2]
        if S != _lib.N_SHAPERS or tuple(film.shape) != (B, _lib.FILM_CH, T) or N != T * HOP:
            raise RuntimeError(f"NEWT: exciter {tuple(exciter.shape)} and FiLM parameters {tuple(film.shape)} disagree")
        if B < 1 or T < 1:
            raise RuntimeError("newt_grad: need at least one utterance and one frame")
        if grad_out.numel() != B * N or grad_out.shape[0] != B:
            raise RuntimeError(f"newt_grad: grad_out {tuple(grad_out.shape)} is not ({B}, 1, {N})")
        w = _struct(wdesc, NwsWeights)
        if w.lut:
            raise RuntimeError("newt_grad: the lookup table has no backward")
        L = _lib.lib()
        nbytes = L.nws_newt_grad_workspace_bytes(B, T, 1 if want_params else 0) if max(B, T) < 2 ** 30 else 0
        if nbytes == 0:
            raise RuntimeError(f"newt_grad: unsupported size (B {B}, T {T}): T <= 65535, B T <= 2^28")
        with torch.cuda.device(exciter.device):
            out = [_new(exciter, B, _lib.FILM_CH, T)]
            ge = torch.empty_like(exciter) if want_exciter else None
            if want_exciter:
                out.append(ge)
            gp = [None] * 11
            if want_params:
                SW = S * _lib.SHAPER_WIDTH
                shapes = [(1, S, 1), (SW, 1, 1), (SW,), (SW, 8, 1), (SW,), (SW, 8, 1), (SW,), (S, 8, 1), (S,), (1, S, 1), (1,)]
                gp = [_new(exciter, *sh) for sh in shapes]
                out += gp
            ws = _new(exciter, nbytes, dtype=torch.uint8)
            check(L.nws_newt_grad(C.byref(w), ptr(exciter), ptr(film), ptr(grad_out), B, T, ptr(ge), ptr(out[0]),
                                  *[ptr(t) for t in gp], ptr(ws), nbytes, _stream(exciter.device)), "nws_newt_grad")
        return out

    def adam_step(self, params, grads, exp_avgs, exp_avg_sqs, step, lr, beta1, beta2, eps, max_norm):
        n = len(params)
        if n < 1:
            raise RuntimeError("adam_step: no tensors")
        if not (len(grads) == len(exp_avgs) == len(exp_avg_sqs) == n):
            raise RuntimeError(f"adam_step: {n} params but {len(grads)} grads, {len(exp_avgs)} exp_avgs, {len(exp_avg_sqs)} exp_avg_sqs")
        if step < 1:
            raise RuntimeError(f"adam_step: step counts from 1, got {step}")
        recs = (_lib.NwsAdamTensor * n)()
        for k, (p, g, m, v) in enumerate(zip(params, grads, exp_avgs, exp_avg_sqs)):
            for name, t in (("param", p), ("grad", g), ("exp_avg", m), ("exp_avg_sq", v)):
                if not t.is_cuda:
                    raise RuntimeError(f"{name} lives on {t.device}: the NEWT forward path only runs as HIP kernels on an AMD GPU "
                                       "(there is no CPU fallback)")
                if t.dtype != torch.float32:
                    raise RuntimeError(f"{name}: expected Float, got {t.dtype}")
                if not t.is_contiguous():
                    raise RuntimeError(f"{name}: expected a contiguous tensor")
                if t.device != params[0].device:
                    raise RuntimeError(f"{name} is on {t.device} but params[0] is on {params[0].device}: all tensors of one call must "
                                       "live on the same GPU")
            if not (g.shape == m.shape == v.shape == p.shape):
                raise RuntimeError(f"adam_step: tensor {k}: param {tuple(p.shape)}, grad {tuple(g.shape)}, exp_avg {tuple(m.shape)}, "
                                   f"exp_avg_sq {tuple(v.shape)} differ in shape")
            if p.numel() < 1:
                raise RuntimeError(f"adam_step: tensor {k} is empty")
            recs[k] = _lib.NwsAdamTensor(ptr(p), ptr(g), ptr(m), ptr(v), p.numel())
        L = _lib.lib()
        nbytes = L.nws_adam_workspace_bytes(recs, n)
        if nbytes == 0:
            raise RuntimeError("adam_step: unsupported sizes")
        like = params[0]
        with torch.cuda.device(like.device):
            total = torch.empty((), dtype=torch.float32, device=like.device)
            ws = _new(like, nbytes // 8, dtype=torch.float64)
            check(L.nws_adam_step(recs, n, int(step), lr, beta1, beta2, eps, max_norm, ptr(total), ptr(ws), nbytes,
                                  _stream(like.device)), "nws_adam_step")
        # the kernels wrote through raw pointers: everything that caches tables derived from the weights keys on ._version
        torch.autograd.graph.increment_version(list(params) + list(exp_avgs) + list(exp_avg_sqs))
        return total

    def grad_pack(self, tensors, out):
        n = len(tensors)
        if n < 1:
            raise RuntimeError("grad_pack: no tensors")
        _check_dev("out", out)
        if out.dim() != 1:
            raise RuntimeError(f"grad_pack: out: expected a 1-D tensor, got {tuple(out.shape)}")
        recs = (_lib.NwsGradTensor * n)()
        for k, t in enumerate(tensors):
            _check_dev("tensor", t, out)
            if t.numel() < 1:
                raise RuntimeError(f"grad_pack: tensor {k} is empty")
            recs[k] = _lib.NwsGradTensor(ptr(t), t.numel())
        total = sum(t.numel() for t in tensors)
        if out.numel() < total:
            raise RuntimeError(f"grad_pack: out holds {out.numel()} elements, the tensors have {total}")
        with torch.cuda.device(out.device):
            check(_lib.lib().nws_grad_pack(recs, n, ptr(out), out.numel(), _stream(out.device)), "nws_grad_pack")
        torch.autograd.graph.increment_version(out)          # written through a raw pointer

    def grad_reduce(self, rows, out):
        _check_dev("rows", rows)
        _check_dev("out", out, rows, "rows")
        if rows.dim() != 2 or rows.shape[0] < 1:
            raise RuntimeError(f"grad_reduce: rows: expected (world, stride), got {tuple(rows.shape)}")
        if out.dim() != 1 or not 1 <= out.numel() <= rows.shape[1]:
            raise RuntimeError(f"grad_reduce: out: expected a 1-D tensor of 1 .. {rows.shape[1]} elements (the rows' stride), got "
                               f"{tuple(out.shape)}")
        with torch.cuda.device(rows.device):
            check(_lib.lib().nws_grad_reduce(ptr(rows), min(int(rows.shape[0]), 1 << 30), out.numel(), int(rows.shape[1]), ptr(out),
                                             _stream(rows.device)), "nws_grad_reduce")
        torch.autograd.graph.increment_version(out)          # written through a raw pointer

    # ---- stand-alone stage kernels (csrc/stages.hip) ---------------------------------------------------------------------
    def td_mlp(self, x, weights, biases, ln_w, ln_b, eps, slope):
        B, in_size, T = x.shape
        hidden, out_size = weights[0].shape[0], weights[-1].shape[0]
        with torch.cuda.device(x.device):
            y = _new(x, B, out_size, T)
            check(_lib.lib().nws_td_mlp(ptr(x), B, in_size, hidden, out_size, len(weights), T, _ptrs(weights), _ptrs(biases),
                                        _ptrs(ln_w), _ptrs(ln_b), eps, slope, ptr(y), _stream(x.device)), "nws_td_mlp")
        return y

    def td_mlp_grad(self, x, grad_y, weights, biases, ln_w, ln_b, eps, slope, want_params):
        B, in_size, T = x.shape
        depth = len(weights)
        hidden, out_size = weights[0].shape[0], weights[-1].shape[0]
        if tuple(grad_y.shape) != (B, out_size, T):
            raise RuntimeError(f"td_mlp_grad: grad_y {tuple(grad_y.shape)} is not ({B}, {out_size}, {T})")
        if len(biases) != depth or len(ln_w) != depth - 1 or len(ln_b) != depth - 1:
            raise RuntimeError("td_mlp_grad: inconsistent layer lists")
        L = _lib.lib()
        with torch.cuda.device(x.device):
            grad_x = torch.empty_like(x)
            gw, gb, gg, gl, ws, nbytes = [], [], [], [], None, 0
            if want_params:
                gw, gb = [torch.empty_like(t) for t in weights], [torch.empty_like(t) for t in biases]
                gg, gl = [torch.empty_like(t) for t in ln_w], [torch.empty_like(t) for t in ln_b]
                nbytes = L.nws_td_mlp_grad_workspace_bytes(B, in_size, hidden, out_size, depth, T, 1)
                ws = _new(x, max(nbytes, 1), dtype=torch.uint8)
            none = None
            check(L.nws_td_mlp_grad(ptr(x), ptr(grad_y), B, in_size, hidden, out_size, depth, T, _ptrs(weights), _ptrs(biases),
                                    _ptrs(ln_w), _ptrs(ln_b), eps, slope, ptr(grad_x), _ptrs(gw) if want_params else none,
                                    _ptrs(gb) if want_params else none, _ptrs(gg) if want_params else none,
                                    _ptrs(gl) if want_params else none, ptr(ws), nbytes, _stream(x.device)), "nws_td_mlp_grad")
        return [grad_x] + gw + gb + gg + gl

    def td_layer_norm(self, x, weight, bias, eps):
        with torch.cuda.device(x.device):
            y = torch.empty_like(x)
            check(_lib.lib().nws_td_layer_norm(ptr(x), ptr(weight), ptr(bias), x.shape[0], x.shape[1], x.shape[2], eps, ptr(y),
                                               _stream(x.device)), "nws_td_layer_norm")
        return y

    def film(self, x, gamma, beta):
        with torch.cuda.device(x.device):
            y = torch.empty_like(x)
            check(_lib.lib().nws_film(ptr(x), ptr(gamma), ptr(beta), x.numel(), ptr(y), _stream(x.device)), "nws_film")
        return y

    def sine(self, x):
        with torch.cuda.device(x.device):
            y = torch.empty_like(x)
            check(_lib.lib().nws_sin(ptr(x), ptr(y), x.numel(), _stream(x.device)), "nws_sin")
        return y

    def loudness(self, audio, dft, n_fft, hop, amin, top_db, normalise):
        B, N = audio.shape
        L = _lib.lib()
        with torch.cuda.device(audio.device):
            ws = _new(audio, L.nws_loudness_workspace_bytes(B, N, n_fft, hop), dtype=torch.uint8)
            out = _new(audio, B, L.nws_loudness_frames(N, hop))
            check(L.nws_loudness(ptr(audio), B, N, n_fft, hop, ptr(dft), amin, top_db, 1 if normalise else 0, ptr(out), ptr(ws),
                                 ws.numel(), _stream(audio.device)), "nws_loudness")
        return out

    @staticmethod
    def _check_loudness_sizes(op, dft, n_fft, hop):
        L = _lib.lib()
        if L.nws_loudness_workspace_bytes(1, 1, n_fft, hop) == 0:
            raise RuntimeError(f"{op}: unsupported n_fft / hop_length ({n_fft}, {hop}): n_fft must be a power of two in [64, 2048], "
                               "1 <= hop <= n_fft and 31 hop + n_fft samples must fit 160 KB of LDS")
        if dft.numel() * 4 != L.nws_loudness_dft_bytes(n_fft):
            raise RuntimeError(f"{op}: dft does not belong to n_fft = {n_fft}")

    def loudness_peak_power(self, audio, dft, n_fft, hop):
        _check_dev("audio", audio)
        _check_dev("dft", dft, audio, "audio")
        if audio.dim() != 2 or audio.shape[0] < 1:
            raise RuntimeError(f"loudness_peak_power: expected (B, N), got {tuple(audio.shape)}")
        B, N = audio.shape
        self._check_loudness_sizes("loudness_peak_power", dft, n_fft, hop)
        if N <= n_fft // 2:
            raise RuntimeError(f"loudness_peak_power: N = {N}: the reflect padding needs more than n_fft / 2 = {n_fft // 2} samples")
        L = _lib.lib()
        with torch.cuda.device(audio.device):
            nbytes = L.nws_loudness_workspace_bytes(B, N, n_fft, hop)
            ws = _new(audio, nbytes, dtype=torch.uint8)
            out = _new(audio, B)
            check(L.nws_loudness_peak_power(ptr(audio), B, N, n_fft, hop, ptr(dft), ptr(out), ptr(ws), nbytes, _stream(audio.device)),
                  "nws_loudness_peak_power")
        return out

    # ---- loudness stream (csrc/loudness_stream.hip): the state blob is a uint8 tensor on the device --------------------------
    @staticmethod
    def _loudness_stream_bytes(op, B, n_fft, hop):
        nbytes = _lib.lib().nws_loudness_stream_state_bytes(B, n_fft, hop) if 1 <= B <= 65535 else 0
        if nbytes == 0:
            raise RuntimeError(f"{op}: unsupported stream (B {B}, n_fft {n_fft}, hop {hop}): 1 <= B <= 65535, sizes the offline "
                               "extractor serves and at most 256 hops in half a frame")
        return nbytes

    def loudness_stream_reset(self, state, B, n_fft, hop, initial_power, track):
        _check_state(state)
        _check_dev("initial_power", initial_power, state, "state")
        nbytes = self._loudness_stream_bytes("loudness_stream_reset", B, n_fft, hop)
        if state.numel() < nbytes:
            raise RuntimeError(f"loudness_stream_reset: state blob too small (expected {nbytes} bytes for B = {B}, got {state.numel()})")
        if initial_power.dim() != 1 or initial_power.shape[0] != B:
            raise RuntimeError(f"loudness_stream_reset: initial_power: expected ({B}), got {tuple(initial_power.shape)}")
        with torch.cuda.device(state.device):
            check(_lib.lib().nws_loudness_stream_reset(ptr(state), state.numel(), B, n_fft, hop, ptr(initial_power), 1 if track else 0,
                                                       _stream(state.device)), "nws_loudness_stream_reset")

    def loudness_stream_reset_release(self, state, B, n_fft, hop, floor_power):
        _check_state(state)
        _check_dev("floor_power", floor_power, state, "state")
        self._loudness_stream_bytes("loudness_stream_reset_release", B, n_fft, hop)
        nbytes = _lib.lib().nws_loudness_stream_release_state_bytes(B, n_fft, hop)
        if state.numel() < nbytes:
            raise RuntimeError(f"loudness_stream_reset_release: state blob too small (expected {nbytes} bytes for B = {B}, got {state.numel()})")
        if floor_power.dim() != 1 or floor_power.shape[0] != B:
            raise RuntimeError(f"loudness_stream_reset_release: floor_power: expected ({B}), got {tuple(floor_power.shape)}")
        with torch.cuda.device(state.device):
            check(_lib.lib().nws_loudness_stream_reset_release(ptr(state), state.numel(), B, n_fft, hop, ptr(floor_power),
                                                               _stream(state.device)), "nws_loudness_stream_reset_release")

    def loudness_stream_step(self, state, dft, n_fft, hop, lag, chunk, n_seen, final, amin, top_db, normalise, loudness,
                             reference_power):
        self._loudness_stream_step("loudness_stream_step", False, state, dft, n_fft, hop, lag, 1.0, True, chunk, n_seen, final, amin,
                                   top_db, normalise, loudness, reference_power)

    def loudness_stream_step_release(self, state, dft, n_fft, hop, lag, release_factor, track, chunk, n_seen, final, amin, top_db,
                                     normalise, loudness, reference_power):
        self._loudness_stream_step("loudness_stream_step_release", True, state, dft, n_fft, hop, lag, release_factor, track, chunk,
                                   n_seen, final, amin, top_db, normalise, loudness, reference_power)

    def _loudness_stream_step(self, op, with_release, state, dft, n_fft, hop, lag, release_factor, track, chunk, n_seen, final, amin,
                              top_db, normalise, loudness, reference_power):
        """the step of both ops.  with_release: loudness_stream_step_release, whose release_factor 1 is loudness_stream_step on either
        kind of blob; below 1 the blob is loudness_stream_reset_release's, hence track"""
        _check_dev("chunk", chunk)
        _check_dev("loudness", loudness, chunk, "chunk")
        _check_state(state, chunk)
        _check_dev("dft", dft, chunk, "chunk")
        if chunk.dim() != 2 or chunk.shape[0] < 1:
            raise RuntimeError(f"{op}: expected a (B, n) chunk, got {tuple(chunk.shape)}")
        B, n = chunk.shape
        lib = _lib.lib()
        nbytes = self._loudness_stream_bytes(op, B, n_fft, hop)
        releasing = release_factor < 1.0
        rbytes = lib.nws_loudness_stream_release_state_bytes(B, n_fft, hop)
        if with_release:
            if not 0.0 < release_factor <= 1.0:
                raise RuntimeError(f"{op}: release_factor {release_factor} outside (0, 1]")
            if releasing and not track:
                raise RuntimeError(f"{op}: a release needs a tracked reference")
        have = state.numel()
        if not (have == rbytes if releasing else have == nbytes or (with_release and have == rbytes)):
            raise RuntimeError(f"{op}: state does not belong to a stream of B = {B} rows of this configuration "
                               f"(expected {rbytes if releasing else nbytes} bytes, got {state.numel()})")
        self._check_loudness_sizes(op, dft, n_fft, hop)
        if not 0 <= lag <= 255:
            raise RuntimeError(f"{op}: lag {lag} outside 0 .. 255")
        if not (amin > 0.0 and top_db >= 0.0):
            raise RuntimeError(f"{op}: amin must be positive and top_db non-negative")
        if n < 1 and not final:
            raise RuntimeError(f"{op}: empty chunk (only a final step may carry no samples)")
        max_chunk = lib.nws_loudness_stream_max_chunk(n_fft, hop)
        if n > max_chunk:
            raise RuntimeError(f"{op}: a step takes at most {max_chunk} samples at this hop, got {n}")
        if final and n_seen + n <= n_fft // 2:
            raise RuntimeError(f"{op}: a stream of {n_seen + n} samples cannot end: the reflect padding needs more "
                               f"than n_fft / 2 = {n_fft // 2}")
        before = lib.nws_loudness_stream_emitted(n_seen, n_fft, hop, lag, 0) if n_seen >= 0 else -1
        after = lib.nws_loudness_stream_emitted(n_seen + n, n_fft, hop, lag, 1 if final else 0) if n_seen >= 0 else -1
        if before < 0 or after < 0:
            raise RuntimeError(f"{op}: n_seen {n_seen} + {n} samples outside 0 .. 2^21 hops")
        m = after - before
        for name, t in (("loudness", loudness), ("reference_power", reference_power)):
            if (not t.is_cuda or t.device != chunk.device or t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 2
                    or t.shape[0] != B or t.shape[1] != loudness.shape[1] or not max(m, 1) <= t.shape[1] < 2 ** 31):
                raise RuntimeError(f"{op}: {name}: expected a contiguous ({B}, >= {max(m, 1)}) Float tensor on the "
                                   f"chunk's GPU, the same width for both outputs, got {tuple(t.shape)} {t.dtype} on {t.device}")
        with torch.cuda.device(chunk.device):
            ws_bytes = lib.nws_loudness_stream_workspace_bytes(B, n, n_fft, hop, 1 if final else 0)
            ws = _new(chunk, ws_bytes, dtype=torch.uint8)
            x = ptr(chunk) if n > 0 else None
            if with_release:
                check(lib.nws_loudness_stream_step_release(ptr(state), state.numel(), x, B, n, n_seen, n_fft, hop, lag, release_factor,
                                                           1 if track else 0, ptr(dft), amin, top_db, 1 if normalise else 0,
                                                           1 if final else 0, ptr(loudness), ptr(reference_power), loudness.shape[1],
                                                           ptr(ws), ws_bytes, _stream(chunk.device)), "nws_loudness_stream_step_release")
            else:
                check(lib.nws_loudness_stream_step(ptr(state), state.numel(), x, B, n, n_seen, n_fft, hop, lag, ptr(dft), amin, top_db,
                                                   1 if normalise else 0, 1 if final else 0, ptr(loudness), ptr(reference_power),
                                                   loudness.shape[1], ptr(ws), ws_bytes, _stream(chunk.device)),
                      "nws_loudness_stream_step")

    def loudness_causal(self, audio, dft, n_fft, hop, lag, release_factor, floor_power, track, amin, top_db, normalise):
        _check_dev("audio", audio)
        _check_dev("dft", dft, audio, "audio")
        _check_dev("floor_power", floor_power, audio, "audio")
        if audio.dim() != 2 or audio.shape[0] < 1:
            raise RuntimeError(f"loudness_causal: expected (B, N), got {tuple(audio.shape)}")
        B, N = audio.shape
        self._check_loudness_sizes("loudness_causal", dft, n_fft, hop)
        if N <= n_fft // 2:
            raise RuntimeError(f"loudness_causal: N = {N}: the reflect padding needs more than n_fft / 2 = {n_fft // 2} samples")
        if not 0 <= lag <= 255:
            raise RuntimeError(f"loudness_causal: lag {lag} outside 0 .. 255")
        if not (amin > 0.0 and top_db >= 0.0):
            raise RuntimeError("loudness_causal: amin must be positive and top_db non-negative")
        if not 0.0 < release_factor <= 1.0:
            raise RuntimeError(f"loudness_causal: release_factor {release_factor} outside (0, 1]")
        if release_factor != 1.0 and not track:
            raise RuntimeError("loudness_causal: a release needs a tracked reference")
        if floor_power.dim() != 1 or floor_power.shape[0] != B:
            raise RuntimeError(f"loudness_causal: floor_power: expected ({B}), got {tuple(floor_power.shape)}")
        L = _lib.lib()
        nbytes = L.nws_loudness_causal_workspace_bytes(B, N, n_fft, hop) if B <= 65535 and N < 2 ** 31 else 0
        if nbytes == 0:
            raise RuntimeError(f"loudness_causal: unsupported clip (B {B}, N {N}, n_fft {n_fft}, hop {hop}): 1 <= B <= 65535, sizes the "
                               "loudness stream serves (at most 256 hops in half a frame) and at most 2^21 hops")
        with torch.cuda.device(audio.device):
            ws = _new(audio, nbytes, dtype=torch.uint8)
            T = L.nws_loudness_frames(N, hop)
            loud, ref, peak = _new(audio, B, T), _new(audio, B, T), _new(audio, B, T)
            check(L.nws_loudness_causal(ptr(audio), B, N, n_fft, hop, ptr(dft), lag, release_factor, ptr(floor_power), 1 if track else 0,
                                        amin, top_db, 1 if normalise else 0, ptr(loud), ptr(ref), ptr(peak), ptr(ws), nbytes,
                                        _stream(audio.device)), "nws_loudness_causal")
        return loud, ref, peak

    # ---- pYIN F0 extractor (csrc/pyin.hip) -------------------------------------------------------------------------------
    def pyin_table(self, sample_rate, fmin, fmax, frame_length, hop):
        cfg = (sample_rate, fmin, fmax, frame_length, hop)
        table = torch.empty(_pyin_dims(cfg)[8], dtype=torch.float64)
        check(_lib.lib().nws_pyin_table(*cfg, table.data_ptr()), "nws_pyin_table")
        return table

    def pyin_cmnd(self, audio, sample_rate, fmin, fmax, frame_length, hop):
        cfg = (sample_rate, fmin, fmax, frame_length, hop)
        B, N = audio.shape
        L = _lib.lib()
        with torch.cuda.device(audio.device):
            yin = _new(audio, B, L.nws_pyin_frames(N, hop), _pyin_dims(cfg)[2])
            check(L.nws_pyin_cmnd(ptr(audio), B, N, *cfg, ptr(yin), _stream(audio.device)), "nws_pyin_cmnd")
        return yin

    def pyin_observe(self, yin, table, sample_rate, fmin, fmax, frame_length, hop):
        cfg = (sample_rate, fmin, fmax, frame_length, hop)
        B, T, lags = yin.shape
        if lags != _pyin_dims(cfg, table)[2]:
            raise RuntimeError(f"pyin_observe: yin {tuple(yin.shape)} does not belong to this configuration")
        with torch.cuda.device(yin.device):
            cand_bin = _new(yin, B, T, lags, dtype=torch.int32)
            cand_prob = _new(yin, B, T, lags, dtype=torch.float64)
            count = _new(yin, B, T, dtype=torch.int32)
            voiced_prob = _new(yin, B, T, dtype=torch.float64)
            check(_lib.lib().nws_pyin_observe(ptr(yin), B, T, *cfg, ptr(table), ptr(cand_bin), ptr(cand_prob), ptr(count),
                                              ptr(voiced_prob), _stream(yin.device)), "nws_pyin_observe")
        return cand_bin, cand_prob, count, voiced_prob

    def pyin_viterbi(self, cand_bin, cand_prob, count, voiced_prob, table, sample_rate, fmin, fmax, frame_length, hop,
                     fill_unvoiced, fill_value):
        cfg = (sample_rate, fmin, fmax, frame_length, hop)
        B, T, lags = cand_bin.shape
        if lags != _pyin_dims(cfg, table)[2] or cand_prob.shape != cand_bin.shape or count.shape != (B, T) or voiced_prob.shape != (B, T):
            raise RuntimeError("pyin_viterbi: observation tensors disagree on (B, T, lags)")
        L = _lib.lib()
        with torch.cuda.device(cand_bin.device):
            nbytes = L.nws_pyin_workspace_bytes(B, (T - 1) * hop + 1, *cfg)
            ws = _new(cand_bin, nbytes, dtype=torch.uint8)
            states = _new(cand_bin, B, T, dtype=torch.int32)
            f0 = _new(cand_bin, B, T)
            check(L.nws_pyin_viterbi(ptr(cand_bin), ptr(cand_prob), ptr(count), ptr(voiced_prob), B, T, *cfg, ptr(table),
                                     1 if fill_unvoiced else 0, fill_value, ptr(states), ptr(f0), ptr(ws), nbytes,
                                     _stream(cand_bin.device)), "nws_pyin_viterbi")
        return states, f0

    def pyin(self, audio, table, sample_rate, fmin, fmax, frame_length, hop, fill_unvoiced, fill_value):
        cfg = (sample_rate, fmin, fmax, frame_length, hop)
        B, N = audio.shape
        _pyin_dims(cfg, table)
        L = _lib.lib()
        with torch.cuda.device(audio.device):
            nbytes = L.nws_pyin_workspace_bytes(B, N, *cfg)
            if nbytes == 0:
                raise RuntimeError("pyin: unsupported size")
            T = L.nws_pyin_frames(N, hop)
            ws = _new(audio, nbytes, dtype=torch.uint8)
            f0 = _new(audio, B, T)
            voiced_prob = _new(audio, B, T, dtype=torch.float64)
            states = _new(audio, B, T, dtype=torch.int32)
            check(L.nws_pyin(ptr(audio), B, N, *cfg, ptr(table), 1 if fill_unvoiced else 0, fill_value, ptr(f0), ptr(voiced_prob),
                             ptr(states), ptr(ws), nbytes, _stream(audio.device)), "nws_pyin")
        return f0, voiced_prob, states

    # ---- fixed-lag pYIN stream (csrc/pyin_stream.hip): the state blob is a uint8 tensor on the device ------------------------
    @staticmethod
    def _pyin_stream_bytes(op, B, cfg):
        _pyin_dims(cfg)
        nbytes = _lib.lib().nws_pyin_stream_state_bytes(B, *cfg) if 1 <= B <= 65535 else 0
        if nbytes == 0:
            raise RuntimeError(f"{op}: unsupported stream (B {B}, frame_length {cfg[3]}, hop {cfg[4]}): 1 <= B <= 65535 and at most "
                               "256 hops in half a frame")
        return nbytes

    def pyin_stream_reset(self, state, B, sample_rate, fmin, fmax, frame_length, hop):
        _check_state(state)
        cfg = (sample_rate, fmin, fmax, frame_length, hop)
        nbytes = self._pyin_stream_bytes("pyin_stream_reset", B, cfg)
        if state.numel() < nbytes:
            raise RuntimeError(f"pyin_stream_reset: state blob too small (expected {nbytes} bytes for B = {B}, got {state.numel()})")
        with torch.cuda.device(state.device):
            check(_lib.lib().nws_pyin_stream_reset(ptr(state), state.numel(), B, *cfg, _stream(state.device)), "nws_pyin_stream_reset")

    def pyin_stream_step(self, state, table, sample_rate, fmin, fmax, frame_length, hop, lag, chunk, n_seen, final, fill_unvoiced,
                         fill_value, f0, voiced_prob, states):
        _check_dev("chunk", chunk)
        _check_dev("f0", f0, chunk, "chunk")
        _check_state(state, chunk)
        cfg = (sample_rate, fmin, fmax, frame_length, hop)
        _pyin_dims(cfg, table)
        if table.device != chunk.device:
            raise RuntimeError(f"chunk is on {chunk.device} but table is on {table.device}: all tensors of one call must live on the "
                               "same GPU")
        if chunk.dim() != 2 or chunk.shape[0] < 1:
            raise RuntimeError(f"pyin_stream_step: expected a (B, n) chunk, got {tuple(chunk.shape)}")
        B, n = chunk.shape
        lib = _lib.lib()
        nbytes = self._pyin_stream_bytes("pyin_stream_step", B, cfg)
        if state.numel() != nbytes:
            raise RuntimeError(f"pyin_stream_step: state does not belong to a stream of B = {B} rows of this configuration (expected "
                               f"{nbytes} bytes, got {state.numel()})")
        if not 0 <= lag <= 255:
            raise RuntimeError(f"pyin_stream_step: lag {lag} outside 0 .. 255")
        if n < 1 and not final:
            raise RuntimeError("pyin_stream_step: empty chunk (only a final step may carry no samples)")
        max_chunk = lib.nws_pyin_stream_max_chunk(*cfg)
        if n > max_chunk:
            raise RuntimeError(f"pyin_stream_step: a step takes at most {max_chunk} samples at this hop, got {n}")
        if final and n_seen + n <= frame_length // 2:
            raise RuntimeError(f"pyin_stream_step: a stream of {n_seen + n} samples cannot end: the reflect padding needs more than "
                               f"frame_length / 2 = {frame_length // 2}")
        before = lib.nws_pyin_stream_emitted(n_seen, *cfg, lag, 0) if n_seen >= 0 else -1
        after = lib.nws_pyin_stream_emitted(n_seen + n, *cfg, lag, 1 if final else 0) if n_seen >= 0 else -1
        if before < 0 or after < 0:
            raise RuntimeError(f"pyin_stream_step: n_seen {n_seen} + {n} samples outside 0 .. 2^21 hops")
        m = after - before
        for name, t, dt in (("f0", f0, torch.float32), ("voiced_prob", voiced_prob, torch.float64), ("states", states, torch.int32)):
            if (not t.is_cuda or t.device != chunk.device or t.dtype != dt or not t.is_contiguous() or t.dim() != 2 or t.shape[0] != B
                    or t.shape[1] != f0.shape[1] or not max(m, 1) <= t.shape[1] < 2 ** 31):
                raise RuntimeError(f"pyin_stream_step: {name}: expected a contiguous ({B}, >= {max(m, 1)}) {dt} tensor on the chunk's GPU, the "
                                   f"same width for all three outputs, got {tuple(t.shape)} {t.dtype} on {t.device}")
        with torch.cuda.device(chunk.device):
            ws_bytes = lib.nws_pyin_stream_workspace_bytes(B, n, *cfg, 1 if final else 0)
            ws = _new(chunk, ws_bytes, dtype=torch.uint8)
            check(lib.nws_pyin_stream_step(ptr(state), state.numel(), ptr(chunk) if n > 0 else None, B, n, n_seen, *cfg, lag, ptr(table),
                                           1 if final else 0, 1 if fill_unvoiced else 0, fill_value, ptr(f0), ptr(voiced_prob),
                                           ptr(states), f0.shape[1], ptr(ws), ws_bytes, _stream(chunk.device)),
                  "nws_pyin_stream_step")

    # ---- sample-rate converter (csrc/resample.hip) ------------------------------------------------------------------------
    def resample_bank(self, sr_in, sr_out):
        L, _, taps = _resample_dims(sr_in, sr_out)[:3]
        bank = torch.empty(L, taps, dtype=torch.float32)
        check(_lib.lib().nws_resample_bank(sr_in, sr_out, bank.data_ptr()), "nws_resample_bank")
        return bank

    def resample(self, audio, bank, sr_in, sr_out):
        L, _, taps = _resample_dims(sr_in, sr_out)[:3]
        if not bank.is_cuda or bank.dtype != torch.float32 or tuple(bank.shape) != (L, taps) or bank.device != audio.device:
            raise RuntimeError(f"resample: bank does not belong to these rates (expected a ({L}, {taps}) float32 tensor on the "
                               f"audio's device, got {tuple(bank.shape)} {bank.dtype} on {bank.device})")
        B, N = audio.shape
        n_out = _lib.lib().nws_resample_length(N, sr_in, sr_out)
        if n_out < 1 or B < 1:
            raise RuntimeError(f"resample: {N} samples at {sr_in} Hz give no sample at {sr_out} Hz")
        with torch.cuda.device(audio.device):
            y = _new(audio, B, n_out)
            check(_lib.lib().nws_resample(ptr(audio), B, N, sr_in, sr_out, ptr(bank), ptr(y), _stream(audio.device)), "nws_resample")
        return y

    # ---- streaming sample-rate converter (csrc/resample_stream.hip): the state blob is a uint8 tensor on the device ----------
    @staticmethod
    def _resample_stream_bytes(op, dims, B, sr_in, sr_out):
        nbytes = _lib.lib().nws_resample_stream_state_bytes(B, sr_in, sr_out) if 1 <= B <= 65535 else 0
        if nbytes == 0:
            raise RuntimeError(f"{op}: unsupported stream (B {B}, {sr_in} -> {sr_out} Hz): 1 <= B <= 65535, and the {dims[2] - 1} "
                               f"samples of history and {dims[4]} of look-ahead must leave room for a chunk in 64 KB of LDS")
        return nbytes

    def resample_stream_reset(self, state, B, sr_in, sr_out):
        _check_state(state)
        nbytes = self._resample_stream_bytes("resample_stream_reset", _resample_dims(sr_in, sr_out), B, sr_in, sr_out)
        if state.numel() < nbytes:
            raise RuntimeError(f"resample_stream_reset: state blob too small (expected {nbytes} bytes for B = {B}, got {state.numel()})")
        with torch.cuda.device(state.device):
            check(_lib.lib().nws_resample_stream_reset(ptr(state), state.numel(), B, sr_in, sr_out, _stream(state.device)),
                  "nws_resample_stream_reset")

    def resample_stream_step(self, state, bank, sr_in, sr_out, chunk, final, out):
        _check_dev("chunk", chunk)
        _check_dev("bank", bank, chunk, "chunk")
        _check_dev("out", out, chunk, "chunk")
        _check_state(state, chunk)
        dims = _resample_dims(sr_in, sr_out)
        L, _, taps = dims[:3]
        if chunk.dim() != 2 or chunk.shape[0] < 1:
            raise RuntimeError(f"resample_stream_step: expected a (B, n) chunk, got {tuple(chunk.shape)}")
        if tuple(bank.shape) != (L, taps):
            raise RuntimeError(f"resample_stream_step: bank does not belong to these rates (expected ({L}, {taps}), got "
                               f"{tuple(bank.shape)})")
        B, n = chunk.shape
        lib = _lib.lib()
        nbytes = self._resample_stream_bytes("resample_stream_step", dims, B, sr_in, sr_out)
        if state.numel() != nbytes:
            raise RuntimeError(f"resample_stream_step: state does not belong to a stream of B = {B} rows at these rates (expected "
                               f"{nbytes} bytes, got {state.numel()})")
        max_chunk = lib.nws_resample_stream_max_chunk(sr_in, sr_out)
        if n < 1 and not final:
            raise RuntimeError("resample_stream_step: empty chunk (only a final step may carry no samples)")
        if n > max_chunk:
            raise RuntimeError(f"resample_stream_step: a step takes at most {max_chunk} samples at these rates, got {n}")
        max_out = lib.nws_resample_stream_max_out(n, sr_in, sr_out, 1 if final else 0)
        if out.dim() != 2 or out.shape[0] != B or not max_out <= out.shape[1] < 2 ** 31:
            raise RuntimeError(f"resample_stream_step: out: expected ({B}, >= {max_out}) for a {'final ' if final else ''}step of {n} "
                               f"samples, got {tuple(out.shape)}")
        with torch.cuda.device(chunk.device):
            check(lib.nws_resample_stream_step(ptr(state), state.numel(), ptr(chunk) if n > 0 else None, B, n, sr_in, sr_out,
                                               ptr(bank), 1 if final else 0, ptr(out), out.shape[1], _stream(chunk.device)),
                  "nws_resample_stream_step")

    # ---- note player (csrc/note_control.hip): the launches in front of and behind a slot stream's hop --------------------------
    @staticmethod
    def _note_player(params):
        """the op's `params` tensor (16 float64 values on the CPU, _lib.NOTE_PARAMS) as the ctypes struct"""
        if not (isinstance(params, torch.Tensor) and params.device.type == "cpu" and params.dtype == torch.float64
                and params.is_contiguous() and params.numel() == 16):
            raise RuntimeError("params: expected a CPU float64 tensor of 16 values [attack, decay, release, vib_delay, vib_ramp, drop, "
                               "silence, peak_lo, peak_hi, vib_rate, vib_depth, sample_rate, mean0, std0, mean1, std1]")
        p = params.tolist()
        for v in p[:5]:
            if not (-1e9 <= v <= 1e9 and v == int(v)):
                raise RuntimeError(f"params: attack, decay, release, vib_delay and vib_ramp are whole frames, got {v}")
        P = _lib.NwsNotePlayer()
        P.attack, P.decay, P.release, P.vib_delay, P.vib_ramp = (int(v) for v in p[:5])
        P.drop, P.silence, P.peak_lo, P.peak_hi = p[5:9]
        P.vib_rate, P.vib_depth, P.sample_rate = p[9:12]
        P.mean[0], P.std[0], P.mean[1], P.std[1] = p[12:16]
        return P

    @staticmethod
    def _note_state_bytes(op, B):
        nbytes = _lib.lib().nws_note_control_state_bytes(B) if 1 <= B <= 65535 else 0
        if nbytes == 0:
            raise RuntimeError(f"{op}: unsupported slot count {B}: 1 <= B <= 65535")
        return nbytes

    def note_control_reset(self, state, B):
        _check_state(state)
        nbytes = self._note_state_bytes("note_control_reset", B)
        if state.numel() < nbytes:
            raise RuntimeError(f"note_control_reset: state blob too small (expected {nbytes} bytes for B = {B}, got {state.numel()})")
        with torch.cuda.device(state.device):
            check(_lib.lib().nws_note_control_reset(ptr(state), state.numel(), B, _stream(state.device)), "nws_note_control_reset")

    def note_control(self, params, events, notes, state, f0, control):
        P = self._note_player(params)
        _check_dev("f0", f0)
        _check_dev("control", control, f0, "f0")
        _check_state(state, f0)
        for name, t in (("events", events), ("notes", notes)):
            if not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous() or t.device != f0.device:
                raise RuntimeError(f"{name}: expected a contiguous Int tensor on {f0.device}, got {t.dtype} on {t.device}")
        if f0.dim() != 2 or f0.shape[0] < 1:
            raise RuntimeError(f"note_control: expected f0 (B, K), got {tuple(f0.shape)}")
        B, K = f0.shape
        if not 1 <= K <= 16:
            raise RuntimeError(f"note_control: a hop has 1 .. 16 frames, got {K}")
        if tuple(control.shape) != (B, 2, K):
            raise RuntimeError(f"note_control: expected control ({B}, 2, {K}), got {tuple(control.shape)}")
        if events.numel() != B:
            raise RuntimeError(f"note_control: expected {B} event words, got {events.numel()}")
        if tuple(notes.shape) != (B, 4):
            raise RuntimeError(f"note_control: expected the note table as int32 ({B}, 4) [pitch bits, velocity bits, j_off, 0], got "
                               f"{tuple(notes.shape)}")
        if P.release < 1 or P.vib_ramp < 1:
            raise RuntimeError("note_control: release and vib_ramp are at least one frame")
        nbytes = self._note_state_bytes("note_control", B)
        if state.numel() < nbytes:
            raise RuntimeError(f"note_control: state blob too small (expected {nbytes} bytes for B = {B}, got {state.numel()})")
        with torch.cuda.device(f0.device):
            check(_lib.lib().nws_note_control(C.byref(P), ptr(events), ptr(notes), ptr(state), state.numel(), B, K, ptr(f0),
                                              ptr(control), _stream(f0.device)), "nws_note_control")

    def voice_mix(self, o, gain, out):
        _check_dev("o", o)
        _check_dev("gain", gain, o, "o")
        _check_dev("out", out, o, "o")
        if o.dim() != 2 or o.shape[0] < 1 or not 1 <= o.shape[1] < 2 ** 31:
            raise RuntimeError(f"voice_mix: expected o (B, N), got {tuple(o.shape)}")
        B, N = o.shape
        if B > 65535:
            raise RuntimeError(f"voice_mix: unsupported slot count {B}: 1 <= B <= 65535")
        if gain.dim() != 2 or gain.shape[0] != B or gain.shape[1] not in (1, 2):
            raise RuntimeError(f"voice_mix: expected gain ({B}, 1 or 2), got {tuple(gain.shape)}")
        Cn = gain.shape[1]
        if tuple(out.shape) != (Cn, N):
            raise RuntimeError(f"voice_mix: expected out ({Cn}, {N}), got {tuple(out.shape)}")
        with torch.cuda.device(o.device):
            check(_lib.lib().nws_voice_mix(ptr(o), ptr(gain), B, N, Cn, ptr(out), _stream(o.device)), "nws_voice_mix")

    # ---- MFCC feature (csrc/mfcc.hip) --------------------------------------------------------------------------------------
    def mfcc_table(self, sample_rate, n_fft, n_mfcc, n_mels):
        words = _mfcc_dims(sample_rate, n_fft, n_mfcc, n_mels)[7]
        table = torch.empty(words, dtype=torch.float32)
        check(_lib.lib().nws_mfcc_table(sample_rate, n_fft, n_mfcc, n_mels, table.data_ptr()), "nws_mfcc_table")
        return table

    def mfcc(self, audio, dft, table, sample_rate, n_fft, hop, n_mfcc, n_mels):
        words = _mfcc_dims(sample_rate, n_fft, n_mfcc, n_mels)[7]
        for name, t in (("dft", dft), ("table", table)):
            if not t.is_cuda or t.dtype != torch.float32 or t.device != audio.device:
                raise RuntimeError(f"mfcc: {name}: expected a float32 tensor on the audio's device, got {t.dtype} on {t.device}")
        if table.numel() != words:
            raise RuntimeError(f"mfcc: table does not belong to this configuration (expected {words} words of mfcc_table, got "
                               f"{table.numel()})")
        B, N = audio.shape
        L = _lib.lib()
        if dft.numel() * 4 != L.nws_loudness_dft_bytes(n_fft):
            raise RuntimeError(f"mfcc: dft does not belong to n_fft = {n_fft}")
        nbytes = L.nws_mfcc_workspace_bytes(B, N, n_fft, hop, n_mels) if 1 <= B <= 65535 else 0
        if nbytes == 0 or N <= n_fft // 2:
            raise RuntimeError(f"mfcc: unsupported size (B {B}, N {N}, n_fft {n_fft}, hop_length {hop}): 1 <= hop <= n_fft, "
                               "31 hop + n_fft samples must fit 160 KB of LDS, N > n_fft / 2, B <= 65535")
        with torch.cuda.device(audio.device):
            ws = _new(audio, nbytes, dtype=torch.uint8)
            out = _new(audio, B, n_mfcc, L.nws_loudness_frames(N, hop))
            check(L.nws_mfcc(ptr(audio), B, N, sample_rate, n_fft, hop, n_mfcc, n_mels, ptr(dft), ptr(table), ptr(out), ptr(ws),
                             nbytes, _stream(audio.device)), "nws_mfcc")
        return out

    # ---- multi-resolution STFT loss (csrc/stft_loss.hip) -------------------------------------------------------------------
    def stft_loss_dft(self, n_fft, win_length):
        L = _lib.lib()
        nbytes = L.nws_stft_loss_dft_bytes(n_fft, win_length) if max(abs(n_fft), abs(win_length)) < 2 ** 31 else 0
        if nbytes == 0:
            raise RuntimeError(f"stft_loss: unsupported resolution (n_fft {n_fft}, win_length {win_length}): n_fft a power of two "
                               "in [64, 2048], 1 <= win_length <= n_fft")
        dev = torch.device("cuda", torch.cuda.current_device())
        dft = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
        check(L.nws_stft_loss_dft_matrix(n_fft, win_length, ptr(dft), _stream(dev)), "nws_stft_loss_dft_matrix")
        return dft

    @staticmethod
    def _stft_sizes(op, x, y, dfts, n_ffts, hops, win_lengths):
        """the argument checks stft_loss and stft_loss_grad share -> B, N, R and the three int arrays (None where a size does not
        fit an int: the caller's workspace query then reports the size as unsupported)"""
        for name, t in (("x", x), ("y", y)):
            if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous():
                raise RuntimeError(f"{op}: {name}: expected a contiguous (B, N) float32 CUDA tensor (there is no CPU fallback), "
                                   f"got {tuple(t.shape)} {t.dtype} on {t.device}")
        if x.shape != y.shape or x.device != y.device:
            raise RuntimeError(f"{op}: x {tuple(x.shape)} on {x.device} and y {tuple(y.shape)} on {y.device} must agree")
        R = len(n_ffts)
        if not (1 <= R <= 8 and len(hops) == R and len(win_lengths) == R and len(dfts) == R):
            raise RuntimeError(f"{op}: 1 to 8 resolutions, one n_fft, hop, win_length and operand each (got {R}, {len(hops)}, "
                               f"{len(win_lengths)}, {len(dfts)})")
        B, N = x.shape
        L = _lib.lib()
        ints = [int(v) for v in (*n_ffts, *hops, *win_lengths)]
        ok = all(abs(v) < 2 ** 31 for v in ints) and 1 <= B and N < 2 ** 31
        nf, hp, wl = ((C.c_int * R)(*ints[i * R:(i + 1) * R]) for i in range(3)) if ok else (None, None, None)
        for r in range(R if ok else 0):
            d = dfts[r]
            if not d.is_cuda or d.dtype != torch.float32 or d.device != x.device or not d.is_contiguous():
                raise RuntimeError(f"{op}: dfts[{r}]: expected a float32 tensor on x's device, got {d.dtype} on {d.device}")
            nbytes = L.nws_stft_loss_dft_bytes(nf[r], wl[r])
            if nbytes == 0 or d.numel() * 4 != nbytes:
                raise RuntimeError(f"{op}: dfts[{r}] does not belong to n_fft = {nf[r]}, win_length = {wl[r]} (n_fft: a power of "
                                   "two in [64, 2048], 1 <= win_length <= n_fft)")
        return B, N, R, nf, hp, wl

    @staticmethod
    def _stft_unsupported(op, B, N, n_ffts, hops):
        return RuntimeError(f"{op}: unsupported size (B {B}, N {N}, n_ffts {list(n_ffts)}, hops {list(hops)}): N > n_fft / 2 "
                            "(reflect padding), hop >= 1, the two signal tiles of 31 hop + n_fft samples must fit 160 KB of LDS "
                            "(n_fft 2048: hop <= 589), B <= 65535")

    def stft_loss(self, x, y, dfts, n_ffts, hops, win_lengths, w_sc, w_log_mag, w_lin_mag, eps):
        B, N, R, nf, hp, wl = self._stft_sizes("stft_loss", x, y, dfts, n_ffts, hops, win_lengths)
        L = _lib.lib()
        nbytes = L.nws_stft_loss_workspace_bytes(B, N, R, nf, hp) if nf is not None else 0
        if nbytes == 0:
            raise self._stft_unsupported("stft_loss", B, N, n_ffts, hops)
        with torch.cuda.device(x.device):
            ws = _new(x, nbytes, dtype=torch.uint8)
            out = _new(x, 1 + 3 * R)
            check(L.nws_stft_loss(ptr(x), ptr(y), B, N, R, nf, hp, wl, _ptrs(dfts), w_sc, w_log_mag, w_lin_mag, eps, ptr(out), ptr(ws),
                                  nbytes, _stream(x.device)), "nws_stft_loss")
        return [out[0], out[1:].view(R, 3)]

    def stft_loss_grad(self, x, y, dfts, n_ffts, hops, win_lengths, w_sc, w_log_mag, w_lin_mag, eps):
        """dL/dx of stft_loss (csrc/stft_grad.hip): (B, N)"""
        B, N, R, nf, hp, wl = self._stft_sizes("stft_loss_grad", x, y, dfts, n_ffts, hops, win_lengths)
        L = _lib.lib()
        nbytes = L.nws_stft_grad_workspace_bytes(B, N, R, nf, hp, wl) if nf is not None else 0
        if nbytes == 0:
            raise self._stft_unsupported("stft_loss_grad", B, N, n_ffts, hops)
        with torch.cuda.device(x.device):
            ws = _new(x, nbytes, dtype=torch.uint8)
            grad = _new(x, B, N)
            check(L.nws_stft_grad(ptr(x), ptr(y), B, N, R, nf, hp, wl, _ptrs(dfts), w_sc, w_log_mag, w_lin_mag, eps, ptr(grad), ptr(ws),
                                  nbytes, _stream(x.device)), "nws_stft_grad")
        return grad

    # ---- runtime-size path (csrc/generic.hip) ----------------------------------------------------------------------------
    def forward_generic(self, gdesc, f0, control, phase_u, rand_phase, noise, plan, reverb_tables, reverb_spectrum,
                        reverb_workspace, workspace, sample_rate):
        B, Cc, T = control.shape
        g = _struct(gdesc, NwsGenericModel)
        p = _plan(plan)
        with torch.cuda.device(f0.device):
            out = _new(f0, B, T * g.hop)
            check(_lib.lib().nws_forward_generic(C.byref(g), ptr(f0), ptr(control), B, Cc, T, sample_rate, ptr(phase_u),
                                                 ptr(rand_phase), ptr(noise), _ref(p), ptr(reverb_tables), ptr(reverb_spectrum),
                                                 ptr(reverb_workspace) if p is not None else None,
                                                 reverb_workspace.numel() if p is not None else 0, ptr(out), ptr(workspace),
                                                 workspace.numel(), _stream(f0.device)), "nws_forward_generic")
        return out

    def g_gru(self, w_ih, w_hh, b_ih, b_hh, control, h0):
        B, Ct, T = control.shape
        H, Cin = w_hh.shape[1], w_ih.shape[1]
        L = _lib.lib()
        with torch.cuda.device(control.device):
            out = _new(control, B, T, H)
            hT = _new(control, B, H)
            nb = L.nws_g_gru_workspace_bytes(H)
            ws = _new(control, nb, dtype=torch.uint8)
            check(L.nws_g_gru(ptr(w_ih), ptr(w_hh), ptr(b_ih), ptr(b_hh), ptr(control), B, Ct, Cin, H, T, ptr(h0), ptr(out), ptr(hT),
                              ptr(ws), nb, _stream(control.device)), "nws_g_gru")
        return out, hT

    def g_oscillator(self, f0_up, phase_u, rand_phase, sample_rate):
        B, N = f0_up.shape
        K = phase_u.numel()
        with torch.cuda.device(f0_up.device):
            st = _stream(f0_up.device)
            phase = torch.empty_like(f0_up)
            out = _new(f0_up, B, K, N)
            check(_lib.lib().nws_g_phase(None, ptr(f0_up), B, N, 1, sample_rate, None, ptr(phase), st), "nws_g_phase")
            check(_lib.lib().nws_g_oscillator(ptr(f0_up), ptr(phase), ptr(phase_u), ptr(rand_phase), K, B, N, sample_rate, ptr(out),
                                              st), "nws_g_oscillator")
        return out

    def g_conv1x1(self, x, weight, bias):
        B, Cin, N = x.shape
        Cout = weight.shape[0]
        with torch.cuda.device(x.device):
            y = _new(x, B, Cout, N)
            check(_lib.lib().nws_g_conv1x1(ptr(x), ptr(weight), ptr(bias), B, Cin, Cout, N, ptr(y), _stream(x.device)),
                  "nws_g_conv1x1")
        return y

    def g_upsample(self, x, hop):
        T = x.shape[-1]
        with torch.cuda.device(x.device):
            y = _new(x, *x.shape[:-1], T * hop)
            check(_lib.lib().nws_g_upsample(ptr(x), x.numel() // T, T, hop, ptr(y), _stream(x.device)), "nws_g_upsample")
        return y

    def g_shaper_apply(self, sdesc, x):
        with torch.cuda.device(x.device):
            y = torch.empty_like(x)
            check(_lib.lib().nws_g_shaper_apply(C.byref(_struct(sdesc, NwsShaperDesc)), ptr(x), x.shape[0] * x.shape[1], x.shape[2],
                                                ptr(y), _stream(x.device)), "nws_g_shaper_apply")
        return y

    def g_shaper_table(self, sdesc, like, size, tmin, tmax):
        d = _struct(sdesc, NwsShaperDesc)
        with torch.cuda.device(like.device):
            table = _new(like, d.n_shapers, size)
            check(_lib.lib().nws_g_shaper_table(C.byref(d), size, tmin, tmax, ptr(table), _stream(like.device)), "nws_g_shaper_table")
        return table

    def g_newt_apply(self, sdesc, exciter, film, mix_w, mix_b):
        B, S, N = exciter.shape
        T = film.shape[2]
        O = mix_w.numel() // S
        with torch.cuda.device(exciter.device):
            st = _stream(exciter.device)
            shaped = torch.empty_like(exciter)
            out = _new(exciter, B, O, N)
            check(_lib.lib().nws_g_film_shaper(C.byref(_struct(sdesc, NwsShaperDesc)), ptr(exciter), ptr(film), B, T, N // T,
                                               ptr(shaped), st), "nws_g_film_shaper")
            check(_lib.lib().nws_g_conv1x1(ptr(shaped), ptr(mix_w), ptr(mix_b), B, S, O, N, ptr(out), st), "nws_g_conv1x1")
        return out

    def g_newt_grad(self, sdesc, exciter, film, grad_out, mix_w, mix_b, want_exciter, want_params):
        d = _struct(sdesc, NwsShaperDesc)
        B, _, N = exciter.shape
        S, W, D = d.n_shapers, d.width, d.depth
        T = film.shape[2]
        if exciter.shape[1] != S or tuple(film.shape) != (B, 4 * S, T) or N != T * HOP:
            raise RuntimeError(f"NEWT: exciter {tuple(exciter.shape)} and FiLM parameters {tuple(film.shape)} disagree "
                               f"({S} shapers, hop {HOP})")
        if B < 1 or T < 1:
            raise RuntimeError("g_newt_grad: need at least one utterance and one frame")
        if grad_out.numel() != B * N or grad_out.shape[0] != B:
            raise RuntimeError(f"g_newt_grad: grad_out {tuple(grad_out.shape)} is not ({B}, 1, {N})")
        if d.lut:
            raise RuntimeError("g_newt_grad: the lookup table has no backward")
        if mix_w.numel() != S or mix_b.numel() != 1:
            raise RuntimeError(f"g_newt_grad: one output channel only: mixer weight {tuple(mix_w.shape)} / bias {tuple(mix_b.shape)} "
                               f"for {S} shapers")
        L = _lib.lib()
        nbytes = L.nws_g_newt_grad_workspace_bytes(C.byref(d), B, T, 1 if want_params else 0) if max(B, T) < 2 ** 30 else 0
        if nbytes == 0:
            raise RuntimeError(f"g_newt_grad: unsupported size ({S} shapers of width {W} and depth {D}, B {B}, T {T}): at most 64 "
                               "shapers of width 16 and depth 4, T <= 65535, B T <= 2^28")
        with torch.cuda.device(exciter.device):
            out = [_new(exciter, B, 4 * S, T)]
            ge = torch.empty_like(exciter) if want_exciter else None
            if want_exciter:
                out.append(ge)
            gp = []
            if want_params:
                gp = [_new(exciter, *sh) for sh in _lib.g_newt_grad_shapes(S, W, D)]
                out += gp
            ws = _new(exciter, nbytes, dtype=torch.uint8)
            check(L.nws_g_newt_grad(C.byref(d), ptr(mix_w), ptr(mix_b), ptr(exciter), ptr(film), ptr(grad_out), B, T, HOP, ptr(ge),
                                    ptr(out[0]), _ptrs(gp) if want_params else None, ptr(ws), nbytes, _stream(exciter.device)),
                  "nws_g_newt_grad")
        return out

    def g_fir_noise(self, H, window, noise, hop):
        B, _, T = H.shape
        Lf = window.numel()
        with torch.cuda.device(H.device):
            st = _stream(H.device)
            fir = _new(H, B, T, Lf)
            out = _new(H, B, T * hop)
            check(_lib.lib().nws_g_fir_design(ptr(H), ptr(window), Lf, B, T, ptr(fir), st), "nws_g_fir_design")
            check(_lib.lib().nws_g_fir_noise(ptr(fir), ptr(noise), Lf, hop, B, T, None, 0, ptr(out), st), "nws_g_fir_noise")
        return out

    def g_reverb_direct(self, x, ir):
        with torch.cuda.device(x.device):
            y = torch.empty_like(x)
            check(_lib.lib().nws_g_reverb_direct(ptr(x), ptr(ir), ir.numel(), x.shape[0], x.shape[1], ptr(y), _stream(x.device)),
                  "nws_g_reverb_direct")
        return y

    # ---- stateful streaming step (csrc/stream.hip) -----------------------------------------------------------------------
    def stream_step(self, wdesc, fir_design, plan, reverb_tables, reverb_spectrum, state, max_frames, f0, control, first, final,
                    frames_seen, nz_prev_start, sample_rate, phase_u, rand_phase, noise_new, noise_all, ir, out, pre_out):
        B, K = f0.shape
        with torch.cuda.device(f0.device):
            check(_lib.lib().nws_stream_step(
                C.byref(_struct(wdesc, NwsWeights)), ptr(fir_design), _ref(_plan(plan)), ptr(reverb_tables), ptr(reverb_spectrum),
                ptr(state), state.numel(), B, max_frames, ptr(f0), ptr(control), control.shape[1], K, int(first), int(final),
                frames_seen, nz_prev_start, sample_rate, ptr(phase_u), ptr(rand_phase), ptr(noise_new), ptr(noise_all),
                noise_all.numel() if noise_all is not None else 0, ptr(ir), ir.numel(), ptr(out), ptr(pre_out),
                _stream(f0.device)), "nws_stream_step")

    def stream_step_slots(self, wdesc, fir_design, state, max_frames, f0, control, frames_seen, nz_prev_start, sample_rate, phase_u,
                          rand_phase, noise_new, noise_all, ir, events, out, pre_out):
        B, K = f0.shape
        with torch.cuda.device(f0.device):
            check(_lib.lib().nws_stream_step_slots(
                C.byref(_struct(wdesc, NwsWeights)), ptr(fir_design), ptr(state), state.numel(), B, max_frames, ptr(f0),
                ptr(control), control.shape[1], K, frames_seen, nz_prev_start, sample_rate, ptr(phase_u), ptr(rand_phase),
                ptr(noise_new), ptr(noise_all), noise_all.numel() if noise_all is not None else 0, ptr(ir), ir.numel(),
                ptr(events), ptr(out), ptr(pre_out), _stream(f0.device)), "nws_stream_step_slots")

    def g_stream_step(self, gdesc, plan, reverb_tables, reverb_spectrum, state, max_frames, f0, control, first, final, frames_seen,
                      nz_prev_start, sample_rate, phase_u, rand_phase, noise_new, noise_all, out, pre_out):
        B, K = f0.shape
        with torch.cuda.device(f0.device):
            check(_lib.lib().nws_g_stream_step(
                C.byref(_struct(gdesc, NwsGenericModel)), _ref(_plan(plan)), ptr(reverb_tables), ptr(reverb_spectrum), ptr(state),
                state.numel(), B, max_frames, ptr(f0), ptr(control), control.shape[1], K, int(first), int(final), frames_seen,
                nz_prev_start, sample_rate, ptr(phase_u), ptr(rand_phase), ptr(noise_new), ptr(noise_all),
                noise_all.numel() if noise_all is not None else 0, ptr(out), ptr(pre_out), _stream(f0.device)), "nws_g_stream_step")

    def g_stream_step_slots(self, gdesc, state, max_frames, f0, control, frames_seen, nz_prev_start, sample_rate, phase_u, rand_phase,
                            noise_new, noise_all, events, out, pre_out):
        B, K = f0.shape
        with torch.cuda.device(f0.device):
            check(_lib.lib().nws_g_stream_step_slots(
                C.byref(_struct(gdesc, NwsGenericModel)), ptr(state), state.numel(), B, max_frames, ptr(f0), ptr(control),
                control.shape[1], K, frames_seen, nz_prev_start, sample_rate, ptr(phase_u), ptr(rand_phase), ptr(noise_new),
                ptr(noise_all), noise_all.numel() if noise_all is not None else 0, ptr(events), ptr(out), ptr(pre_out),
                _stream(f0.device)), "nws_g_stream_step_slots")
