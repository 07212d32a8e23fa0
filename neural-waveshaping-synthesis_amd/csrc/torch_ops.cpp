// torch.ops.newt_hip.* - the PyTorch-ROCm custom-op layer over the C-ABI of include/nws_hip.h (last row).
//
// The reference's hot path is a chain of ATen ops dispatched from NeuralWaveshaping.forward (models/neural_waveshaping.py:74-90);
// this layer gives the HIP replacement the same standing: dispatcher-visible operators that take contiguous fp32 tensors,
// check shapes / dtypes / devices with TORCH_CHECK (-> RuntimeError, the reference's error convention), enqueue the
// hand-written kernels on torch's CURRENT stream of the tensors' device and return fresh tensors.  Nothing is computed
// here: every op is one call of an extern "C" launcher of libnws_hip.so.
//
// Weights travel as `wdesc`: a CPU uint8 tensor holding one NwsWeights struct (device pointers into the module's own
// parameters and derived tables; built once per weights version by engine.py, which keeps those tensors alive).
// Host-only translation unit: compiled with g++ against the torch headers, linked to libnws_hip.so (build.py).
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/library.h>

#include <algorithm>
#include <cstdlib>
#include <tuple>
#include <vector>

#include "../../include/nws_hip.h"
#include "../../include/nws_hip_debug.h"

namespace {

using at::Tensor;
using OptTensor = c10::optional<at::Tensor>;

const NwsWeights* weights_of(const Tensor& wdesc) {
  TORCH_CHECK(wdesc.device().is_cpu() && wdesc.scalar_type() == at::kByte && wdesc.is_contiguous() &&
                  (size_t)wdesc.numel() == sizeof(NwsWeights),
              "wdesc: expected a contiguous CPU uint8 tensor of ", sizeof(NwsWeights), " bytes (one NwsWeights struct), got ",
              wdesc.sizes(), " ", wdesc.scalar_type(), " on ", wdesc.device());
  return reinterpret_cast<const NwsWeights*>(wdesc.data_ptr());
}

void check_dev(const Tensor& t, const char* name, at::ScalarType st = at::kFloat) {
  TORCH_CHECK(t.is_cuda(), name, " lives on ", t.device(),
              ": the NEWT forward path only runs as HIP kernels on an AMD GPU (there is no CPU fallback)");
  TORCH_CHECK(t.scalar_type() == st, name, ": expected ", st, ", got ", t.scalar_type());
  TORCH_CHECK(t.is_contiguous(), name, ": expected a contiguous tensor");
}

void check_same_device(const Tensor& a, const char* an, const Tensor& b, const char* bn) {
  TORCH_CHECK(a.device() == b.device(), an, " is on ", a.device(), " but ", bn, " is on ", b.device(),
              ": all tensors of one call must live on the same GPU");
}

void nws_check(int rc, const char* what) {
  TORCH_CHECK(rc == NWS_OK, what, " failed (", rc, "): ", nws_error_string(rc));
}

const float* fptr(const OptTensor& t) { return t.has_value() ? t->data_ptr<float>() : nullptr; }

// device guard + torch's current stream on that device: kernels go where the ATen ops they replace would have gone
struct Launch {
  c10::hip::HIPGuardMasqueradingAsCUDA guard;
  void* stream;
  explicit Launch(const Tensor& t)
      : guard(t.device()), stream(c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream()) {}
};

NwsReverbPlan plan_of(const Tensor& plan) {
  TORCH_CHECK(plan.device().is_cpu() && plan.scalar_type() == at::kInt && plan.is_contiguous() && plan.numel() == 8,
              "plan: expected a CPU int32 tensor [L, N1, N2, Lc, hist, nblk, 0, 0] (the NwsReverbPlan of nws_reverb_plan)");
  const int32_t* p = plan.data_ptr<int32_t>();
  return NwsReverbPlan{p[0], p[1], p[2], p[3], p[4], p[5], {p[6], p[7]}};
}

// the spectrum / table tensors must be the ones built for THIS plan: the kernels index them by plan.L / N1 / N2 (a tensor made
// for another L, or for an older layout of the spectrum buffer, would be read out of bounds)
void check_reverb_buffers(const NwsReverbPlan& plan, const Tensor& tables, const Tensor& spectrum) {
  TORCH_CHECK(plan.L > 0 && plan.N1 > 0 && plan.N2 > 0 && (int64_t)plan.N1 * plan.N2 == plan.L, "plan: inconsistent [L, N1, N2] = [",
              plan.L, ", ", plan.N1, ", ", plan.N2, "]");
  TORCH_CHECK((size_t)tables.numel() * tables.element_size() == nws_reverb_table_bytes(&plan), "reverb_tables: ",
              (size_t)tables.numel() * tables.element_size(), " bytes, the plan (L = ", plan.L, ") needs ", nws_reverb_table_bytes(&plan));
  TORCH_CHECK((size_t)spectrum.numel() * spectrum.element_size() == nws_reverb_spectrum_bytes(&plan), "reverb_spectrum: ",
              (size_t)spectrum.numel() * spectrum.element_size(), " bytes, the plan (L = ", plan.L, ") needs ",
              nws_reverb_spectrum_bytes(&plan), " (Sre | Sim | ir_)");
}

struct Aux {
  NwsReverbPlan plan;
  NwsForwardAux aux;
  Aux(const Tensor& fir_design, const Tensor& plan_t, const Tensor& tables, const Tensor& spectrum) : plan(plan_of(plan_t)) {
    check_dev(fir_design, "fir_design");
    check_dev(tables, "reverb_tables");
    check_dev(spectrum, "reverb_spectrum");
    TORCH_CHECK(fir_design.numel() == NWS_FIR_LEN * 132, "fir_design: expected (256, 132)");
    check_reverb_buffers(plan, tables, spectrum);
    aux.fir_design = fir_design.data_ptr<float>();
    aux.plan = &plan;
    aux.reverb_tables = tables.data_ptr();
    aux.reverb_spectrum = spectrum.data_ptr();
  }
};

void check_inputs(const Tensor& f0, const Tensor& control, int64_t& B, int64_t& C, int64_t& T) {
  check_dev(f0, "f0");
  check_dev(control, "control");
  check_same_device(f0, "f0", control, "control");
  TORCH_CHECK(f0.dim() == 3 && f0.size(1) == 1, "f0: expected (B, 1, T), got ", f0.sizes());
  TORCH_CHECK(control.dim() == 3 && control.size(1) >= 2, "control: expected (B, C>=2, T), got ", control.sizes());
  B = f0.size(0);
  T = f0.size(2);
  C = control.size(1);
  TORCH_CHECK(control.size(0) == B && control.size(2) == T, "f0 ", f0.sizes(), " and control ", control.sizes(),
              " disagree on batch / frames");
  TORCH_CHECK(T >= 2, "need at least 2 control frames (reflect padding of the noise STFT, generators.py:31)");
}

void check_draws(const Tensor& phase_u, const Tensor& rand_phase, const Tensor& noise, int64_t T, const Tensor& like) {
  check_dev(phase_u, "phase_u");
  check_dev(rand_phase, "rand_phase");
  check_dev(noise, "noise");
  check_same_device(like, "f0", phase_u, "phase_u");
  check_same_device(like, "f0", noise, "noise");
  check_same_device(like, "f0", rand_phase, "osc.rand_phase");
  TORCH_CHECK(phase_u.numel() == NWS_N_HARMONICS, "phase_u: expected 101 elements, got ", phase_u.sizes());
  TORCH_CHECK(rand_phase.numel() == NWS_N_HARMONICS, "rand_phase: expected 101 elements, got ", rand_phase.sizes());
  TORCH_CHECK(noise.numel() == NWS_HOP * T - 1, "noise: expected ", NWS_HOP * T - 1, " elements, got ", noise.sizes());
}

// what forward_audio, forward_audio_pre and forward_audio_blocks check before anything else: f0's shape, the two draws and the
// workspace, then (Aux) the model's tables as the launchers' NwsForwardAux
struct AudioShape {
  int64_t B, T;
  AudioShape(const Tensor& f0, const Tensor& phase_u, const Tensor& rand_phase, const Tensor& noise, const Tensor& workspace) {
    check_dev(f0, "f0");
    TORCH_CHECK(f0.dim() == 3 && f0.size(1) == 1 && f0.size(2) >= 2, "f0: expected (B, 1, T>=2), got ", f0.sizes());
    B = f0.size(0);
    T = f0.size(2);
    check_draws(phase_u, rand_phase, noise, T, f0);
    check_dev(workspace, "workspace", at::kByte);
    check_same_device(f0, "f0", workspace, "workspace");
  }
};

struct AudioArgs : AudioShape, Aux {      // (bases are built in this order: the checks above run first, as they always did)
  AudioArgs(const Tensor& f0, const Tensor& phase_u, const Tensor& rand_phase, const Tensor& noise, const Tensor& fir_design,
            const Tensor& plan_t, const Tensor& tables, const Tensor& spectrum, const Tensor& workspace)
      : AudioShape(f0, phase_u, rand_phase, noise, workspace), Aux(fir_design, plan_t, tables, spectrum) {}
};

// ---- whole forward: models/neural_waveshaping.py:74-90 ---------------------------------------------------------------
Tensor forward(const Tensor& wdesc, const Tensor& f0, const Tensor& control, const Tensor& phase_u, const Tensor& rand_phase,
               const Tensor& noise, const Tensor& fir_design, const Tensor& plan, const Tensor& reverb_tables,
               const Tensor& reverb_spectrum, Tensor& workspace, double sample_rate) {
  const NwsWeights* w = weights_of(wdesc);
  int64_t B, C, T;
  check_inputs(f0, control, B, C, T);
  check_draws(phase_u, rand_phase, noise, T, f0);
  check_dev(workspace, "workspace", at::kByte);
  check_same_device(f0, "f0", workspace, "workspace");
  Aux a(fir_design, plan, reverb_tables, reverb_spectrum);
  check_same_device(f0, "f0", fir_design, "the model's tables");
  Launch L(f0);
  Tensor out = at::empty({B, T * NWS_HOP}, f0.options());
  nws_check(nws_forward(w, &a.aux, f0.data_ptr<float>(), control.data_ptr<float>(), (int)B, (int)C, (int)T, (float)sample_rate,
                        phase_u.data_ptr<float>(), rand_phase.data_ptr<float>(), noise.data_ptr<float>(), out.data_ptr<float>(),
                        workspace.data_ptr(), (size_t)workspace.numel(), L.stream),
            "nws_forward");
  return out;
}

void forward_control(const Tensor& wdesc, const Tensor& f0, const Tensor& control, Tensor& workspace, bool batched_gru) {
  const NwsWeights* w = weights_of(wdesc);
  int64_t B, C, T;
  check_inputs(f0, control, B, C, T);
  check_dev(workspace, "workspace", at::kByte);
  check_same_device(f0, "f0", workspace, "workspace");
  Launch L(f0);
  nws_check(nws_forward_control(w, f0.data_ptr<float>(), control.data_ptr<float>(), (int)B, (int)C, (int)T, batched_gru ? 1 : 0,
                                workspace.data_ptr(), (size_t)workspace.numel(), L.stream),
            "nws_forward_control");
}

Tensor forward_audio(const Tensor& wdesc, const Tensor& f0, const Tensor& phase_u, const Tensor& rand_phase, const Tensor& noise,
                     const Tensor& fir_design, const Tensor& plan, const Tensor& reverb_tables, const Tensor& reverb_spectrum,
                     Tensor& workspace, double sample_rate, const OptTensor& out_opt, int64_t wait_event, int64_t record_event) {
  const NwsWeights* w = weights_of(wdesc);
  AudioArgs a(f0, phase_u, rand_phase, noise, fir_design, plan, reverb_tables, reverb_spectrum, workspace);
  const int64_t B = a.B, T = a.T;
  Launch L(f0);
  Tensor out;
  if (out_opt.has_value()) {
    out = *out_opt;
    check_dev(out, "out");
    check_same_device(f0, "f0", out, "out");
    TORCH_CHECK(out.dim() == 2 && out.size(0) == B && out.size(1) == T * NWS_HOP, "out: expected (", B, ", ", T * NWS_HOP, ")");
  } else {
    out = at::empty({B, T * NWS_HOP}, f0.options());
  }
  // wait_event / record_event: raw hipEvent_t handles (torch.cuda.Event.cuda_event) or 0, see nws_forward_audio_ev
  nws_check(nws_forward_audio_ev(w, &a.aux, f0.data_ptr<float>(), (int)B, (int)T, (float)sample_rate, phase_u.data_ptr<float>(),
                                 rand_phase.data_ptr<float>(), noise.data_ptr<float>(), out.data_ptr<float>(), workspace.data_ptr(),
                                 (size_t)workspace.numel(), L.stream, reinterpret_cast<void*>(wait_event),
                                 reinterpret_cast<void*>(record_event)),
            "nws_forward_audio");
  return out;
}

// the audio half in two parts (sub-batch gathers): up to the reverb input; then the reverb of a block of rows
void forward_audio_pre(const Tensor& wdesc, const Tensor& f0, const Tensor& phase_u, const Tensor& rand_phase, const Tensor& noise,
                       const Tensor& fir_design, const Tensor& plan, const Tensor& reverb_tables, const Tensor& reverb_spectrum,
                       Tensor& workspace, double sample_rate) {
  const NwsWeights* w = weights_of(wdesc);
  AudioArgs a(f0, phase_u, rand_phase, noise, fir_design, plan, reverb_tables, reverb_spectrum, workspace);
  const int64_t B = a.B, T = a.T;
  Launch L(f0);
  nws_check(nws_forward_audio_pre(w, &a.aux, f0.data_ptr<float>(), (int)B, (int)T, (float)sample_rate, phase_u.data_ptr<float>(),
                                  rand_phase.data_ptr<float>(), noise.data_ptr<float>(), workspace.data_ptr(),
                                  (size_t)workspace.numel(), L.stream), "nws_forward_audio_pre");
}

void forward_reverb_rows(const Tensor& fir_design, const Tensor& plan, const Tensor& reverb_tables, const Tensor& reverb_spectrum,
                         Tensor& workspace, int64_t T, int64_t row0, int64_t nrows, Tensor& out) {
  check_dev(workspace, "workspace", at::kByte);
  check_dev(out, "out");
  check_same_device(out, "out", workspace, "workspace");
  TORCH_CHECK(out.dim() == 2 && out.size(1) == T * NWS_HOP, "out: expected (B, ", T * NWS_HOP, "), got ", out.sizes());
  TORCH_CHECK(row0 >= 0 && nrows > 0 && row0 + nrows <= out.size(0) && (row0 & 1) == 0, "forward_reverb_rows: bad row block");
  Aux a(fir_design, plan, reverb_tables, reverb_spectrum);
  Launch L(out);
  nws_check(nws_forward_reverb_rows(&a.aux, (int)out.size(0), (int)T, (int)row0, (int)nrows, out.data_ptr<float>(), workspace.data_ptr(),
                                    (size_t)workspace.numel(), L.stream), "nws_forward_reverb_rows");
}

// the same two in one call for a fixed list of row blocks, an event recorded behind each block (sub-batch exchange: one op per step)
void forward_audio_blocks(const Tensor& wdesc, const Tensor& f0, const Tensor& phase_u, const Tensor& rand_phase, const Tensor& noise,
                          const Tensor& fir_design, const Tensor& plan, const Tensor& reverb_tables, const Tensor& reverb_spectrum,
                          Tensor& workspace, double sample_rate, Tensor& out, at::IntArrayRef row0, at::IntArrayRef nrows,
                          at::IntArrayRef events) {
  const NwsWeights* w = weights_of(wdesc);
  AudioArgs a(f0, phase_u, rand_phase, noise, fir_design, plan, reverb_tables, reverb_spectrum, workspace);
  const int64_t B = a.B, T = a.T;
  check_dev(out, "out");
  check_same_device(f0, "f0", out, "out");
  TORCH_CHECK(out.dim() == 2 && out.size(0) == B && out.size(1) == T * NWS_HOP && out.is_contiguous(), "out: expected a contiguous (", B, ", ",
              T * NWS_HOP, "), got ", out.sizes());
  TORCH_CHECK(!row0.empty() && row0.size() == nrows.size() && (events.empty() || events.size() == row0.size()),
              "forward_audio_blocks: row0 / nrows / events must have one entry per block");
  std::vector<int32_t> r0(row0.begin(), row0.end()), nr(nrows.begin(), nrows.end());
  std::vector<void*> ev(events.size());
  for (size_t q = 0; q < events.size(); ++q) ev[q] = reinterpret_cast<void*>(static_cast<uintptr_t>(events[q]));
  Launch L(f0);
  nws_check(nws_forward_audio_blocks(w, &a.aux, f0.data_ptr<float>(), (int)B, (int)T, (float)sample_rate, phase_u.data_ptr<float>(),
                                     rand_phase.data_ptr<float>(), noise.data_ptr<float>(), out.data_ptr<float>(), workspace.data_ptr(),
                                     (size_t)workspace.numel(), L.stream, r0.data(), nr.data(), ev.empty() ? nullptr : ev.data(), (int)r0.size()),
            "nws_forward_audio_blocks");
}

// ---- stages ------------------------------------------------------------------------------------------------------------
// exclusive fp64 prefix sums at 32-sample granularity (torch.cumsum of generators.py:59): f0 (B, T) frames or f0_up (B, 128 T)
Tensor phase_carry(const OptTensor& f0, const OptTensor& f0_up) {
  TORCH_CHECK(f0.has_value() != f0_up.has_value(), "phase_carry: give exactly one of f0 (B, T) and f0_up (B, 128 T)");
  const Tensor& src = f0.has_value() ? *f0 : *f0_up;
  check_dev(src, f0.has_value() ? "f0" : "f0_up");
  TORCH_CHECK(src.dim() == 2, "phase_carry: expected a 2-D tensor, got ", src.sizes());
  const int64_t B = src.size(0);
  TORCH_CHECK(f0.has_value() || src.size(1) % NWS_HOP == 0, "f0_up: the sample count must be a multiple of ", NWS_HOP);
  const int64_t T = f0.has_value() ? src.size(1) : src.size(1) / NWS_HOP;
  Launch L(src);
  Tensor carry = at::empty({B, T * NWS_HOP / 32}, src.options().dtype(at::kDouble));
  nws_check(nws_phase_carry(fptr(f0), fptr(f0_up), (int)B, (int)T, carry.data_ptr<double>(), L.stream), "nws_phase_carry");
  return carry;
}

std::tuple<Tensor, Tensor> exciter_newt(const Tensor& wdesc, const OptTensor& f0, const OptTensor& f0_up, const Tensor& carry,
                                        const Tensor& phase_u, const Tensor& rand_phase, const OptTensor& film,
                                        double sample_rate, bool want_exciter, bool want_newt) {
  const NwsWeights* w = weights_of(wdesc);
  TORCH_CHECK(f0.has_value() != f0_up.has_value(), "exciter_newt: give exactly one of f0 (B, T) and f0_up (B, 128 T)");
  TORCH_CHECK(want_exciter || want_newt, "exciter_newt: nothing to compute");
  const Tensor& src = f0.has_value() ? *f0 : *f0_up;
  check_dev(src, "f0");
  check_dev(carry, "carry", at::kDouble);
  check_dev(phase_u, "phase_u");
  check_dev(rand_phase, "rand_phase");
  check_same_device(src, "f0", carry, "carry");
  check_same_device(src, "f0", phase_u, "phase_u");
  TORCH_CHECK(src.dim() == 2, "exciter_newt: f0 / f0_up must be 2-D, got ", src.sizes());
  const int64_t B = src.size(0);
  const int64_t T = f0.has_value() ? src.size(1) : src.size(1) / NWS_HOP;
  const int64_t N = T * NWS_HOP;
  TORCH_CHECK(f0.has_value() || src.size(1) == N, "f0_up: the sample count must be a multiple of ", NWS_HOP);
  TORCH_CHECK(carry.numel() == B * (N / 32), "carry: expected (", B, ", ", N / 32, "), got ", carry.sizes());
  TORCH_CHECK(phase_u.numel() == NWS_N_HARMONICS && rand_phase.numel() == NWS_N_HARMONICS, "phase_u / rand_phase: 101 elements each");
  if (want_newt) {
    TORCH_CHECK(film.has_value(), "exciter_newt: the waveshaper bank needs the FiLM parameters (film)");
    check_dev(*film, "film");
    check_same_device(src, "f0", *film, "film");
    TORCH_CHECK(film->numel() == B * T * NWS_FILM_CH, "film: expected (", B, ", ", T, ", 256), got ", film->sizes());
  }
  Launch L(src);
  Tensor exc = want_exciter ? at::empty({B, NWS_N_SHAPERS, N}, src.options()) : at::empty({0}, src.options());
  Tensor out = want_newt ? at::empty({B, N}, src.options()) : at::empty({0}, src.options());
  nws_check(nws_exciter_newt(w, fptr(f0), fptr(f0_up), carry.data_ptr<double>(), phase_u.data_ptr<float>(),
                             rand_phase.data_ptr<float>(), fptr(film), (int)B, (int)T, (float)sample_rate,
                             want_exciter ? exc.data_ptr<float>() : nullptr, want_newt ? out.data_ptr<float>() : nullptr, L.stream),
            "nws_exciter_newt");
  return {exc, out};
}

// HarmonicOscillator.forward (generators.py:58-66): f0_up (B, N) -> (B, 101, N)
Tensor oscillator(const Tensor& f0_up, const Tensor& phase_u, const Tensor& rand_phase, double sample_rate) {
  check_dev(f0_up, "f0");
  check_dev(phase_u, "phase_u");
  check_dev(rand_phase, "rand_phase");
  check_same_device(f0_up, "f0", phase_u, "phase_u");
  check_same_device(f0_up, "f0", rand_phase, "rand_phase");
  TORCH_CHECK(f0_up.dim() == 2, "HarmonicOscillator: expected f0 of shape (B, N), got ", f0_up.sizes());
  TORCH_CHECK(f0_up.size(1) % NWS_HOP == 0 && f0_up.size(1) > 0,
              "HarmonicOscillator on the HIP path: the sample count must be a multiple of ", NWS_HOP, ", got ", f0_up.size(1));
  TORCH_CHECK(phase_u.numel() == NWS_N_HARMONICS && rand_phase.numel() == NWS_N_HARMONICS,
              "kernels are specialised for 101 harmonics (gin/models/newt.gin)");
  const int64_t B = f0_up.size(0), N = f0_up.size(1);
  Launch L(f0_up);
  Tensor carry = at::empty({B, N / 32}, f0_up.options().dtype(at::kDouble));
  nws_check(nws_phase_carry(nullptr, f0_up.data_ptr<float>(), (int)B, (int)(N / NWS_HOP), carry.data_ptr<double>(), L.stream),
            "nws_phase_carry");
  Tensor out = at::empty({B, NWS_N_HARMONICS, N}, f0_up.options());
  nws_check(nws_oscillator(f0_up.data_ptr<float>(), carry.data_ptr<double>(), phase_u.data_ptr<float>(),
                           rand_phase.data_ptr<float>(), (int)B, (int)N, (float)sample_rate, out.data_ptr<float>(), L.stream),
            "nws_oscillator");
  return out;
}

// GRU(2 -> 128) over T frames of control[:, 0:2] (models/neural_waveshaping.py:24-25): -> (gru_out (B, T, 128), hT (B, 128))
std::tuple<Tensor, Tensor> control_gru(const Tensor& wdesc, const Tensor& control, const OptTensor& h0, bool batched) {
  const NwsWeights* w = weights_of(wdesc);
  check_dev(control, "control");
  TORCH_CHECK(control.dim() == 3 && control.size(1) >= 2, "control: expected (B, C>=2, T), got ", control.sizes());
  const int64_t B = control.size(0), C = control.size(1), T = control.size(2);
  TORCH_CHECK(T >= 1, "control: need at least one frame");
  if (h0.has_value()) {
    check_dev(*h0, "h0");
    check_same_device(control, "control", *h0, "h0");
    TORCH_CHECK(h0->numel() == B * NWS_HIDDEN, "h0: expected (", B, ", 128), got ", h0->sizes());
  }
  Launch L(control);
  Tensor out = at::empty({B, T, NWS_HIDDEN}, control.options());
  Tensor hT = at::empty({B, NWS_HIDDEN}, control.options());
  if (batched)
    nws_check(nws_control_gru_batched(w, control.data_ptr<float>(), (int)B, (int)C, (int)T, fptr(h0), out.data_ptr<float>(),
                                      hT.data_ptr<float>(), L.stream), "nws_control_gru_batched");
  else
    nws_check(nws_control_gru_state(w, control.data_ptr<float>(), (int)B, (int)C, (int)T, fptr(h0), out.data_ptr<float>(),
                                    hT.data_ptr<float>(), L.stream), "nws_control_gru_state");
  return {out, hT};
}

// The backward of control_gru for grad_out = dL/d(gru_out) (B, T, 128) and grad_hT = dL/d(hT): [grad_control
// (B, 2, T), grad_h0 (B, 128)], with want_params followed by [grad_w_ih, grad_w_hh, grad_b_ih, grad_b_hh].  gru_out is the forward's
// own output; the workspace comes from torch's allocator.
std::vector<Tensor> control_gru_grad(const Tensor& wdesc, const Tensor& control, const OptTensor& h0, const Tensor& gru_out,
                                     const Tensor& grad_out, const OptTensor& grad_hT, bool want_params) {
  const NwsWeights* w = weights_of(wdesc);
  check_dev(control, "control");
  check_dev(gru_out, "gru_out");
  check_dev(grad_out, "grad_out");
  check_same_device(control, "control", gru_out, "gru_out");
  check_same_device(control, "control", grad_out, "grad_out");
  TORCH_CHECK(control.dim() == 3 && control.size(1) >= 2, "control: expected (B, C>=2, T), got ", control.sizes());
  const int64_t B = control.size(0), C = control.size(1), T = control.size(2);
  TORCH_CHECK(B >= 1 && T >= 1, "control: need at least one utterance and one frame");
  for (const Tensor* t : {&gru_out, &grad_out})
    TORCH_CHECK(t->dim() == 3 && t->size(0) == B && t->size(1) == T && t->size(2) == NWS_HIDDEN,
                "control_gru_grad: gru_out / grad_out ", t->sizes(), " is not (", B, ", ", T, ", 128)");
  for (const OptTensor* o : {&h0, &grad_hT})
    if (o->has_value()) {
      check_dev(**o, "h0 / grad_hT");
      check_same_device(control, "control", **o, "h0 / grad_hT");
      TORCH_CHECK((*o)->numel() == B * NWS_HIDDEN, "h0 / grad_hT: expected (", B, ", 128), got ", (*o)->sizes());
    }
  Launch L(control);
  Tensor grad_control = at::empty({B, 2, T}, control.options());
  Tensor grad_h0 = at::empty({B, NWS_HIDDEN}, control.options());
  std::vector<Tensor> out{grad_control, grad_h0};
  float* gp[4] = {nullptr, nullptr, nullptr, nullptr};
  if (want_params) {
    out.push_back(at::empty({3 * NWS_HIDDEN, 2}, control.options()));
    out.push_back(at::empty({3 * NWS_HIDDEN, NWS_HIDDEN}, control.options()));
    out.push_back(at::empty({3 * NWS_HIDDEN}, control.options()));
    out.push_back(at::empty({3 * NWS_HIDDEN}, control.options()));
    for (int i = 0; i < 4; ++i) gp[i] = out[2 + i].data_ptr<float>();
  }
  const size_t nbytes = nws_control_gru_grad_workspace_bytes((int)B, (int)T, want_params ? 1 : 0);
  Tensor ws = at::empty({(int64_t)(nbytes > 0 ? nbytes : 1)}, control.options().dtype(at::kByte));
  nws_check(nws_control_gru_grad(w, control.data_ptr<float>(), (int)B, (int)C, (int)T, fptr(h0), gru_out.data_ptr<float>(),
                                 grad_out.data_ptr<float>(), fptr(grad_hT), grad_control.data_ptr<float>(), grad_h0.data_ptr<float>(),
                                 gp[0], gp[1], gp[2], gp[3], ws.data_ptr(), nbytes, L.stream), "nws_control_gru_grad");
  return out;
}

// proj + newt.mlp + h_generator + FIR design in one kernel: -> (emb (B,128,T), film (B,T,256), H (B,T,129), fir (B,T,128) upper half-taps)
std::tuple<Tensor, Tensor, Tensor, Tensor> frame_mlps(const Tensor& wdesc, const Tensor& gru_out, const Tensor& fir_design,
                                                       bool want_emb, bool want_H) {
  const NwsWeights* w = weights_of(wdesc);
  check_dev(gru_out, "gru_out");
  check_dev(fir_design, "fir_design");
  check_same_device(gru_out, "gru_out", fir_design, "fir_design");
  TORCH_CHECK(gru_out.dim() == 3 && gru_out.size(2) == NWS_HIDDEN, "gru_out: expected (B, T, 128), got ", gru_out.sizes());
  TORCH_CHECK(fir_design.numel() == NWS_FIR_LEN * 132, "fir_design: expected (256, 132)");
  const int64_t B = gru_out.size(0), T = gru_out.size(1);
  Launch L(gru_out);
  const auto o = gru_out.options();
  Tensor emb = want_emb ? at::empty({B, NWS_HIDDEN, T}, o) : at::empty({0}, o);
  Tensor film = at::empty({B, T, NWS_FILM_CH}, o);
  Tensor H = want_H ? at::empty({B, T, NWS_N_BANDS}, o) : at::empty({0}, o);
  Tensor fir = at::empty({B, T, NWS_FIR_HALF}, o);
  nws_check(nws_frame_mlps(w, gru_out.data_ptr<float>(), fir_design.data_ptr<float>(), (int)B, (int)T,
                           want_emb ? emb.data_ptr<float>() : nullptr, film.data_ptr<float>(),
                           want_H ? H.data_ptr<float>() : nullptr, fir.data_ptr<float>(), L.stream), "nws_frame_mlps");
  return {emb, film, H, fir};
}

// time-varying FIR noise (generators.py:30-35) + optional branch sum; origin / noise_len < 0: the reference's own framing
Tensor fir_noise(const Tensor& fir, const Tensor& noise, const OptTensor& add_in, int64_t origin) {
  check_dev(fir, "fir");
  check_dev(noise, "noise");
  check_same_device(fir, "fir", noise, "noise");
  TORCH_CHECK(fir.dim() == 3 && fir.size(2) == NWS_FIR_HALF, "fir: expected (B, T, 128) upper half-taps (nws_frame_mlps), got ", fir.sizes());
  const int64_t B = fir.size(0), T = fir.size(1);
  if (add_in.has_value()) {
    check_dev(*add_in, "add_in");
    check_same_device(fir, "fir", *add_in, "add_in");
    TORCH_CHECK(add_in->numel() == B * T * NWS_HOP, "add_in: expected (", B, ", ", T * NWS_HOP, "), got ", add_in->sizes());
  }
  Launch L(fir);
  Tensor out = at::empty({B, T * NWS_HOP}, fir.options());
  if (origin < 0) {
    TORCH_CHECK(noise.numel() == T * NWS_HOP - 1, "noise: expected ", T * NWS_HOP - 1, " samples, got ", noise.sizes());
    nws_check(nws_fir_noise(fir.data_ptr<float>(), noise.data_ptr<float>(), fptr(add_in), (int)B, (int)T, out.data_ptr<float>(),
                            L.stream), "nws_fir_noise");
  } else {
    nws_check(nws_fir_noise_window(fir.data_ptr<float>(), noise.data_ptr<float>(), (int)noise.numel(), (int)origin, fptr(add_in),
                                   (int)B, (int)T, out.data_ptr<float>(), L.stream), "nws_fir_noise_window");
  }
  return out;
}

// the frame MLPs with the folded weights (NwsWeights.mlp_spec): -> (film (B,T,256), spec (B,T,132) rows of filter spectra G[0 .. 128])
std::tuple<Tensor, Tensor> frame_mlps_spec(const Tensor& wdesc, const Tensor& gru_out) {
  const NwsWeights* w = weights_of(wdesc);
  check_dev(gru_out, "gru_out");
  TORCH_CHECK(gru_out.dim() == 3 && gru_out.size(2) == NWS_HIDDEN, "gru_out: expected (B, T, 128), got ", gru_out.sizes());
  const int64_t B = gru_out.size(0), T = gru_out.size(1);
  Launch L(gru_out);
  Tensor film = at::empty({B, T, NWS_FILM_CH}, gru_out.options());
  Tensor spec = at::zeros({B, T, NWS_SPEC_ROW}, gru_out.options());      // (the three floats behind bin 128 are never written)
  nws_check(nws_frame_mlps_spec(w, gru_out.data_ptr<float>(), (int)B, (int)T, film.data_ptr<float>(), spec.data_ptr<float>(), L.stream),
            "nws_frame_mlps_spec");
  return {film, spec};
}

// fir_noise on rows of filter spectra (B, T, 132) instead of half-taps; the reference's own framing, B >= 16
Tensor fir_noise_spec(const Tensor& spec, const Tensor& noise, const OptTensor& add_in) {
  check_dev(spec, "spec");
  check_dev(noise, "noise");
  check_same_device(spec, "spec", noise, "noise");
  TORCH_CHECK(spec.dim() == 3 && spec.size(2) == NWS_SPEC_ROW, "spec: expected (B, T, 132) filter spectra (nws_frame_mlps_spec), got ", spec.sizes());
  const int64_t B = spec.size(0), T = spec.size(1);
  TORCH_CHECK(noise.numel() == T * NWS_HOP - 1, "noise: expected ", T * NWS_HOP - 1, " samples, got ", noise.sizes());
  if (add_in.has_value()) {
    check_dev(*add_in, "add_in");
    check_same_device(spec, "spec", *add_in, "add_in");
    TORCH_CHECK(add_in->numel() == B * T * NWS_HOP, "add_in: expected (", B, ", ", T * NWS_HOP, "), got ", add_in->sizes());
  }
  Launch L(spec);
  Tensor out = at::empty({B, T * NWS_HOP}, spec.options());
  nws_check(nws_fir_noise_spec(spec.data_ptr<float>(), noise.data_ptr<float>(), fptr(add_in), (int)B, (int)T, out.data_ptr<float>(), L.stream),
            "nws_fir_noise_spec");
  return out;
}

// FIRNoiseSynth's zero-phase FIR design from H (B, 129, T) (generators.py:22-28) -> upper half-taps (B, T, 128)
Tensor fir_from_h(const Tensor& H, const Tensor& fir_design) {
  check_dev(H, "H");
  check_dev(fir_design, "fir_design");
  check_same_device(H, "H", fir_design, "fir_design");
  TORCH_CHECK(H.dim() == 3 && H.size(1) == NWS_N_BANDS, "FIRNoiseSynth: expected H of shape (B, 129, T), got ", H.sizes());
  TORCH_CHECK(fir_design.numel() == NWS_FIR_LEN * 132, "fir_design: expected (256, 132)");
  Launch L(H);
  Tensor fir = at::empty({H.size(0), H.size(2), NWS_FIR_HALF}, H.options());
  nws_check(nws_fir_from_h(H.data_ptr<float>(), fir_design.data_ptr<float>(), (int)H.size(0), (int)H.size(2), fir.data_ptr<float>(),
                           L.stream), "nws_fir_from_h");
  return fir;
}

// dL/d(fir) of fir_noise for grad_out = dL/d(out) (B, 128 T) and the excitation the forward used: (B, T, 128)
Tensor fir_noise_grad(const Tensor& noise, const Tensor& grad_out) {
  check_dev(noise, "noise");
  check_dev(grad_out, "grad_out");
  check_same_device(grad_out, "grad_out", noise, "noise");
  TORCH_CHECK(grad_out.dim() == 2 && grad_out.size(1) % NWS_HOP == 0 && grad_out.size(1) >= 2 * NWS_HOP,
              "fir_noise_grad: expected grad_out (B, 128 T) with T >= 2, got ", grad_out.sizes());
  const int64_t B = grad_out.size(0), T = grad_out.size(1) / NWS_HOP;
  TORCH_CHECK(noise.numel() == T * NWS_HOP - 1, "noise: expected ", T * NWS_HOP - 1, " samples, got ", noise.sizes());
  Launch L(grad_out);
  Tensor grad_fir = at::empty({B, T, NWS_FIR_HALF}, grad_out.options());
  nws_check(nws_fir_noise_grad(noise.data_ptr<float>(), grad_out.data_ptr<float>(), (int)B, (int)T, grad_fir.data_ptr<float>(),
                               L.stream), "nws_fir_noise_grad");
  return grad_fir;
}

// dL/dH of fir_from_h for grad_fir (B, T, 128): (B, 129, T)
Tensor fir_from_h_grad(const Tensor& grad_fir, const Tensor& fir_design) {
  check_dev(grad_fir, "grad_fir");
  check_dev(fir_design, "fir_design");
  check_same_device(grad_fir, "grad_fir", fir_design, "fir_design");
  TORCH_CHECK(grad_fir.dim() == 3 && grad_fir.size(2) == NWS_FIR_HALF, "fir_from_h_grad: expected grad_fir (B, T, 128), got ", grad_fir.sizes());
  TORCH_CHECK(fir_design.numel() == NWS_FIR_LEN * 132, "fir_design: expected (256, 132)");
  Launch L(grad_fir);
  Tensor grad_H = at::empty({grad_fir.size(0), NWS_N_BANDS, grad_fir.size(1)}, grad_fir.options());
  nws_check(nws_fir_from_h_grad(grad_fir.data_ptr<float>(), fir_design.data_ptr<float>(), (int)grad_fir.size(0), (int)grad_fir.size(1),
                                grad_H.data_ptr<float>(), L.stream), "nws_fir_from_h_grad");
  return grad_H;
}

// (B, C, T) -> (C): the sum over batch and time in float64, in a fixed order (the backward of adding a per-channel offset)
Tensor sum_batch_time(const Tensor& x) {
  check_dev(x, "x");
  TORCH_CHECK(x.dim() == 3, "sum_batch_time: expected (B, C, T), got ", x.sizes());
  Launch L(x);
  Tensor out = at::empty({x.size(1)}, x.options());
  nws_check(nws_sum_batch_time(x.data_ptr<float>(), (int)x.size(0), (int)x.size(1), (int)x.size(2), out.data_ptr<float>(), L.stream),
            "nws_sum_batch_time");
  return out;
}

// Reverb.forward (shaping.py:161-173): x (B, N) -> x + circconv_L(x, [0, ir])[:N]
Tensor reverb(const Tensor& plan_t, const Tensor& tables, const Tensor& spectrum, const Tensor& x) {
  NwsReverbPlan plan = plan_of(plan_t);
  check_dev(x, "x");
  check_dev(tables, "reverb_tables");
  check_dev(spectrum, "reverb_spectrum");
  check_same_device(x, "x", tables, "reverb tables");
  check_same_device(x, "x", spectrum, "reverb.ir spectrum");
  TORCH_CHECK(x.dim() == 2, "Reverb: expected (B, N), got ", x.sizes());
  check_reverb_buffers(plan, tables, spectrum);
  const int64_t B = x.size(0), N = x.size(1);
  TORCH_CHECK(nws_reverb_plan_serves(&plan, (int)N, 0), "Reverb: the plan [L ", plan.L, ", Lc ", plan.Lc, ", hist ", plan.hist, ", nblk ", plan.nblk,
              "] was not made for ", N, " samples");
  Launch L(x);
  const size_t nbytes = nws_reverb_workspace_bytes(&plan, (int)B);
  Tensor ws = at::empty({(int64_t)nbytes}, x.options().dtype(at::kByte));
  Tensor y = at::empty_like(x);
  nws_check(nws_reverb(&plan, tables.data_ptr(), spectrum.data_ptr(), x.data_ptr<float>(), (int)B, (int)N, y.data_ptr<float>(),
                       ws.data_ptr(), nbytes, L.stream), "nws_reverb");
  return y;
}

// dL/dx of Reverb.forward for grad_out = dL/dy (B, N): the forward's launches with the conjugated IR spectrum
Tensor reverb_grad_x(const Tensor& plan_t, const Tensor& tables, const Tensor& spectrum, const Tensor& grad_out) {
  NwsReverbPlan plan = plan_of(plan_t);
  check_dev(grad_out, "grad_out");
  check_dev(tables, "reverb_tables");
  check_dev(spectrum, "reverb_spectrum");
  check_same_device(grad_out, "grad_out", tables, "reverb tables");
  check_same_device(grad_out, "grad_out", spectrum, "reverb.ir spectrum");
  TORCH_CHECK(grad_out.dim() == 2, "reverb_grad_x: expected (B, N), got ", grad_out.sizes());
  check_reverb_buffers(plan, tables, spectrum);
  const int64_t B = grad_out.size(0), N = grad_out.size(1);
  TORCH_CHECK(nws_reverb_plan_serves(&plan, (int)N, 0), "reverb_grad_x: the plan [L ", plan.L, ", Lc ", plan.Lc, ", hist ", plan.hist,
              ", nblk ", plan.nblk, "] was not made for ", N, " samples");
  Launch L(grad_out);
  const size_t nbytes = nws_reverb_grad_workspace_bytes(&plan, (int)B, 0);
  Tensor ws = at::empty({(int64_t)nbytes}, grad_out.options().dtype(at::kByte));
  Tensor dx = at::empty_like(grad_out);
  nws_check(nws_reverb_grad_x(&plan, tables.data_ptr(), spectrum.data_ptr(), grad_out.data_ptr<float>(), (int)B, (int)N,
                              dx.data_ptr<float>(), ws.data_ptr(), nbytes, L.stream), "nws_reverb_grad_x");
  return dx;
}

// dL/d(ir) of Reverb.forward, summed over the batch: (ir_len)
Tensor reverb_grad_ir(const Tensor& plan_t, const Tensor& tables, const Tensor& x, const Tensor& grad_out, int64_t ir_len) {
  NwsReverbPlan plan = plan_of(plan_t);
  check_dev(x, "x");
  check_dev(grad_out, "grad_out");
  check_dev(tables, "reverb_tables");
  check_same_device(x, "x", tables, "reverb tables");
  check_same_device(x, "x", grad_out, "grad_out");
  TORCH_CHECK(x.dim() == 2 && grad_out.sizes() == x.sizes(), "reverb_grad_ir: x ", x.sizes(), " and grad_out ", grad_out.sizes(),
              " differ in shape");
  TORCH_CHECK((size_t)tables.numel() * tables.element_size() == nws_reverb_table_bytes(&plan), "reverb_tables: ",
              (size_t)tables.numel() * tables.element_size(), " bytes, the plan (L = ", plan.L, ") needs ", nws_reverb_table_bytes(&plan));
  const int64_t B = x.size(0), N = x.size(1);
  TORCH_CHECK(ir_len > 0 && ir_len < (1 << 30) && nws_reverb_plan_serves(&plan, (int)N, (int)ir_len + 1), "reverb_grad_ir: the plan [L ",
              plan.L, ", Lc ", plan.Lc, ", hist ", plan.hist, ", nblk ", plan.nblk, "] was not made for ", N, " samples and an impulse response of ",
              ir_len);
  Launch L(x);
  const size_t nbytes = nws_reverb_grad_workspace_bytes(&plan, (int)B, 1);
  Tensor ws = at::empty({(int64_t)nbytes}, x.options().dtype(at::kByte));
  Tensor dir = at::empty({ir_len}, x.options());
  nws_check(nws_reverb_grad_ir(&plan, tables.data_ptr(), x.data_ptr<float>(), grad_out.data_ptr<float>(), (int)B, (int)N, (int)ir_len,
                               dir.data_ptr<float>(), ws.data_ptr(), nbytes, L.stream), "nws_reverb_grad_ir");
  return dir;
}

// streaming (linear) reverb chunk: -> (y (B, M), tail_out (B, tail_len))
std::tuple<Tensor, Tensor> reverb_linear_chunk(const Tensor& plan_t, const Tensor& tables, const Tensor& spectrum, const Tensor& x,
                                               const Tensor& tail_in) {
  NwsReverbPlan plan = plan_of(plan_t);
  check_dev(x, "x");
  check_dev(tail_in, "tail_in");
  check_dev(tables, "reverb_tables");
  check_dev(spectrum, "reverb_spectrum");
  check_same_device(x, "x", tail_in, "tail_in");
  check_same_device(x, "x", tables, "reverb tables");
  TORCH_CHECK(x.dim() == 2 && tail_in.dim() == 2 && tail_in.size(0) == x.size(0), "reverb_linear_chunk: x (B, M), tail_in (B, tail)");
  const int64_t B = x.size(0), M = x.size(1), tail_len = tail_in.size(1);
  check_reverb_buffers(plan, tables, spectrum);
  check_same_device(x, "x", spectrum, "reverb.ir spectrum");
  TORCH_CHECK(plan.Lc == 0, "reverb_linear_chunk: needs a direct plan (one transform of M + tail_len samples)");
  TORCH_CHECK(M + tail_len <= plan.L, "reverb_linear_chunk: chunk of ", M, " + tail of ", tail_len, " samples wraps around L = ", plan.L);
  Launch L(x);
  const size_t nbytes = (size_t)(2 * ((B + 1) / 2) * plan.L + B * plan.L) * sizeof(float);
  Tensor ws = at::empty({(int64_t)nbytes}, x.options().dtype(at::kByte));
  Tensor y = at::empty_like(x);
  Tensor tail_out = at::empty_like(tail_in);
  nws_check(nws_reverb_linear_chunk(&plan, tables.data_ptr(), spectrum.data_ptr(), x.data_ptr<float>(), (int)B, (int)M,
                                    tail_in.data_ptr<float>(), tail_out.data_ptr<float>(), (int)tail_len, y.data_ptr<float>(),
                                    ws.data_ptr(), nbytes, L.stream), "nws_reverb_linear_chunk");
  return {y, tail_out};
}

// TrainableNonlinearity.forward / FastNEWT.shaping_fn on (B, 64, N) (shaping.py:36-37, :136-151)
Tensor shaper_apply(const Tensor& wdesc, const Tensor& x) {
  const NwsWeights* w = weights_of(wdesc);
  check_dev(x, "x");
  TORCH_CHECK(x.dim() == 3 && x.size(1) == NWS_N_SHAPERS, "expected (B, 64, N), got ", x.sizes());
  Launch L(x);
  Tensor y = at::empty_like(x);
  nws_check(nws_shaper_apply(w, x.data_ptr<float>(), x.size(0), x.size(2), y.data_ptr<float>(), L.stream), "nws_shaper_apply");
  return y;
}

// FastNEWT._init_lookup_table (shaping.py:107-119)
Tensor shaper_table(const Tensor& wdesc, const Tensor& like, int64_t size, double tmin, double tmax) {
  const NwsWeights* w = weights_of(wdesc);
  check_dev(like, "shaping_fn.input_scale");
  TORCH_CHECK(size >= 2 && tmax > tmin, "FastNEWT: need table_size >= 2 and table_max > table_min");
  Launch L(like);
  Tensor table = at::empty({NWS_N_SHAPERS, size}, like.options());
  nws_check(nws_shaper_table(w, (int)size, (float)tmin, (float)tmax, table.data_ptr<float>(), L.stream), "nws_shaper_table");
  return table;
}

// NEWT.forward / FastNEWT.forward on a materialised exciter (shaping.py:67-79): film (B, 256, T) channel-major
Tensor newt_apply(const Tensor& wdesc, const Tensor& exciter, const Tensor& film) {
  const NwsWeights* w = weights_of(wdesc);
  check_dev(exciter, "exciter");
  check_dev(film, "film_params");
  check_same_device(exciter, "exciter", film, "control embedding");
  TORCH_CHECK(exciter.dim() == 3 && exciter.size(1) == NWS_N_SHAPERS, "NEWT: expected an exciter of shape (B, 64, N), got ", exciter.sizes());
  TORCH_CHECK(film.dim() == 3 && film.size(1) == NWS_FILM_CH && film.size(0) == exciter.size(0),
              "NEWT: expected FiLM parameters of shape (B, 256, T), got ", film.sizes());
  const int64_t B = exciter.size(0), T = film.size(2);
  TORCH_CHECK(exciter.size(2) == T * NWS_HOP, "NEWT: exciter has ", exciter.size(2), " samples, the control embedding ", T,
              " frames (x128 = ", T * NWS_HOP, ")");
  Launch L(exciter);
  Tensor out = at::empty({B, 1, T * NWS_HOP}, exciter.options());
  nws_check(nws_newt_apply(w, exciter.data_ptr<float>(), film.data_ptr<float>(), (int)B, (int)T, out.data_ptr<float>(), L.stream),
            "nws_newt_apply");
  return out;
}

// The backward of newt_apply with the exact shapers for grad_out = dL/d(out) (B, 1, N): [grad_film (B, 256, T)],
// then grad_exciter (B, 64, N) when wanted, then with want_params the eleven parameter gradients in the shapes of their
// parameters: input_scale, net.0.weight, net.0.bias, net.2.*, net.4.*, net.6.*, mixer.0.weight, mixer.0.bias.  Nothing was saved
// by the forward; the workspace comes from torch's allocator.
std::vector<Tensor> newt_grad(const Tensor& wdesc, const Tensor& exciter, const Tensor& film, const Tensor& grad_out, bool want_exciter,
                              bool want_params) {
  const NwsWeights* w = weights_of(wdesc);
  check_dev(exciter, "exciter");
  check_dev(film, "film_params");
  check_dev(grad_out, "grad_out");
  check_same_device(exciter, "exciter", film, "control embedding");
  check_same_device(exciter, "exciter", grad_out, "grad_out");
  TORCH_CHECK(exciter.dim() == 3 && exciter.size(1) == NWS_N_SHAPERS, "NEWT: expected an exciter of shape (B, 64, N), got ", exciter.sizes());
  TORCH_CHECK(film.dim() == 3 && film.size(1) == NWS_FILM_CH && film.size(0) == exciter.size(0),
              "NEWT: expected FiLM parameters of shape (B, 256, T), got ", film.sizes());
  const int64_t B = exciter.size(0), T = film.size(2), N = T * NWS_HOP;
  TORCH_CHECK(B >= 1 && T >= 1, "newt_grad: need at least one utterance and one frame");
  TORCH_CHECK(exciter.size(2) == N, "NEWT: exciter has ", exciter.size(2), " samples, the control embedding ", T, " frames (x128 = ",
              N, ")");
  TORCH_CHECK(grad_out.numel() == B * N && grad_out.size(0) == B, "newt_grad: grad_out ", grad_out.sizes(), " is not (", B, ", 1, ", N, ")");
  TORCH_CHECK(w->lut == nullptr, "newt_grad: the lookup table has no backward");
  const size_t nbytes = B < (1 << 30) && T < (1 << 30) ? nws_newt_grad_workspace_bytes((int)B, (int)T, want_params ? 1 : 0) : 0;
  TORCH_CHECK(nbytes > 0, "newt_grad: unsupported size (B ", B, ", T ", T, "): T <= 65535, B T <= 2^28");
  Launch L(exciter);
  auto opt = exciter.options();
  std::vector<Tensor> out{at::empty({B, NWS_FILM_CH, T}, opt)};
  float* ge = nullptr;
  if (want_exciter) {
    out.push_back(at::empty_like(exciter));
    ge = out.back().data_ptr<float>();
  }
  float* gp[11] = {nullptr};
  if (want_params) {
    const int64_t S = NWS_N_SHAPERS, SW = NWS_N_SHAPERS * 8;
    const std::vector<std::vector<int64_t>> shapes = {{1, S, 1}, {SW, 1, 1}, {SW}, {SW, 8, 1}, {SW}, {SW, 8, 1}, {SW}, {S, 8, 1}, {S},
                                                      {1, S, 1}, {1}};
    for (int i = 0; i < 11; ++i) {
      out.push_back(at::empty(shapes[i], opt));
      gp[i] = out.back().data_ptr<float>();
    }
  }
  Tensor ws = at::empty({(int64_t)nbytes}, opt.dtype(at::kByte));
  nws_check(nws_newt_grad(w, exciter.data_ptr<float>(), film.data_ptr<float>(), grad_out.data_ptr<float>(), (int)B, (int)T, ge,
                          out[0].data_ptr<float>(), gp[0], gp[1], gp[2], gp[3], gp[4], gp[5], gp[6], gp[7], gp[8], gp[9], gp[10],
                          ws.data_ptr(), nbytes, L.stream), "nws_newt_grad");
  return out;
}

// clip_grad_norm_(max_norm, 2.0) + Adam over every listed tensor in two launches (csrc/adam_step.hip): params,
// exp_avgs and exp_avg_sqs are updated in place and their version counters raised - everything that caches tables derived from
// the weights keys on Tensor._version - grads are read and not rewritten; returns the gradients' total norm, a 0-dim tensor.
Tensor adam_step(at::TensorList params, at::TensorList grads, at::TensorList exp_avgs, at::TensorList exp_avg_sqs, int64_t step,
                 double lr, double beta1, double beta2, double eps, double max_norm) {
  const size_t n = params.size();
  TORCH_CHECK(n >= 1, "adam_step: no tensors");
  TORCH_CHECK(grads.size() == n && exp_avgs.size() == n && exp_avg_sqs.size() == n, "adam_step: ", n, " params but ", grads.size(),
              " grads, ", exp_avgs.size(), " exp_avgs, ", exp_avg_sqs.size(), " exp_avg_sqs");
  TORCH_CHECK(step >= 1, "adam_step: step counts from 1, got ", step);
  std::vector<NwsAdamTensor> recs(n);
  for (size_t k = 0; k < n; ++k) {
    check_dev(params[k], "param");
    check_dev(grads[k], "grad");
    check_dev(exp_avgs[k], "exp_avg");
    check_dev(exp_avg_sqs[k], "exp_avg_sq");
    check_same_device(params[0], "params[0]", params[k], "param");
    check_same_device(params[k], "param", grads[k], "grad");
    check_same_device(params[k], "param", exp_avgs[k], "exp_avg");
    check_same_device(params[k], "param", exp_avg_sqs[k], "exp_avg_sq");
    TORCH_CHECK(grads[k].sizes() == params[k].sizes() && exp_avgs[k].sizes() == params[k].sizes() &&
                    exp_avg_sqs[k].sizes() == params[k].sizes(), "adam_step: tensor ", k, ": param ", params[k].sizes(), ", grad ",
                grads[k].sizes(), ", exp_avg ", exp_avgs[k].sizes(), ", exp_avg_sq ", exp_avg_sqs[k].sizes(), " differ in shape");
    TORCH_CHECK(params[k].numel() >= 1, "adam_step: tensor ", k, " is empty");
    recs[k] = NwsAdamTensor{params[k].data_ptr<float>(), grads[k].data_ptr<float>(), exp_avgs[k].data_ptr<float>(),
                            exp_avg_sqs[k].data_ptr<float>(), (long long)params[k].numel()};
  }
  const size_t nbytes = nws_adam_workspace_bytes(recs.data(), (int)n);
  TORCH_CHECK(nbytes > 0, "adam_step: unsupported sizes");
  Launch L(params[0]);
  Tensor total = at::empty({}, params[0].options());
  Tensor ws = at::empty({(int64_t)(nbytes / 8)}, params[0].options().dtype(at::kDouble));
  nws_check(nws_adam_step(recs.data(), (int)n, (long long)step, lr, beta1, beta2, eps, max_norm, total.data_ptr<float>(), ws.data_ptr(),
                          nbytes, L.stream), "nws_adam_step");
  for (size_t k = 0; k < n; ++k) {
    params[k].unsafeGetTensorImpl()->bump_version();
    exp_avgs[k].unsafeGetTensorImpl()->bump_version();
    exp_avg_sqs[k].unsafeGetTensorImpl()->bump_version();
  }
  return total;
}

// Data-parallel training (csrc/grad_reduce.hip).  grad_pack: the listed tensors one after the other into the
// front of `out` (a 1-D tensor, usually one rank's row of the exchange buffer).  grad_reduce: out[i] = mean over the rows of
// rows[:, i] for i < out.numel(), summed in float64 in row order.  Both write `out` only, which no cache keys on.
void grad_pack(at::TensorList tensors, Tensor& out) {
  const size_t n = tensors.size();
  TORCH_CHECK(n >= 1, "grad_pack: no tensors");
  check_dev(out, "out");
  TORCH_CHECK(out.dim() == 1, "grad_pack: out: expected a 1-D tensor, got ", out.sizes());
  std::vector<NwsGradTensor> recs(n);
  int64_t total = 0;
  for (size_t k = 0; k < n; ++k) {
    check_dev(tensors[k], "tensor");
    check_same_device(out, "out", tensors[k], "tensor");
    TORCH_CHECK(tensors[k].numel() >= 1, "grad_pack: tensor ", k, " is empty");
    recs[k] = NwsGradTensor{tensors[k].data_ptr<float>(), (size_t)tensors[k].numel()};
    total += tensors[k].numel();
  }
  TORCH_CHECK(out.numel() >= total, "grad_pack: out holds ", out.numel(), " elements, the tensors have ", total);
  Launch L(out);
  nws_check(nws_grad_pack(recs.data(), (int)n, out.data_ptr<float>(), (size_t)out.numel(), L.stream), "nws_grad_pack");
}

void grad_reduce(const Tensor& rows, Tensor& out) {
  check_dev(rows, "rows");
  check_dev(out, "out");
  check_same_device(rows, "rows", out, "out");
  TORCH_CHECK(rows.dim() == 2 && rows.size(0) >= 1, "grad_reduce: rows: expected (world, stride), got ", rows.sizes());
  TORCH_CHECK(out.dim() == 1 && out.numel() >= 1 && out.numel() <= rows.size(1), "grad_reduce: out: expected a 1-D tensor of 1 .. ",
              rows.size(1), " elements (the rows' stride), got ", out.sizes());
  Launch L(rows);
  nws_check(nws_grad_reduce(rows.data_ptr<float>(), (int)std::min<int64_t>(rows.size(0), 1 << 30), (size_t)out.numel(),
                            (size_t)rows.size(1), out.data_ptr<float>(), L.stream), "nws_grad_reduce");
}

// TimeDistributedMLP.forward (dynamic.py:20-40): x (B, in, T); weights[i] (rows_i, cols_i[, 1]), biases[i]; ln_w / ln_b for
// every layer but the last
Tensor td_mlp(const Tensor& x, at::TensorList weights, at::TensorList biases, at::TensorList ln_w, at::TensorList ln_b, double eps,
              double slope) {
  check_dev(x, "x");
  TORCH_CHECK(x.dim() == 3, "TimeDistributedMLP: expected (B, C, T), got ", x.sizes());
  const int depth = (int)weights.size();
  TORCH_CHECK(depth >= 1 && depth <= 8 && (int)biases.size() == depth && (int)ln_w.size() == depth - 1 &&
                  (int)ln_b.size() == depth - 1, "TimeDistributedMLP: inconsistent layer lists");
  const int64_t B = x.size(0), in_size = x.size(1), T = x.size(2);
  const int64_t hidden = weights[0].size(0), out_size = weights[depth - 1].size(0);
  const float* wp[8];
  const float* bp[8];
  const float* gp[8] = {nullptr};
  const float* lp[8] = {nullptr};
  for (int i = 0; i < depth; ++i) {
    check_dev(weights[i], "net weight");
    check_dev(biases[i], "net bias");
    check_same_device(x, "x", weights[i], "the MLP's parameters");
    const int64_t rows = i == depth - 1 ? out_size : hidden, cols = i == 0 ? in_size : hidden;
    TORCH_CHECK(weights[i].numel() == rows * cols && weights[i].size(0) == rows, "TimeDistributedMLP layer ", i, ": weight ",
                weights[i].sizes(), " does not match (", rows, ", ", cols, ") - input has ", in_size, " channels");
    TORCH_CHECK(biases[i].numel() == rows, "TimeDistributedMLP layer ", i, ": bias ", biases[i].sizes());
    wp[i] = weights[i].data_ptr<float>();
    bp[i] = biases[i].data_ptr<float>();
    if (i < depth - 1) {
      check_dev(ln_w[i], "layer_norm weight");
      check_dev(ln_b[i], "layer_norm bias");
      TORCH_CHECK(ln_w[i].numel() == hidden && ln_b[i].numel() == hidden, "LayerNorm ", i, ": expected ", hidden, " elements");
      gp[i] = ln_w[i].data_ptr<float>();
      lp[i] = ln_b[i].data_ptr<float>();
    }
  }
  Launch L(x);
  Tensor y = at::empty({B, out_size, T}, x.options());
  nws_check(nws_td_mlp(x.data_ptr<float>(), (int)B, (int)in_size, (int)hidden, (int)out_size, depth, (int)T, wp, bp, gp, lp,
                       (float)eps, (float)slope, y.data_ptr<float>(), L.stream), "nws_td_mlp");
  return y;
}

// The backward of td_mlp for grad_y = dL/dy: [grad_x] + grad_weights + grad_biases + grad_ln_w + grad_ln_b, or
// grad_x alone without want_params.  Nothing was saved by the forward; the workspace comes from torch's allocator.
std::vector<Tensor> td_mlp_grad(const Tensor& x, const Tensor& grad_y, at::TensorList weights, at::TensorList biases, at::TensorList ln_w,
                                at::TensorList ln_b, double eps, double slope, bool want_params) {
  check_dev(x, "x");
  check_dev(grad_y, "grad_y");
  check_same_device(x, "x", grad_y, "grad_y");
  TORCH_CHECK(x.dim() == 3, "td_mlp_grad: expected x (B, C, T), got ", x.sizes());
  const int depth = (int)weights.size();
  TORCH_CHECK(depth >= 1 && depth <= 8 && (int)biases.size() == depth && (int)ln_w.size() == depth - 1 &&
                  (int)ln_b.size() == depth - 1, "td_mlp_grad: inconsistent layer lists");
  const int64_t B = x.size(0), in_size = x.size(1), T = x.size(2);
  const int64_t hidden = weights[0].size(0), out_size = weights[depth - 1].size(0);
  TORCH_CHECK(grad_y.dim() == 3 && grad_y.size(0) == B && grad_y.size(1) == out_size && grad_y.size(2) == T,
              "td_mlp_grad: grad_y ", grad_y.sizes(), " is not (", B, ", ", out_size, ", ", T, ")");
  const float* wp[8];
  const float* bp[8];
  const float* gp[8] = {nullptr};
  const float* lp[8] = {nullptr};
  float* gwp[8] = {nullptr};
  float* gbp[8] = {nullptr};
  float* ggp[8] = {nullptr};
  float* glp[8] = {nullptr};
  std::vector<Tensor> gw, gb, gg, gl;
  for (int i = 0; i < depth; ++i) {
    check_dev(weights[i], "net weight");
    check_dev(biases[i], "net bias");
    check_same_device(x, "x", weights[i], "the MLP's parameters");
    const int64_t rows = i == depth - 1 ? out_size : hidden, cols = i == 0 ? in_size : hidden;
    TORCH_CHECK(weights[i].numel() == rows * cols && weights[i].size(0) == rows, "td_mlp_grad layer ", i, ": weight ",
                weights[i].sizes(), " does not match (", rows, ", ", cols, ") - input has ", in_size, " channels");
    TORCH_CHECK(biases[i].numel() == rows, "td_mlp_grad layer ", i, ": bias ", biases[i].sizes());
    wp[i] = weights[i].data_ptr<float>();
    bp[i] = biases[i].data_ptr<float>();
    if (want_params) {
      gw.push_back(at::empty(weights[i].sizes(), x.options()));
      gb.push_back(at::empty(biases[i].sizes(), x.options()));
      gwp[i] = gw.back().data_ptr<float>();
      gbp[i] = gb.back().data_ptr<float>();
    }
    if (i < depth - 1) {
      check_dev(ln_w[i], "layer_norm weight");
      check_dev(ln_b[i], "layer_norm bias");
      TORCH_CHECK(ln_w[i].numel() == hidden && ln_b[i].numel() == hidden, "LayerNorm ", i, ": expected ", hidden, " elements");
      gp[i] = ln_w[i].data_ptr<float>();
      lp[i] = ln_b[i].data_ptr<float>();
      if (want_params) {
        gg.push_back(at::empty(ln_w[i].sizes(), x.options()));
        gl.push_back(at::empty(ln_b[i].sizes(), x.options()));
        ggp[i] = gg.back().data_ptr<float>();
        glp[i] = gl.back().data_ptr<float>();
      }
    }
  }
  Launch L(x);
  Tensor grad_x = at::empty_like(x);
  const size_t nbytes = want_params ? nws_td_mlp_grad_workspace_bytes((int)B, (int)in_size, (int)hidden, (int)out_size, depth, (int)T, 1) : 0;
  Tensor ws = at::empty({(int64_t)(nbytes > 0 ? nbytes : 1)}, x.options().dtype(at::kByte));
  nws_check(nws_td_mlp_grad(x.data_ptr<float>(), grad_y.data_ptr<float>(), (int)B, (int)in_size, (int)hidden, (int)out_size, depth,
                            (int)T, wp, bp, gp, lp, (float)eps, (float)slope, grad_x.data_ptr<float>(), want_params ? gwp : nullptr,
                            want_params ? gbp : nullptr, want_params ? ggp : nullptr, want_params ? glp : nullptr,
                            ws.data_ptr(), nbytes, L.stream), "nws_td_mlp_grad");
  std::vector<Tensor> out{grad_x};
  for (auto* lst : {&gw, &gb, &gg, &gl}) out.insert(out.end(), lst->begin(), lst->end());
  return out;
}

Tensor td_layer_norm(const Tensor& x, const Tensor& weight, const Tensor& bias, double eps) {
  check_dev(x, "x");
  check_dev(weight, "layer_norm.weight");
  check_dev(bias, "layer_norm.bias");
  check_same_device(x, "x", weight, "layer_norm.weight");
  TORCH_CHECK(x.dim() == 3, "TimeDistributedLayerNorm: expected (B, C, T), got ", x.sizes());
  TORCH_CHECK(weight.numel() == x.size(1) && bias.numel() == x.size(1), "TimeDistributedLayerNorm: input has ", x.size(1),
              " channels, the LayerNorm ", weight.numel());
  Launch L(x);
  Tensor y = at::empty_like(x);
  nws_check(nws_td_layer_norm(x.data_ptr<float>(), weight.data_ptr<float>(), bias.data_ptr<float>(), (int)x.size(0), (int)x.size(1),
                              (int)x.size(2), (float)eps, y.data_ptr<float>(), L.stream), "nws_td_layer_norm");
  return y;
}

Tensor film(const Tensor& x, const Tensor& gamma, const Tensor& beta) {
  check_dev(x, "x");
  check_dev(gamma, "gamma");
  check_dev(beta, "beta");
  check_same_device(x, "x", gamma, "gamma");
  check_same_device(x, "x", beta, "beta");
  TORCH_CHECK(x.sizes() == gamma.sizes() && x.sizes() == beta.sizes(), "FiLM: x ", x.sizes(), ", gamma ", gamma.sizes(), ", beta ",
              beta.sizes(), " must have the same shape (expand and make contiguous first)");
  Launch L(x);
  Tensor y = at::empty_like(x);
  nws_check(nws_film(x.data_ptr<float>(), gamma.data_ptr<float>(), beta.data_ptr<float>(), x.numel(), y.data_ptr<float>(), L.stream),
            "nws_film");
  return y;
}

Tensor sine(const Tensor& x) {
  check_dev(x, "x");
  Launch L(x);
  Tensor y = at::empty_like(x);
  nws_check(nws_sin(x.data_ptr<float>(), y.data_ptr<float>(), x.numel(), L.stream), "nws_sin");
  return y;
}

// extract_perceptual_loudness (data/utils/loudness_extraction.py:41-67): audio (B, N) -> (B, 1 + N / hop)
Tensor loudness(const Tensor& audio, const Tensor& dft, int64_t n_fft, int64_t hop, double amin, double top_db, bool normalise) {
  check_dev(audio, "audio");
  check_dev(dft, "dft");
  check_same_device(audio, "audio", dft, "dft");
  TORCH_CHECK(audio.dim() == 2, "loudness: expected (B, N), got ", audio.sizes());
  const int64_t B = audio.size(0), N = audio.size(1);
  const size_t nbytes = nws_loudness_workspace_bytes((int)B, (int)N, (int)n_fft, (int)hop);
  TORCH_CHECK(nbytes > 0, "loudness: unsupported n_fft / hop_length (", n_fft, ", ", hop,
              "): n_fft must be a power of two in [64, 2048], 1 <= hop <= n_fft and 31 hop + n_fft samples must fit 160 KB of LDS");
  TORCH_CHECK((size_t)dft.numel() * sizeof(float) == nws_loudness_dft_bytes((int)n_fft), "loudness: dft does not belong to n_fft = ", n_fft);
  Launch L(audio);
  Tensor ws = at::empty({(int64_t)nbytes}, audio.options().dtype(at::kByte));
  Tensor out = at::empty({B, nws_loudness_frames((int)N, (int)hop)}, audio.options());
  nws_check(nws_loudness(audio.data_ptr<float>(), (int)B, (int)N, (int)n_fft, (int)hop, dft.data_ptr<float>(), (float)amin,
                         (float)top_db, normalise ? 1 : 0, out.data_ptr<float>(), ws.data_ptr(), nbytes, L.stream), "nws_loudness");
  return out;
}

void check_loudness_sizes(const char* op, const Tensor& dft, int64_t n_fft, int64_t hop) {
  TORCH_CHECK(nws_loudness_workspace_bytes(1, 1, (int)n_fft, (int)hop) > 0, op, ": unsupported n_fft / hop_length (", n_fft, ", ", hop,
              "): n_fft must be a power of two in [64, 2048], 1 <= hop <= n_fft and 31 hop + n_fft samples must fit 160 KB of LDS");
  TORCH_CHECK((size_t)dft.numel() * sizeof(float) == nws_loudness_dft_bytes((int)n_fft), op, ": dft does not belong to n_fft = ", n_fft);
}

// the clip maximum `loudness` normalises by: audio (B, N) -> (B) powers
Tensor loudness_peak_power(const Tensor& audio, const Tensor& dft, int64_t n_fft, int64_t hop) {
  check_dev(audio, "audio");
  check_dev(dft, "dft");
  check_same_device(audio, "audio", dft, "dft");
  TORCH_CHECK(audio.dim() == 2 && audio.size(0) >= 1, "loudness_peak_power: expected (B, N), got ", audio.sizes());
  const int64_t B = audio.size(0), N = audio.size(1);
  check_loudness_sizes("loudness_peak_power", dft, n_fft, hop);
  TORCH_CHECK(N > n_fft / 2, "loudness_peak_power: N = ", N, ": the reflect padding needs more than n_fft / 2 = ", n_fft / 2, " samples");
  const size_t nbytes = nws_loudness_workspace_bytes((int)B, (int)N, (int)n_fft, (int)hop);
  Launch L(audio);
  Tensor ws = at::empty({(int64_t)nbytes}, audio.options().dtype(at::kByte));
  Tensor out = at::empty({B}, audio.options());
  nws_check(nws_loudness_peak_power(audio.data_ptr<float>(), (int)B, (int)N, (int)n_fft, (int)hop, dft.data_ptr<float>(),
                                    out.data_ptr<float>(), ws.data_ptr(), nbytes, L.stream), "nws_loudness_peak_power");
  return out;
}

// ---- loudness stream (csrc/loudness_stream.hip): the state blob is a uint8 tensor on the device ----------------------------
size_t loudness_stream_bytes(const char* op, int64_t B, int64_t n_fft, int64_t hop) {
  const size_t nbytes = B >= 1 && B <= 65535 ? nws_loudness_stream_state_bytes((int)B, (int)n_fft, (int)hop) : 0;
  TORCH_CHECK(nbytes > 0, op, ": unsupported stream (B ", B, ", n_fft ", n_fft, ", hop ", hop,
              "): 1 <= B <= 65535, sizes the offline extractor serves and at most 256 hops in half a frame");
  return nbytes;
}

void loudness_stream_reset(Tensor& state, int64_t B, int64_t n_fft, int64_t hop, const Tensor& initial_power, bool track) {
  check_dev(state, "state", at::kByte);
  check_dev(initial_power, "initial_power");
  check_same_device(state, "state", initial_power, "initial_power");
  const size_t nbytes = loudness_stream_bytes("loudness_stream_reset", B, n_fft, hop);
  TORCH_CHECK((size_t)state.numel() >= nbytes, "loudness_stream_reset: state blob too small (expected ", nbytes, " bytes for B = ", B,
              ", got ", state.numel(), ")");
  TORCH_CHECK(initial_power.dim() == 1 && initial_power.size(0) == B, "loudness_stream_reset: initial_power: expected (", B, "), got ",
              initial_power.sizes());
  Launch L(state);
  nws_check(nws_loudness_stream_reset(state.data_ptr(), (size_t)state.numel(), (int)B, (int)n_fft, (int)hop,
                                      initial_power.data_ptr<float>(), track ? 1 : 0, L.stream), "nws_loudness_stream_reset");
}

// a releasing stream: tracking, M = floor_power, the floors kept behind the rows of the larger blob
void loudness_stream_reset_release(Tensor& state, int64_t B, int64_t n_fft, int64_t hop, const Tensor& floor_power) {
  check_dev(state, "state", at::kByte);
  check_dev(floor_power, "floor_power");
  check_same_device(state, "state", floor_power, "floor_power");
  loudness_stream_bytes("loudness_stream_reset_release", B, n_fft, hop);
  const size_t nbytes = nws_loudness_stream_release_state_bytes((int)B, (int)n_fft, (int)hop);
  TORCH_CHECK((size_t)state.numel() >= nbytes, "loudness_stream_reset_release: state blob too small (expected ", nbytes, " bytes for B = ", B,
              ", got ", state.numel(), ")");
  TORCH_CHECK(floor_power.dim() == 1 && floor_power.size(0) == B, "loudness_stream_reset_release: floor_power: expected (", B, "), got ",
              floor_power.sizes());
  Launch L(state);
  nws_check(nws_loudness_stream_reset_release(state.data_ptr(), (size_t)state.numel(), (int)B, (int)n_fft, (int)hop,
                                              floor_power.data_ptr<float>(), L.stream), "nws_loudness_stream_reset_release");
}

// the step of both ops.  with_release: loudness_stream_step_release, whose release_factor 1 is loudness_stream_step on either kind
// of blob; below 1 the blob is loudness_stream_reset_release's, hence track
void loudness_stream_step_impl(const char* op, bool with_release, Tensor& state, const Tensor& dft, int64_t n_fft, int64_t hop, int64_t lag,
                               double release_factor, bool track, const Tensor& chunk, int64_t n_seen, bool final, double amin,
                               double top_db, bool normalise, Tensor& loudness, Tensor& reference_power) {
  check_dev(chunk, "chunk");
  check_dev(loudness, "loudness");
  check_same_device(chunk, "chunk", loudness, "loudness");
  check_dev(state, "state", at::kByte);
  check_same_device(chunk, "chunk", state, "state");
  check_dev(dft, "dft");
  check_same_device(chunk, "chunk", dft, "dft");
  TORCH_CHECK(chunk.dim() == 2 && chunk.size(0) >= 1, op, ": expected a (B, n) chunk, got ", chunk.sizes());
  const int64_t B = chunk.size(0), n = chunk.size(1);
  const size_t nbytes = loudness_stream_bytes(op, B, n_fft, hop);
  const bool releasing = release_factor < 1.0;
  const size_t rbytes = nws_loudness_stream_release_state_bytes((int)B, (int)n_fft, (int)hop);
  if (with_release) {
    TORCH_CHECK(release_factor > 0.0 && release_factor <= 1.0, op, ": release_factor ", release_factor, " outside (0, 1]");
    TORCH_CHECK(!releasing || track, op, ": a release needs a tracked reference");
  }
  const size_t have = (size_t)state.numel();
  TORCH_CHECK(releasing ? have == rbytes : have == nbytes || (with_release && have == rbytes), op,
              ": state does not belong to a stream of B = ", B, " rows of this configuration (expected ", releasing ? rbytes : nbytes,
              " bytes, got ", state.numel(), ")");
  check_loudness_sizes(op, dft, n_fft, hop);
  TORCH_CHECK(lag >= 0 && lag <= 255, op, ": lag ", lag, " outside 0 .. 255");
  TORCH_CHECK(amin > 0.0 && top_db >= 0.0, op, ": amin must be positive and top_db non-negative");
  TORCH_CHECK(final || n >= 1, op, ": empty chunk (only a final step may carry no samples)");
  const int64_t max_chunk = nws_loudness_stream_max_chunk((int)n_fft, (int)hop);
  TORCH_CHECK(n <= max_chunk, op, ": a step takes at most ", max_chunk, " samples at this hop, got ", n);
  TORCH_CHECK(!final || n_seen + n > n_fft / 2, op, ": a stream of ", n_seen + n,
              " samples cannot end: the reflect padding needs more than n_fft / 2 = ", n_fft / 2);
  const int64_t before = n_seen >= 0 ? nws_loudness_stream_emitted(n_seen, (int)n_fft, (int)hop, (int)lag, 0) : -1;
  const int64_t after = n_seen >= 0 ? nws_loudness_stream_emitted(n_seen + n, (int)n_fft, (int)hop, (int)lag, final ? 1 : 0) : -1;
  TORCH_CHECK(before >= 0 && after >= 0, op, ": n_seen ", n_seen, " + ", n, " samples outside 0 .. 2^21 hops");
  const int64_t m = std::max<int64_t>(after - before, 1);
  const std::pair<const char*, const Tensor*> outs[2] = {{"loudness", &loudness}, {"reference_power", &reference_power}};
  for (const auto& [name, t] : outs) {
    TORCH_CHECK(t->is_cuda() && t->device() == chunk.device() && t->scalar_type() == at::kFloat && t->is_contiguous() && t->dim() == 2 &&
                    t->size(0) == B && t->size(1) == loudness.size(1) && t->size(1) >= m && t->size(1) <= INT32_MAX,
                op, ": ", name, ": expected a contiguous (", B, ", >= ", m,
                ") Float tensor on the chunk's GPU, the same width for both outputs, got ", t->sizes(), " ", t->scalar_type(), " on ",
                t->device());
  }
  Launch L(chunk);
  const size_t ws_bytes = nws_loudness_stream_workspace_bytes((int)B, (int)n, (int)n_fft, (int)hop, final ? 1 : 0);
  Tensor ws = at::empty({(int64_t)ws_bytes}, chunk.options().dtype(at::kByte));
  const float* x = n > 0 ? chunk.data_ptr<float>() : nullptr;
  if (with_release)
    nws_check(nws_loudness_stream_step_release(state.data_ptr(), (size_t)state.numel(), x, (int)B, (int)n, n_seen, (int)n_fft, (int)hop,
                                               (int)lag, (float)release_factor, track ? 1 : 0, dft.data_ptr<float>(), (float)amin,
                                               (float)top_db, normalise ? 1 : 0, final ? 1 : 0, loudness.data_ptr<float>(),
                                               reference_power.data_ptr<float>(), (int)loudness.size(1), ws.data_ptr(), ws_bytes,
                                               L.stream), "nws_loudness_stream_step_release");
  else
    nws_check(nws_loudness_stream_step(state.data_ptr(), (size_t)state.numel(), x, (int)B, (int)n, n_seen, (int)n_fft, (int)hop, (int)lag,
                                       dft.data_ptr<float>(), (float)amin, (float)top_db, normalise ? 1 : 0, final ? 1 : 0,
                                       loudness.data_ptr<float>(), reference_power.data_ptr<float>(), (int)loudness.size(1),
                                       ws.data_ptr(), ws_bytes, L.stream), "nws_loudness_stream_step");
}

void loudness_stream_step(Tensor& state, const Tensor& dft, int64_t n_fft, int64_t hop, int64_t lag, const Tensor& chunk, int64_t n_seen,
                          bool final, double amin, double top_db, bool normalise, Tensor& loudness, Tensor& reference_power) {
  loudness_stream_step_impl("loudness_stream_step", false, state, dft, n_fft, hop, lag, 1.0, true, chunk, n_seen, final, amin, top_db,
                            normalise, loudness, reference_power);
}

void loudness_stream_step_release(Tensor& state, const Tensor& dft, int64_t n_fft, int64_t hop, int64_t lag, double release_factor,
                                  bool track, const Tensor& chunk, int64_t n_seen, bool final, double amin, double top_db, bool normalise,
                                  Tensor& loudness, Tensor& reference_power) {
  loudness_stream_step_impl("loudness_stream_step_release", true, state, dft, n_fft, hop, lag, release_factor, track, chunk, n_seen,
                            final, amin, top_db, normalise, loudness, reference_power);
}

// the loudness stream's feature of a whole clip (csrc/loudness_causal.hip): audio (B, N) -> loudness, reference_power,
// frame_peak_power, (B, 1 + N / hop) each.  floor_power: (B) powers, the floors with track, the fixed references without
std::tuple<Tensor, Tensor, Tensor> loudness_causal(const Tensor& audio, const Tensor& dft, int64_t n_fft, int64_t hop, int64_t lag,
                                                   double release_factor, const Tensor& floor_power, bool track, double amin,
                                                   double top_db, bool normalise) {
  check_dev(audio, "audio");
  check_dev(dft, "dft");
  check_same_device(audio, "audio", dft, "dft");
  check_dev(floor_power, "floor_power");
  check_same_device(audio, "audio", floor_power, "floor_power");
  TORCH_CHECK(audio.dim() == 2 && audio.size(0) >= 1, "loudness_causal: expected (B, N), got ", audio.sizes());
  const int64_t B = audio.size(0), N = audio.size(1);
  check_loudness_sizes("loudness_causal", dft, n_fft, hop);
  TORCH_CHECK(N > n_fft / 2, "loudness_causal: N = ", N, ": the reflect padding needs more than n_fft / 2 = ", n_fft / 2, " samples");
  TORCH_CHECK(lag >= 0 && lag <= 255, "loudness_causal: lag ", lag, " outside 0 .. 255");
  TORCH_CHECK(amin > 0.0 && top_db >= 0.0, "loudness_causal: amin must be positive and top_db non-negative");
  TORCH_CHECK(release_factor > 0.0 && release_factor <= 1.0, "loudness_causal: release_factor ", release_factor, " outside (0, 1]");
  TORCH_CHECK(release_factor == 1.0 || track, "loudness_causal: a release needs a tracked reference");
  TORCH_CHECK(floor_power.dim() == 1 && floor_power.size(0) == B, "loudness_causal: floor_power: expected (", B, "), got ",
              floor_power.sizes());
  const size_t nbytes = B <= 65535 && N <= INT32_MAX ? nws_loudness_causal_workspace_bytes((int)B, (int)N, (int)n_fft, (int)hop) : 0;
  TORCH_CHECK(nbytes > 0, "loudness_causal: unsupported clip (B ", B, ", N ", N, ", n_fft ", n_fft, ", hop ", hop,
              "): 1 <= B <= 65535, sizes the loudness stream serves (at most 256 hops in half a frame) and at most 2^21 hops");
  Launch L(audio);
  Tensor ws = at::empty({(int64_t)nbytes}, audio.options().dtype(at::kByte));
  const int64_t T = nws_loudness_frames((int)N, (int)hop);
  Tensor loud = at::empty({B, T}, audio.options()), ref = at::empty({B, T}, audio.options()), peak = at::empty({B, T}, audio.options());
  nws_check(nws_loudness_causal(audio.data_ptr<float>(), (int)B, (int)N, (int)n_fft, (int)hop, dft.data_ptr<float>(), (int)lag,
                                (float)release_factor, floor_power.data_ptr<float>(), track ? 1 : 0, (float)amin, (float)top_db,
                                normalise ? 1 : 0, loud.data_ptr<float>(), ref.data_ptr<float>(), peak.data_ptr<float>(), ws.data_ptr(),
                                nbytes, L.stream), "nws_loudness_causal");
  return {loud, ref, peak};
}

// ---- pYIN F0 extractor (csrc/pyin.hip; data/utils/f0_extraction.py:61-92) ------------------------------------------------
struct PyinCfg {
  double sr, fmin, fmax;
  int fl, hop;
  int32_t dims[8];   // min_period, max_period, lags, n_bps, n_pitch_bins, window, W, shared blocks
  PyinCfg(double sample_rate, double fmin_, double fmax_, int64_t frame_length, int64_t hop_)
      : sr(sample_rate), fmin(fmin_), fmax(fmax_), fl((int)frame_length), hop((int)hop_) {
    TORCH_CHECK(nws_pyin_dims(sr, fmin, fmax, fl, hop, dims) == NWS_OK, "pyin: unsupported configuration (sample_rate ", sr,
                ", fmin ", fmin, ", fmax ", fmax, ", frame_length ", fl, ", hop ", hop,
                "): at most 512 lags (frame_length <= 1024), 1024 pitch bins and a transition window of 127; hop <= frame_length");
  }
  int lags() const { return dims[2]; }
  void check_table(const Tensor& table) const {
    check_dev(table, "table", at::kDouble);
    TORCH_CHECK((size_t)table.numel() * sizeof(double) == nws_pyin_table_bytes(sr, fmin, fmax, fl, hop),
                "pyin: table does not belong to this configuration");
  }
};

Tensor pyin_table(double sample_rate, double fmin, double fmax, int64_t frame_length, int64_t hop) {
  PyinCfg c(sample_rate, fmin, fmax, frame_length, hop);
  Tensor t = at::empty({(int64_t)(nws_pyin_table_bytes(c.sr, c.fmin, c.fmax, c.fl, c.hop) / sizeof(double))},
                       at::TensorOptions().dtype(at::kDouble));
  nws_check(nws_pyin_table(c.sr, c.fmin, c.fmax, c.fl, c.hop, t.data_ptr<double>()), "nws_pyin_table");
  return t;
}

Tensor pyin_cmnd(const Tensor& audio, double sample_rate, double fmin, double fmax, int64_t frame_length, int64_t hop) {
  check_dev(audio, "audio");
  TORCH_CHECK(audio.dim() == 2, "pyin_cmnd: expected (B, N), got ", audio.sizes());
  PyinCfg c(sample_rate, fmin, fmax, frame_length, hop);
  const int64_t B = audio.size(0), N = audio.size(1);
  Launch L(audio);
  Tensor yin = at::empty({B, nws_pyin_frames((int)N, c.hop), c.lags()}, audio.options());
  nws_check(nws_pyin_cmnd(audio.data_ptr<float>(), (int)B, (int)N, c.sr, c.fmin, c.fmax, c.fl, c.hop, yin.data_ptr<float>(), L.stream),
            "nws_pyin_cmnd");
  return yin;
}

std::tuple<Tensor, Tensor, Tensor, Tensor> pyin_observe(const Tensor& yin, const Tensor& table, double sample_rate, double fmin,
                                                        double fmax, int64_t frame_length, int64_t hop) {
  check_dev(yin, "yin");
  PyinCfg c(sample_rate, fmin, fmax, frame_length, hop);
  c.check_table(table);
  check_same_device(yin, "yin", table, "table");
  TORCH_CHECK(yin.dim() == 3 && yin.size(2) == c.lags(), "pyin_observe: expected (B, T, ", c.lags(), "), got ", yin.sizes());
  const int64_t B = yin.size(0), T = yin.size(1);
  Launch L(yin);
  Tensor cand_bin = at::empty({B, T, c.lags()}, yin.options().dtype(at::kInt));
  Tensor cand_prob = at::empty({B, T, c.lags()}, yin.options().dtype(at::kDouble));
  Tensor count = at::empty({B, T}, yin.options().dtype(at::kInt));
  Tensor voiced_prob = at::empty({B, T}, yin.options().dtype(at::kDouble));
  nws_check(nws_pyin_observe(yin.data_ptr<float>(), (int)B, (int)T, c.sr, c.fmin, c.fmax, c.fl, c.hop, table.data_ptr<double>(),
                             cand_bin.data_ptr<int32_t>(), cand_prob.data_ptr<double>(), count.data_ptr<int32_t>(),
                             voiced_prob.data_ptr<double>(), L.stream), "nws_pyin_observe");
  return {cand_bin, cand_prob, count, voiced_prob};
}

std::tuple<Tensor, Tensor> pyin_viterbi(const Tensor& cand_bin, const Tensor& cand_prob, const Tensor& count, const Tensor& voiced_prob,
                                        const Tensor& table, double sample_rate, double fmin, double fmax, int64_t frame_length,
                                        int64_t hop, bool fill_unvoiced, double fill_value) {
  check_dev(cand_bin, "cand_bin", at::kInt);
  check_dev(cand_prob, "cand_prob", at::kDouble);
  check_dev(count, "count", at::kInt);
  check_dev(voiced_prob, "voiced_prob", at::kDouble);
  PyinCfg c(sample_rate, fmin, fmax, frame_length, hop);
  c.check_table(table);
  check_same_device(cand_bin, "cand_bin", table, "table");
  check_same_device(cand_bin, "cand_bin", cand_prob, "cand_prob");
  check_same_device(cand_bin, "cand_bin", count, "count");
  check_same_device(cand_bin, "cand_bin", voiced_prob, "voiced_prob");
  TORCH_CHECK(cand_bin.dim() == 3 && cand_bin.size(2) == c.lags(), "pyin_viterbi: cand_bin: expected (B, T, ", c.lags(), "), got ",
              cand_bin.sizes());
  const int64_t B = cand_bin.size(0), T = cand_bin.size(1);
  TORCH_CHECK(cand_prob.sizes() == cand_bin.sizes() && count.dim() == 2 && count.size(0) == B && count.size(1) == T &&
                  voiced_prob.sizes() == count.sizes(), "pyin_viterbi: observation tensors disagree on (B, T, lags)");
  // the Viterbi part of the workspace does not depend on N beyond T: any N with 1 + N / hop = T
  const size_t nbytes = nws_pyin_workspace_bytes((int)B, (int)((T - 1) * c.hop + 1), c.sr, c.fmin, c.fmax, c.fl, c.hop);
  TORCH_CHECK(nbytes > 0, "pyin_viterbi: unsupported size");
  Launch L(cand_bin);
  Tensor ws = at::empty({(int64_t)nbytes}, cand_bin.options().dtype(at::kByte));
  Tensor states = at::empty({B, T}, cand_bin.options());
  Tensor f0 = at::empty({B, T}, cand_bin.options().dtype(at::kFloat));
  nws_check(nws_pyin_viterbi(cand_bin.data_ptr<int32_t>(), cand_prob.data_ptr<double>(), count.data_ptr<int32_t>(),
                             voiced_prob.data_ptr<double>(), (int)B, (int)T, c.sr, c.fmin, c.fmax, c.fl, c.hop,
                             table.data_ptr<double>(), fill_unvoiced ? 1 : 0, (float)fill_value, states.data_ptr<int32_t>(),
                             f0.data_ptr<float>(), ws.data_ptr(), nbytes, L.stream), "nws_pyin_viterbi");
  return {states, f0};
}

std::tuple<Tensor, Tensor, Tensor> pyin(const Tensor& audio, const Tensor& table, double sample_rate, double fmin, double fmax,
                                        int64_t frame_length, int64_t hop, bool fill_unvoiced, double fill_value) {
  check_dev(audio, "audio");
  TORCH_CHECK(audio.dim() == 2, "pyin: expected (B, N), got ", audio.sizes());
  PyinCfg c(sample_rate, fmin, fmax, frame_length, hop);
  c.check_table(table);
  check_same_device(audio, "audio", table, "table");
  const int64_t B = audio.size(0), N = audio.size(1);
  const size_t nbytes = nws_pyin_workspace_bytes((int)B, (int)N, c.sr, c.fmin, c.fmax, c.fl, c.hop);
  TORCH_CHECK(nbytes > 0, "pyin: unsupported size");
  const int64_t T = nws_pyin_frames((int)N, c.hop);
  Launch L(audio);
  Tensor ws = at::empty({(int64_t)nbytes}, audio.options().dtype(at::kByte));
  Tensor f0 = at::empty({B, T}, audio.options());
  Tensor voiced_prob = at::empty({B, T}, audio.options().dtype(at::kDouble));
  Tensor states = at::empty({B, T}, audio.options().dtype(at::kInt));
  nws_check(nws_pyin(audio.data_ptr<float>(), (int)B, (int)N, c.sr, c.fmin, c.fmax, c.fl, c.hop, table.data_ptr<double>(),
                     fill_unvoiced ? 1 : 0, (float)fill_value, f0.data_ptr<float>(), voiced_prob.data_ptr<double>(),
                     states.data_ptr<int32_t>(), ws.data_ptr(), nbytes, L.stream), "nws_pyin");
  return {f0, voiced_prob, states};
}

// ---- fixed-lag pYIN stream (csrc/pyin_stream.hip): the state blob is a uint8 tensor on the device ---------------------------
size_t pyin_stream_bytes(const char* op, const PyinCfg& c, int64_t B) {
  const size_t nbytes = B >= 1 && B <= 65535 ? nws_pyin_stream_state_bytes((int)B, c.sr, c.fmin, c.fmax, c.fl, c.hop) : 0;
  TORCH_CHECK(nbytes > 0, op, ": unsupported stream (B ", B, ", frame_length ", c.fl, ", hop ", c.hop,
              "): 1 <= B <= 65535 and at most 256 hops in half a frame");
  return nbytes;
}

void pyin_stream_reset(Tensor& state, int64_t B, double sample_rate, double fmin, double fmax, int64_t frame_length, int64_t hop) {
  check_dev(state, "state", at::kByte);
  PyinCfg c(sample_rate, fmin, fmax, frame_length, hop);
  const size_t nbytes = pyin_stream_bytes("pyin_stream_reset", c, B);
  TORCH_CHECK((size_t)state.numel() >= nbytes, "pyin_stream_reset: state blob too small (expected ", nbytes, " bytes for B = ", B,
              ", got ", state.numel(), ")");
  Launch L(state);
  nws_check(nws_pyin_stream_reset(state.data_ptr(), (size_t)state.numel(), (int)B, c.sr, c.fmin, c.fmax, c.fl, c.hop, L.stream),
            "nws_pyin_stream_reset");
}

void pyin_stream_step(Tensor& state, const Tensor& table, double sample_rate, double fmin, double fmax, int64_t frame_length,
                      int64_t hop, int64_t lag, const Tensor& chunk, int64_t n_seen, bool final, bool fill_unvoiced, double fill_value,
                      Tensor& f0, Tensor& voiced_prob, Tensor& states) {
  check_dev(chunk, "chunk");
  check_dev(f0, "f0");
  check_same_device(chunk, "chunk", f0, "f0");
  check_dev(state, "state", at::kByte);
  check_same_device(chunk, "chunk", state, "state");
  PyinCfg c(sample_rate, fmin, fmax, frame_length, hop);
  c.check_table(table);
  check_same_device(chunk, "chunk", table, "table");
  TORCH_CHECK(chunk.dim() == 2 && chunk.size(0) >= 1, "pyin_stream_step: expected a (B, n) chunk, got ", chunk.sizes());
  const int64_t B = chunk.size(0), n = chunk.size(1);
  const size_t nbytes = pyin_stream_bytes("pyin_stream_step", c, B);
  TORCH_CHECK((size_t)state.numel() == nbytes, "pyin_stream_step: state does not belong to a stream of B = ", B,
              " rows of this configuration (expected ", nbytes, " bytes, got ", state.numel(), ")");
  TORCH_CHECK(lag >= 0 && lag <= 255, "pyin_stream_step: lag ", lag, " outside 0 .. 255");
  TORCH_CHECK(final || n >= 1, "pyin_stream_step: empty chunk (only a final step may carry no samples)");
  const int64_t max_chunk = nws_pyin_stream_max_chunk(c.sr, c.fmin, c.fmax, c.fl, c.hop);
  TORCH_CHECK(n <= max_chunk, "pyin_stream_step: a step takes at most ", max_chunk, " samples at this hop, got ", n);
  TORCH_CHECK(!final || n_seen + n > c.fl / 2, "pyin_stream_step: a stream of ", n_seen + n,
              " samples cannot end: the reflect padding needs more than frame_length / 2 = ", c.fl / 2);
  const int64_t before = n_seen >= 0 ? nws_pyin_stream_emitted(n_seen, c.sr, c.fmin, c.fmax, c.fl, c.hop, (int)lag, 0) : -1;
  const int64_t after =
      n_seen >= 0 ? nws_pyin_stream_emitted(n_seen + n, c.sr, c.fmin, c.fmax, c.fl, c.hop, (int)lag, final ? 1 : 0) : -1;
  TORCH_CHECK(before >= 0 && after >= 0, "pyin_stream_step: n_seen ", n_seen, " + ", n, " samples outside 0 .. 2^21 hops");
  const int64_t m = std::max<int64_t>(after - before, 1);
  const std::tuple<const char*, const Tensor*, at::ScalarType> outs[3] = {
      {"f0", &f0, at::kFloat}, {"voiced_prob", &voiced_prob, at::kDouble}, {"states", &states, at::kInt}};
  for (const auto& [name, t, st] : outs) {
    TORCH_CHECK(t->is_cuda() && t->device() == chunk.device() && t->scalar_type() == st && t->is_contiguous() && t->dim() == 2 &&
                    t->size(0) == B && t->size(1) == f0.size(1) && t->size(1) >= m && t->size(1) <= INT32_MAX,
                "pyin_stream_step: ", name, ": expected a contiguous (", B, ", >= ", m, ") ", st,
                " tensor on the chunk's GPU, the same width for all three outputs, got ", t->sizes(), " ", t->scalar_type(), " on ",
                t->device());
  }
  Launch L(chunk);
  const size_t ws_bytes = nws_pyin_stream_workspace_bytes((int)B, (int)n, c.sr, c.fmin, c.fmax, c.fl, c.hop, final ? 1 : 0);
  Tensor ws = at::empty({(int64_t)ws_bytes}, chunk.options().dtype(at::kByte));
  nws_check(nws_pyin_stream_step(state.data_ptr(), (size_t)state.numel(), n > 0 ? chunk.data_ptr<float>() : nullptr, (int)B, (int)n,
                                 n_seen, c.sr, c.fmin, c.fmax, c.fl, c.hop, (int)lag, table.data_ptr<double>(), final ? 1 : 0,
                                 fill_unvoiced ? 1 : 0, (float)fill_value, f0.data_ptr<float>(), voiced_prob.data_ptr<double>(),
                                 states.data_ptr<int32_t>(), (int)f0.size(1), ws.data_ptr(), ws_bytes, L.stream),
            "nws_pyin_stream_step");
}


// ---- sample-rate converter (csrc/resample.hip; data/utils/preprocess_audio.py:65-66) ---------------------------------------
struct ResampleCfg {
  int sr_in, sr_out;
  int32_t dims[6];   // L, M, taps, left, right, step
  ResampleCfg(int64_t sr_in_, int64_t sr_out_) : sr_in((int)sr_in_), sr_out((int)sr_out_) {
    TORCH_CHECK(sr_in_ >= 1 && sr_out_ >= 1 && sr_in_ <= INT32_MAX && sr_out_ <= INT32_MAX &&
                    nws_resample_dims(sr_in, sr_out, dims) == NWS_OK,
                "resample: unsupported rates ", sr_in_, " -> ", sr_out_, ": integers >= 1 whose weight bank (sr_out / gcd rows) stays "
                "below 64 MB");
  }
};

Tensor resample_bank(int64_t sr_in, int64_t sr_out) {
  ResampleCfg c(sr_in, sr_out);
  Tensor bank = at::empty({(int64_t)c.dims[0], (int64_t)c.dims[2]}, at::TensorOptions().dtype(at::kFloat));
  nws_check(nws_resample_bank(c.sr_in, c.sr_out, bank.data_ptr<float>()), "nws_resample_bank");
  return bank;
}

Tensor resample(const Tensor& audio, const Tensor& bank, int64_t sr_in, int64_t sr_out) {
  check_dev(audio, "audio");
  check_dev(bank, "bank");
  check_same_device(audio, "audio", bank, "bank");
  ResampleCfg c(sr_in, sr_out);
  TORCH_CHECK(audio.dim() == 2 && audio.size(0) >= 1 && audio.size(1) <= INT32_MAX, "resample: expected (B, N), got ", audio.sizes());
  TORCH_CHECK(bank.dim() == 2 && bank.size(0) == c.dims[0] && bank.size(1) == c.dims[2],
              "resample: bank does not belong to these rates (expected (", c.dims[0], ", ", c.dims[2], "), got ", bank.sizes(), ")");
  const int64_t B = audio.size(0), N = audio.size(1), n_out = nws_resample_length(N, c.sr_in, c.sr_out);
  TORCH_CHECK(n_out >= 1 && B <= INT32_MAX, "resample: ", N, " samples at ", sr_in, " Hz give no sample at ", sr_out, " Hz");
  Launch L(audio);
  Tensor y = at::empty({B, n_out}, audio.options());
  nws_check(nws_resample(audio.data_ptr<float>(), (int)B, (int)N, c.sr_in, c.sr_out, bank.data_ptr<float>(), y.data_ptr<float>(),
                         L.stream), "nws_resample");
  return y;
}

// ---- streaming sample-rate converter (csrc/resample_stream.hip): the state blob is a uint8 tensor on the device -------------
size_t resample_stream_bytes(const char* op, const ResampleCfg& c, int64_t B) {
  const size_t nbytes = B >= 1 && B <= 65535 ? nws_resample_stream_state_bytes((int)B, c.sr_in, c.sr_out) : 0;
  TORCH_CHECK(nbytes > 0, op, ": unsupported stream (B ", B, ", ", c.sr_in, " -> ", c.sr_out, " Hz): 1 <= B <= 65535, and the ",
              c.dims[2] - 1, " samples of history and ", c.dims[4], " of look-ahead must leave room for a chunk in 64 KB of LDS");
  return nbytes;
}

void resample_stream_reset(Tensor& state, int64_t B, int64_t sr_in, int64_t sr_out) {
  check_dev(state, "state", at::kByte);
  ResampleCfg c(sr_in, sr_out);
  const size_t nbytes = resample_stream_bytes("resample_stream_reset", c, B);
  TORCH_CHECK((size_t)state.numel() >= nbytes, "resample_stream_reset: state blob too small (expected ", nbytes, " bytes for B = ", B,
              ", got ", state.numel(), ")");
  Launch L(state);
  nws_check(nws_resample_stream_reset(state.data_ptr(), (size_t)state.numel(), (int)B, c.sr_in, c.sr_out, L.stream),
            "nws_resample_stream_reset");
}

void resample_stream_step(Tensor& state, const Tensor& bank, int64_t sr_in, int64_t sr_out, const Tensor& chunk, bool final,
                          Tensor& out) {
  check_dev(chunk, "chunk");
  check_dev(bank, "bank");
  check_dev(out, "out");
  check_dev(state, "state", at::kByte);
  check_same_device(chunk, "chunk", bank, "bank");
  check_same_device(chunk, "chunk", out, "out");
  check_same_device(chunk, "chunk", state, "state");
  ResampleCfg c(sr_in, sr_out);
  TORCH_CHECK(chunk.dim() == 2 && chunk.size(0) >= 1, "resample_stream_step: expected a (B, n) chunk, got ", chunk.sizes());
  TORCH_CHECK(bank.dim() == 2 && bank.size(0) == c.dims[0] && bank.size(1) == c.dims[2],
              "resample_stream_step: bank does not belong to these rates (expected (", c.dims[0], ", ", c.dims[2], "), got ",
              bank.sizes(), ")");
  const int64_t B = chunk.size(0), n = chunk.size(1);
  const size_t nbytes = resample_stream_bytes("resample_stream_step", c, B);
  TORCH_CHECK((size_t)state.numel() == nbytes, "resample_stream_step: state does not belong to a stream of B = ", B, " rows at these "
              "rates (expected ", nbytes, " bytes, got ", state.numel(), ")");
  const int64_t max_chunk = nws_resample_stream_max_chunk(c.sr_in, c.sr_out);
  TORCH_CHECK(final || n >= 1, "resample_stream_step: empty chunk (only a final step may carry no samples)");
  TORCH_CHECK(n <= max_chunk, "resample_stream_step: a step takes at most ", max_chunk, " samples at these rates, got ", n);
  const int64_t max_out = nws_resample_stream_max_out((int)n, c.sr_in, c.sr_out, final ? 1 : 0);
  TORCH_CHECK(out.dim() == 2 && out.size(0) == B && out.size(1) >= max_out && out.size(1) <= INT32_MAX,
              "resample_stream_step: out: expected (", B, ", >= ", max_out, ") for a ", final ? "final " : "", "step of ", n,
              " samples, got ", out.sizes());
  Launch L(chunk);
  nws_check(nws_resample_stream_step(state.data_ptr(), (size_t)state.numel(), n > 0 ? chunk.data_ptr<float>() : nullptr, (int)B,
                                     (int)n, c.sr_in, c.sr_out, bank.data_ptr<float>(), final ? 1 : 0, out.data_ptr<float>(),
                                     (int)out.size(1), L.stream), "nws_resample_stream_step");
}

// ---- MFCC feature (csrc/mfcc.hip; data/utils/mfcc_extraction.py:7-13) ------------------------------------------------------
struct MfccCfg {
  double sr;
  int n_fft, n_mfcc, n_mels;
  int32_t dims[8];   // bins, n_mels, n_mfcc, jpad, nnz, off_w, off_dct, words
  MfccCfg(double sample_rate, int64_t n_fft_, int64_t n_mfcc_, int64_t n_mels_)
      : sr(sample_rate), n_fft((int)n_fft_), n_mfcc((int)n_mfcc_), n_mels((int)n_mels_) {
    TORCH_CHECK(n_fft_ <= INT32_MAX && n_mfcc_ <= INT32_MAX && n_mels_ <= INT32_MAX &&
                    nws_mfcc_dims(sr, n_fft, n_mfcc, n_mels, dims) == NWS_OK,
                "mfcc: unsupported configuration (sample_rate ", sr, ", n_fft ", n_fft_, ", n_mfcc ", n_mfcc_, ", n_mels ", n_mels_,
                "): sample_rate > 0, n_fft a power of two in [64, 2048], 1 <= n_mfcc <= n_mels <= 1024");
  }
};

Tensor mfcc_table(double sample_rate, int64_t n_fft, int64_t n_mfcc, int64_t n_mels) {
  MfccCfg c(sample_rate, n_fft, n_mfcc, n_mels);
  Tensor t = at::empty({(int64_t)c.dims[7]}, at::TensorOptions().dtype(at::kFloat));
  nws_check(nws_mfcc_table(c.sr, c.n_fft, c.n_mfcc, c.n_mels, t.data_ptr<float>()), "nws_mfcc_table");
  return t;
}

// extract_mfcc: audio (B, N) -> (B, n_mfcc, 1 + N / hop)
Tensor mfcc(const Tensor& audio, const Tensor& dft, const Tensor& table, double sample_rate, int64_t n_fft, int64_t hop,
            int64_t n_mfcc, int64_t n_mels) {
  check_dev(audio, "audio");
  check_dev(dft, "dft");
  check_dev(table, "table");
  check_same_device(audio, "audio", dft, "dft");
  check_same_device(audio, "audio", table, "table");
  MfccCfg c(sample_rate, n_fft, n_mfcc, n_mels);
  TORCH_CHECK(audio.dim() == 2 && audio.size(0) >= 1 && audio.size(1) <= INT32_MAX, "mfcc: expected (B, N), got ", audio.sizes());
  const int64_t B = audio.size(0), N = audio.size(1);
  TORCH_CHECK(table.numel() == c.dims[7], "mfcc: table does not belong to this configuration (expected ", c.dims[7],
              " words of mfcc_table, got ", table.numel(), ")");
  TORCH_CHECK((size_t)dft.numel() * sizeof(float) == nws_loudness_dft_bytes(c.n_fft), "mfcc: dft does not belong to n_fft = ", n_fft);
  const size_t nbytes = B <= 65535 && hop <= INT32_MAX ? nws_mfcc_workspace_bytes((int)B, (int)N, c.n_fft, (int)hop, c.n_mels) : 0;
  TORCH_CHECK(nbytes > 0 && N > c.n_fft / 2, "mfcc: unsupported size (B ", B, ", N ", N, ", n_fft ", n_fft, ", hop_length ", hop,
              "): 1 <= hop <= n_fft, 31 hop + n_fft samples must fit 160 KB of LDS, N > n_fft / 2, B <= 65535");
  Launch L(audio);
  Tensor ws = at::empty({(int64_t)nbytes}, audio.options().dtype(at::kByte));
  Tensor out = at::empty({B, (int64_t)c.n_mfcc, (int64_t)nws_loudness_frames((int)N, (int)hop)}, audio.options());
  nws_check(nws_mfcc(audio.data_ptr<float>(), (int)B, (int)N, c.sr, c.n_fft, (int)hop, c.n_mfcc, c.n_mels, dft.data_ptr<float>(),
                     table.data_ptr<float>(), out.data_ptr<float>(), ws.data_ptr(), nbytes, L.stream), "nws_mfcc");
  return out;
}

// ---- multi-resolution STFT loss (csrc/stft_loss.hip; models/neural_waveshaping.py:93, 104-112 of the reference) ----------
// the constant operand of one resolution, on the current device
Tensor stft_loss_dft(int64_t n_fft, int64_t win_length) {
  const size_t nbytes =
      std::max(std::abs(n_fft), std::abs(win_length)) <= INT32_MAX ? nws_stft_loss_dft_bytes((int)n_fft, (int)win_length) : 0;
  TORCH_CHECK(nbytes > 0, "stft_loss: unsupported resolution (n_fft ", n_fft, ", win_length ", win_length,
              "): n_fft a power of two in [64, 2048], 1 <= win_length <= n_fft");
  Tensor dft = at::empty({(int64_t)(nbytes / sizeof(float))}, at::TensorOptions().dtype(at::kFloat).device(at::kCUDA));
  Launch L(dft);
  nws_check(nws_stft_loss_dft_matrix((int)n_fft, (int)win_length, dft.data_ptr<float>(), L.stream), "nws_stft_loss_dft_matrix");
  return dft;
}

// the argument checks stft_loss and stft_loss_grad share; ok == false: a size does not fit an int (reported as unsupported)
struct StftSizes {
  int64_t B, N;
  size_t R;
  bool ok;
  int nf[NWS_STFT_LOSS_MAX_RES], hp[NWS_STFT_LOSS_MAX_RES], wl[NWS_STFT_LOSS_MAX_RES];
  const float* dp[NWS_STFT_LOSS_MAX_RES];
};
StftSizes stft_sizes(const char* op, const Tensor& x, const Tensor& y, at::TensorList dfts, at::IntArrayRef n_ffts, at::IntArrayRef hops,
                     at::IntArrayRef win_lengths) {
  check_dev(x, "x");
  check_dev(y, "y");
  check_same_device(x, "x", y, "y");
  TORCH_CHECK(x.dim() == 2 && x.sizes() == y.sizes(), op, ": expected x and y of one shape (B, N), got ", x.sizes(), " and ", y.sizes());
  StftSizes s;
  s.R = n_ffts.size();
  const size_t R = s.R;
  TORCH_CHECK(R >= 1 && R <= NWS_STFT_LOSS_MAX_RES && hops.size() == R && win_lengths.size() == R && dfts.size() == R, op,
              ": 1 to 8 resolutions, one n_fft, hop, win_length and operand each (got ", R, ", ", hops.size(), ", ", win_lengths.size(),
              ", ", dfts.size(), ")");
  s.B = x.size(0), s.N = x.size(1);
  s.ok = s.B >= 1 && s.B <= 65535 && s.N <= INT32_MAX;
  for (size_t r = 0; r < R; ++r)
    s.ok = s.ok && std::abs(n_ffts[r]) <= INT32_MAX && std::abs(hops[r]) <= INT32_MAX && std::abs(win_lengths[r]) <= INT32_MAX;
  for (size_t r = 0; s.ok && r < R; ++r) {
    s.nf[r] = (int)n_ffts[r], s.hp[r] = (int)hops[r], s.wl[r] = (int)win_lengths[r];
    check_dev(dfts[r], "dfts");
    check_same_device(x, "x", dfts[r], "dfts");
    const size_t nbytes = nws_stft_loss_dft_bytes(s.nf[r], s.wl[r]);
    TORCH_CHECK(nbytes > 0 && (size_t)dfts[r].numel() * sizeof(float) == nbytes, op, ": dfts[", r, "] does not belong to n_fft = ",
                s.nf[r], ", win_length = ", s.wl[r], " (n_fft: a power of two in [64, 2048], 1 <= win_length <= n_fft)");
    s.dp[r] = dfts[r].data_ptr<float>();
  }
  return s;
}
#define STFT_CHECK_SUPPORTED(op, nbytes, s, n_ffts, hops)                                                                              \
  TORCH_CHECK(nbytes > 0, op, ": unsupported size (B ", s.B, ", N ", s.N, ", n_ffts ", n_ffts, ", hops ", hops,                        \
              "): N > n_fft / 2 (reflect padding), hop >= 1, the two signal tiles of 31 hop + n_fft samples must fit 160 KB of LDS " \
              "(n_fft 2048: hop <= 589), B <= 65535")

// x, y (B, N) -> [loss (0-dim), components (R, 3) = (sc_r, log_r, lin_r)]
std::vector<Tensor> stft_loss(const Tensor& x, const Tensor& y, at::TensorList dfts, at::IntArrayRef n_ffts, at::IntArrayRef hops,
                              at::IntArrayRef win_lengths, double w_sc, double w_log_mag, double w_lin_mag, double eps) {
  const StftSizes s = stft_sizes("stft_loss", x, y, dfts, n_ffts, hops, win_lengths);
  const int B = (int)s.B, N = (int)s.N, R = (int)s.R;
  const size_t nbytes = s.ok ? nws_stft_loss_workspace_bytes(B, N, R, s.nf, s.hp) : 0;
  STFT_CHECK_SUPPORTED("stft_loss", nbytes, s, n_ffts, hops);
  Launch L(x);
  Tensor ws = at::empty({(int64_t)nbytes}, x.options().dtype(at::kByte));
  Tensor out = at::empty({(int64_t)(1 + 3 * R)}, x.options());
  nws_check(nws_stft_loss(x.data_ptr<float>(), y.data_ptr<float>(), B, N, R, s.nf, s.hp, s.wl, s.dp, (float)w_sc, (float)w_log_mag,
                          (float)w_lin_mag, (float)eps, out.data_ptr<float>(), ws.data_ptr(), nbytes, L.stream),
            "nws_stft_loss");
  return {out[0], out.slice(0, 1).view({(int64_t)R, 3})};
}

// dL/dx of stft_loss(x, y, ...) (csrc/stft_grad.hip): x, y (B, N) -> (B, N).  No gradient for the target y.
Tensor stft_loss_grad(const Tensor& x, const Tensor& y, at::TensorList dfts, at::IntArrayRef n_ffts, at::IntArrayRef hops,
                      at::IntArrayRef win_lengths, double w_sc, double w_log_mag, double w_lin_mag, double eps) {
  const StftSizes s = stft_sizes("stft_loss_grad", x, y, dfts, n_ffts, hops, win_lengths);
  const int B = (int)s.B, N = (int)s.N, R = (int)s.R;
  const size_t nbytes = s.ok ? nws_stft_grad_workspace_bytes(B, N, R, s.nf, s.hp, s.wl) : 0;
  STFT_CHECK_SUPPORTED("stft_loss_grad", nbytes, s, n_ffts, hops);
  Launch L(x);
  Tensor ws = at::empty({(int64_t)nbytes}, x.options().dtype(at::kByte));
  Tensor grad = at::empty({s.B, s.N}, x.options());
  nws_check(nws_stft_grad(x.data_ptr<float>(), y.data_ptr<float>(), B, N, R, s.nf, s.hp, s.wl, s.dp, (float)w_sc, (float)w_log_mag,
                          (float)w_lin_mag, (float)eps, grad.data_ptr<float>(), ws.data_ptr(), nbytes, L.stream),
            "nws_stft_grad");
  return grad;
}

// ---- runtime-size path (csrc/generic.hip): any gin configuration of the reference --------------------------------------
template <class T>
const T* struct_of(const Tensor& desc, const char* name) {
  TORCH_CHECK(desc.device().is_cpu() && desc.scalar_type() == at::kByte && desc.is_contiguous() && (size_t)desc.numel() == sizeof(T),
              name, ": expected a contiguous CPU uint8 tensor of ", sizeof(T), " bytes, got ", desc.sizes());
  return reinterpret_cast<const T*>(desc.data_ptr());
}

Tensor forward_generic(const Tensor& gdesc, const Tensor& f0, const Tensor& control, const Tensor& phase_u, const Tensor& rand_phase,
                       const Tensor& noise, const OptTensor& plan_t, const OptTensor& tables, const OptTensor& spectrum,
                       Tensor& reverb_workspace, Tensor& workspace, double sample_rate) {
  const NwsGenericModel* m = struct_of<NwsGenericModel>(gdesc, "gdesc");
  int64_t B, C, T;
  check_inputs(f0, control, B, C, T);
  check_dev(phase_u, "phase_u");
  check_dev(rand_phase, "rand_phase");
  check_dev(noise, "noise");
  check_same_device(f0, "f0", phase_u, "phase_u");
  check_same_device(f0, "f0", noise, "noise");
  check_same_device(f0, "f0", rand_phase, "osc.rand_phase");
  check_dev(workspace, "workspace", at::kByte);
  check_dev(reverb_workspace, "reverb_workspace", at::kByte);
  check_same_device(f0, "f0", workspace, "workspace");
  TORCH_CHECK(m->hop > 0 && m->n_harmonics > 0, "gdesc: not a NwsGenericModel");
  TORCH_CHECK(phase_u.numel() == m->n_harmonics && rand_phase.numel() == m->n_harmonics, "phase_u / rand_phase: expected ",
              m->n_harmonics, " elements");
  const int64_t N = T * m->hop;
  TORCH_CHECK(noise.numel() == N - 1, "noise: expected ", N - 1, " elements, got ", noise.sizes());
  TORCH_CHECK((size_t)workspace.numel() >= nws_forward_generic_workspace_bytes(m, (int)B, (int)T), "workspace too small");
  NwsReverbPlan plan{};
  const bool fft = plan_t.has_value();
  if (fft) {
    TORCH_CHECK(tables.has_value() && spectrum.has_value(), "forward_generic: plan without tables / spectrum");
    plan = plan_of(*plan_t);
    check_dev(*tables, "reverb_tables");
    check_dev(*spectrum, "reverb_spectrum");
    check_reverb_buffers(plan, *tables, *spectrum);
    TORCH_CHECK(nws_reverb_plan_serves(&plan, (int)N, m->ir_len + 1), "forward_generic: the reverb plan was not made for ", N, " samples");
    TORCH_CHECK((size_t)reverb_workspace.numel() >= nws_reverb_workspace_bytes(&plan, (int)B), "reverb workspace too small");
  }
  Launch L(f0);
  Tensor out = at::empty({B, N}, f0.options());
  nws_check(nws_forward_generic(m, f0.data_ptr<float>(), control.data_ptr<float>(), (int)B, (int)C, (int)T, (float)sample_rate,
                                phase_u.data_ptr<float>(), rand_phase.data_ptr<float>(), noise.data_ptr<float>(),
                                fft ? &plan : nullptr, fft ? tables->data_ptr() : nullptr, fft ? spectrum->data_ptr() : nullptr,
                                fft ? reverb_workspace.data_ptr() : nullptr, fft ? (size_t)reverb_workspace.numel() : 0,
                                out.data_ptr<float>(), workspace.data_ptr(), (size_t)workspace.numel(), L.stream),
            "nws_forward_generic");
  return out;
}

// nn.GRU(C_in -> H, batch_first) over control[:, 0:C_in] of (B, C_total, T): -> (out (B, T, H), hT (B, H))
std::tuple<Tensor, Tensor> g_gru(const Tensor& w_ih, const Tensor& w_hh, const Tensor& b_ih, const Tensor& b_hh, const Tensor& control,
                                 const OptTensor& h0) {
  check_dev(control, "control");
  for (const Tensor* t : {&w_ih, &w_hh, &b_ih, &b_hh}) {
    check_dev(*t, "gru parameter");
    check_same_device(control, "control", *t, "the GRU's parameters");
  }
  TORCH_CHECK(control.dim() == 3 && w_hh.dim() == 2 && w_ih.dim() == 2, "g_gru: control (B, C, T), weight_ih (3H, C_in), weight_hh (3H, H)");
  const int64_t B = control.size(0), Ct = control.size(1), T = control.size(2), H = w_hh.size(1), Cin = w_ih.size(1);
  TORCH_CHECK(w_hh.size(0) == 3 * H && w_ih.size(0) == 3 * H && b_ih.numel() == 3 * H && b_hh.numel() == 3 * H, "g_gru: inconsistent GRU parameter shapes");
  TORCH_CHECK(Ct >= Cin && T >= 1, "g_gru: control has ", Ct, " channels, the GRU takes ", Cin);
  if (h0.has_value()) {
    check_dev(*h0, "h0");
    TORCH_CHECK(h0->numel() == B * H, "h0: expected (", B, ", ", H, ")");
  }
  Launch L(control);
  Tensor out = at::empty({B, T, H}, control.options());
  Tensor hT = at::empty({B, H}, control.options());
  const size_t nb = nws_g_gru_workspace_bytes((int)H);
  Tensor ws = at::empty({(int64_t)nb}, control.options().dtype(at::kByte));
  nws_check(nws_g_gru(w_ih.data_ptr<float>(), w_hh.data_ptr<float>(), b_ih.data_ptr<float>(), b_hh.data_ptr<float>(),
                      control.data_ptr<float>(), (int)B, (int)Ct, (int)Cin, (int)H, (int)T, fptr(h0), out.data_ptr<float>(),
                      hT.data_ptr<float>(), ws.data_ptr(), nb, L.stream), "nws_g_gru");
  return {out, hT};
}

// HarmonicOscillator.forward for any n_harmonics / length: f0_up (B, N) -> (B, K, N)
Tensor g_oscillator(const Tensor& f0_up, const Tensor& phase_u, const Tensor& rand_phase, double sample_rate) {
  check_dev(f0_up, "f0");
  check_dev(phase_u, "phase_u");
  check_dev(rand_phase, "rand_phase");
  check_same_device(f0_up, "f0", phase_u, "phase_u");
  check_same_device(f0_up, "f0", rand_phase, "rand_phase");
  TORCH_CHECK(f0_up.dim() == 2 && f0_up.size(1) > 0, "HarmonicOscillator: expected f0 of shape (B, N), got ", f0_up.sizes());
  const int64_t B = f0_up.size(0), N = f0_up.size(1), K = phase_u.numel();
  TORCH_CHECK(rand_phase.numel() == K && K > 0, "phase_u / rand_phase disagree");
  Launch L(f0_up);
  Tensor phase = at::empty_like(f0_up);
  nws_check(nws_g_phase(nullptr, f0_up.data_ptr<float>(), (int)B, (int)N, 1, (float)sample_rate, nullptr, phase.data_ptr<float>(),
                        L.stream), "nws_g_phase");
  Tensor out = at::empty({B, K, N}, f0_up.options());
  nws_check(nws_g_oscillator(f0_up.data_ptr<float>(), phase.data_ptr<float>(), phase_u.data_ptr<float>(), rand_phase.data_ptr<float>(),
                             (int)K, (int)B, (int)N, (float)sample_rate, out.data_ptr<float>(), L.stream), "nws_g_oscillator");
  return out;
}

// F.upsample(x, T * hop, mode="linear") on the last axis of (..., T)
Tensor g_upsample(const Tensor& x, int64_t hop) {
  check_dev(x, "x");
  TORCH_CHECK(x.dim() >= 1 && x.size(-1) >= 1 && hop >= 1, "upsample: expected (..., T) and hop >= 1");
  const int64_t T = x.size(-1), rows = x.numel() / T;
  Launch L(x);
  auto shape = x.sizes().vec();
  shape.back() = T * hop;
  Tensor y = at::empty(shape, x.options());
  nws_check(nws_g_upsample(x.data_ptr<float>(), rows, (int)T, (int)hop, y.data_ptr<float>(), L.stream), "nws_g_upsample");
  return y;
}

Tensor g_conv1x1(const Tensor& x, const Tensor& w, const OptTensor& bias) {
  check_dev(x, "x");
  check_dev(w, "weight");
  check_same_device(x, "x", w, "weight");
  TORCH_CHECK(x.dim() == 3 && w.dim() >= 2 && w.size(1) == x.size(1) && w.numel() == w.size(0) * w.size(1),
              "conv1x1: x (B, Cin, N), weight (Cout, Cin[, 1]); got ", x.sizes(), " / ", w.sizes());
  if (bias.has_value()) {
    check_dev(*bias, "bias");
    TORCH_CHECK(bias->numel() == w.size(0), "conv1x1: bias ", bias->sizes());
  }
  Launch L(x);
  Tensor y = at::empty({x.size(0), w.size(0), x.size(2)}, x.options());
  nws_check(nws_g_conv1x1(x.data_ptr<float>(), w.data_ptr<float>(), fptr(bias), (int)x.size(0), (int)x.size(1), (int)w.size(0),
                          (int)x.size(2), y.data_ptr<float>(), L.stream), "nws_g_conv1x1");
  return y;
}

Tensor g_shaper_apply(const Tensor& sdesc, const Tensor& x) {
  const NwsShaperDesc* d = struct_of<NwsShaperDesc>(sdesc, "sdesc");
  check_dev(x, "x");
  TORCH_CHECK(x.dim() == 3 && x.size(1) == d->n_shapers, "expected (B, ", d->n_shapers, ", N), got ", x.sizes());
  Launch L(x);
  Tensor y = at::empty_like(x);
  nws_check(nws_g_shaper_apply(d, x.data_ptr<float>(), x.size(0) * x.size(1), x.size(2), y.data_ptr<float>(), L.stream),
            "nws_g_shaper_apply");
  return y;
}

Tensor g_shaper_table(const Tensor& sdesc, const Tensor& like, int64_t size, double tmin, double tmax) {
  const NwsShaperDesc* d = struct_of<NwsShaperDesc>(sdesc, "sdesc");
  check_dev(like, "shaping_fn.input_scale");
  TORCH_CHECK(size >= 2 && tmax > tmin, "FastNEWT: need table_size >= 2 and table_max > table_min");
  Launch L(like);
  Tensor table = at::empty({(int64_t)d->n_shapers, size}, like.options());
  nws_check(nws_g_shaper_table(d, (int)size, (float)tmin, (float)tmax, table.data_ptr<float>(), L.stream), "nws_g_shaper_table");
  return table;
}

// NEWT.forward / FastNEWT.forward for any sizes: exciter (B, S, N), film (B, 4S, T) -> (B, O, N)
Tensor g_newt_apply(const Tensor& sdesc, const Tensor& exciter, const Tensor& film, const Tensor& mix_w, const Tensor& mix_b) {
  const NwsShaperDesc* d = struct_of<NwsShaperDesc>(sdesc, "sdesc");
  check_dev(exciter, "exciter");
  check_dev(film, "film_params");
  check_dev(mix_w, "mixer weight");
  check_dev(mix_b, "mixer bias");
  check_same_device(exciter, "exciter", film, "control embedding");
  check_same_device(exciter, "exciter", mix_w, "newt.mixer");
  const int64_t S = d->n_shapers;
  TORCH_CHECK(exciter.dim() == 3 && exciter.size(1) == S, "NEWT: expected an exciter of shape (B, ", S, ", N), got ", exciter.sizes());
  TORCH_CHECK(film.dim() == 3 && film.size(1) == 4 * S && film.size(0) == exciter.size(0), "NEWT: expected FiLM parameters of shape (B, ",
              4 * S, ", T), got ", film.sizes());
  const int64_t B = exciter.size(0), N = exciter.size(2), T = film.size(2);
  TORCH_CHECK(T > 0 && N % T == 0, "NEWT: ", N, " samples are not a whole multiple of ", T, " control frames");
  TORCH_CHECK(mix_w.numel() % S == 0 && mix_b.numel() == mix_w.numel() / S, "NEWT: mixer weight ", mix_w.sizes(), " / bias ", mix_b.sizes());
  const int64_t O = mix_w.numel() / S;
  Launch L(exciter);
  Tensor shaped = at::empty_like(exciter);
  nws_check(nws_g_film_shaper(d, exciter.data_ptr<float>(), film.data_ptr<float>(), (int)B, (int)T, (int)(N / T),
                              shaped.data_ptr<float>(), L.stream), "nws_g_film_shaper");
  Tensor out = at::empty({B, O, N}, exciter.options());
  nws_check(nws_g_conv1x1(shaped.data_ptr<float>(), mix_w.data_ptr<float>(), mix_b.data_ptr<float>(), (int)B, (int)S, (int)O, (int)N,
                          out.data_ptr<float>(), L.stream), "nws_g_conv1x1");
  return out;
}

// The backward of g_newt_apply with one output channel for grad_out = dL/d(out) (B, 1, N) (csrc/g_newt_grad.hip):
// [grad_film (B, 4S, T)], then grad_exciter (B, S, N) when wanted, then with want_params the 2 D + 3 parameter gradients in the
// shapes of their parameters: input_scale, net.{2l}.weight and net.{2l}.bias for l < D, mixer.0.weight, mixer.0.bias.  Nothing was
// saved by the forward; the workspace comes from torch's allocator.
std::vector<Tensor> g_newt_grad(const Tensor& sdesc, const Tensor& exciter, const Tensor& film, const Tensor& grad_out, const Tensor& mix_w,
                                const Tensor& mix_b, bool want_exciter, bool want_params) {
  const NwsShaperDesc* d = struct_of<NwsShaperDesc>(sdesc, "sdesc");
  check_dev(exciter, "exciter");
  check_dev(film, "film_params");
  check_dev(grad_out, "grad_out");
  check_dev(mix_w, "mixer weight");
  check_dev(mix_b, "mixer bias");
  check_same_device(exciter, "exciter", film, "control embedding");
  check_same_device(exciter, "exciter", grad_out, "grad_out");
  check_same_device(exciter, "exciter", mix_w, "newt.mixer");
  const int64_t S = d->n_shapers, W = d->width, D = d->depth;
  TORCH_CHECK(exciter.dim() == 3, "NEWT: expected an exciter of shape (B, ", S, ", N), got ", exciter.sizes());
  const int64_t B = exciter.size(0), N = exciter.size(2);
  TORCH_CHECK(film.dim() == 3, "NEWT: expected FiLM parameters of shape (B, ", 4 * S, ", T), got ", film.sizes());
  const int64_t T = film.size(2);
  TORCH_CHECK(exciter.size(1) == S && film.size(0) == B && film.size(1) == 4 * S && N == T * NWS_HOP, "NEWT: exciter ", exciter.sizes(),
              " and FiLM parameters ", film.sizes(), " disagree (", S, " shapers, hop ", NWS_HOP, ")");
  TORCH_CHECK(B >= 1 && T >= 1, "g_newt_grad: need at least one utterance and one frame");
  TORCH_CHECK(grad_out.numel() == B * N && grad_out.size(0) == B, "g_newt_grad: grad_out ", grad_out.sizes(), " is not (", B, ", 1, ", N, ")");
  TORCH_CHECK(d->lut == nullptr, "g_newt_grad: the lookup table has no backward");
  TORCH_CHECK(mix_w.numel() == S && mix_b.numel() == 1, "g_newt_grad: one output channel only: mixer weight ", mix_w.sizes(), " / bias ",
              mix_b.sizes(), " for ", S, " shapers");
  const size_t nbytes = B < (1 << 30) && T < (1 << 30) ? nws_g_newt_grad_workspace_bytes(d, (int)B, (int)T, want_params ? 1 : 0) : 0;
  TORCH_CHECK(nbytes > 0, "g_newt_grad: unsupported size (", S, " shapers of width ", W, " and depth ", D, ", B ", B, ", T ", T,
              "): at most 64 shapers of width 16 and depth 4, T <= 65535, B T <= 2^28");
  Launch L(exciter);
  auto opt = exciter.options();
  std::vector<Tensor> out{at::empty({B, 4 * S, T}, opt)};
  float* ge = nullptr;
  if (want_exciter) {
    out.push_back(at::empty_like(exciter));
    ge = out.back().data_ptr<float>();
  }
  std::vector<float*> gp;
  if (want_params) {
    auto add = [&](std::vector<int64_t> shape) {
      out.push_back(at::empty(shape, opt));
      gp.push_back(out.back().data_ptr<float>());
    };
    add({1, S, 1});
    for (int64_t l = 0; l < D; ++l) {
      const int64_t cin = l == 0 ? 1 : W, cout = l == D - 1 ? 1 : W;
      add({S * cout, cin, 1});
      add({S * cout});
    }
    add({1, S, 1});
    add({1});
  }
  Tensor ws = at::empty({(int64_t)nbytes}, opt.dtype(at::kByte));
  nws_check(nws_g_newt_grad(d, mix_w.data_ptr<float>(), mix_b.data_ptr<float>(), exciter.data_ptr<float>(), film.data_ptr<float>(),
                            grad_out.data_ptr<float>(), (int)B, (int)T, NWS_HOP, ge, out[0].data_ptr<float>(),
                            want_params ? gp.data() : nullptr, ws.data_ptr(), nbytes, L.stream), "nws_g_newt_grad");
  return out;
}

// FIRNoiseSynth.forward for any even ir_length >= hop: H (B, L/2+1, T) -> (B, hop * T)
Tensor g_fir_noise(const Tensor& H, const Tensor& window, const Tensor& noise, int64_t hop) {
  check_dev(H, "H");
  check_dev(window, "window");
  check_dev(noise, "noise");
  check_same_device(H, "H", window, "noise_synth.window");
  check_same_device(H, "H", noise, "noise");
  const int64_t Lf = window.numel();
  TORCH_CHECK(H.dim() == 3 && H.size(1) == Lf / 2 + 1, "FIRNoiseSynth: expected H of shape (B, ", Lf / 2 + 1, ", T), got ", H.sizes());
  const int64_t B = H.size(0), T = H.size(2);
  TORCH_CHECK(noise.numel() == hop * T - 1, "noise: expected ", hop * T - 1, " samples, got ", noise.sizes());
  Launch L(H);
  Tensor fir = at::empty({B, T, Lf}, H.options());
  nws_check(nws_g_fir_design(H.data_ptr<float>(), window.data_ptr<float>(), (int)Lf, (int)B, (int)T, fir.data_ptr<float>(), L.stream),
            "nws_g_fir_design");
  Tensor out = at::empty({B, hop * T}, H.options());
  nws_check(nws_g_fir_noise(fir.data_ptr<float>(), noise.data_ptr<float>(), (int)Lf, (int)hop, (int)B, (int)T, nullptr, 0,
                            out.data_ptr<float>(), L.stream), "nws_g_fir_noise");
  return out;
}

Tensor g_reverb_direct(const Tensor& x, const Tensor& ir) {
  check_dev(x, "x");
  check_dev(ir, "reverb.ir");
  check_same_device(x, "x", ir, "reverb.ir");
  TORCH_CHECK(x.dim() == 2, "Reverb: expected (B, N), got ", x.sizes());
  Launch L(x);
  Tensor y = at::empty_like(x);
  nws_check(nws_g_reverb_direct(x.data_ptr<float>(), ir.data_ptr<float>(), (int)ir.numel(), (int)x.size(0), (int)x.size(1),
                                y.data_ptr<float>(), L.stream), "nws_g_reverb_direct");
  return y;
}

// ---- what stream_step and stream_step_slots check alike; `op` is the name their messages carry -----------------------------
struct StepDims {
  int64_t B, K, C;
};

// (fir_design / ir: NULL for g_stream_step, whose descriptor carries both)
StepDims check_step_tensors(const char* op, const Tensor& f0, const Tensor& control, const Tensor* fir_design, const Tensor& state,
                            const Tensor& phase_u, const Tensor& rand_phase, const Tensor* ir, const Tensor& out) {
  check_dev(f0, "f0");
  check_dev(control, "control");
  if (fir_design) check_dev(*fir_design, "fir_design");
  check_dev(state, "state", at::kByte);
  check_dev(phase_u, "phase_u");
  check_dev(rand_phase, "rand_phase");
  if (ir) check_dev(*ir, "reverb.ir");
  check_dev(out, "out");
  check_same_device(f0, "f0", control, "control");
  check_same_device(f0, "f0", state, "state");
  check_same_device(f0, "f0", out, "out");
  if (ir) check_same_device(f0, "f0", *ir, "reverb.ir");
  TORCH_CHECK(f0.dim() == 2 && control.dim() == 3 && control.size(0) == f0.size(0) && control.size(2) == f0.size(1) && control.size(1) >= 2,
              op, ": f0 (B, K), control (B, C>=2, K); got ", f0.sizes(), " / ", control.sizes());
  return {f0.size(0), f0.size(1), control.size(1)};
}

void check_step_io(const char* op, const StepDims& d, bool first, bool final, int64_t frames_seen, const Tensor& phase_u,
                   const Tensor& rand_phase, const OptTensor& noise_new, const OptTensor& noise_all, const Tensor& out,
                   const OptTensor& pre_out, int64_t n_harmonics = NWS_N_HARMONICS) {
  TORCH_CHECK(phase_u.numel() == n_harmonics && rand_phase.numel() == n_harmonics, "phase_u / rand_phase: ", n_harmonics,
              " elements each");
  TORCH_CHECK(noise_new.has_value() != noise_all.has_value(), op, ": give exactly one of noise_new and noise_all");
  const int M = nws_stream_out_samples((int)d.K, first, final);
  TORCH_CHECK(out.numel() == d.B * M, "out: expected (", d.B, ", ", M, "), got ", out.sizes());
  if (pre_out.has_value()) {
    check_dev(*pre_out, "pre_out");
    TORCH_CHECK(pre_out->numel() == d.B * M, "pre_out: expected (", d.B, ", ", M, ")");
  }
  if (noise_new.has_value()) {
    check_dev(*noise_new, "noise_new");
    TORCH_CHECK(noise_new->numel() >= nws_stream_noise_draws((int)d.K, first, frames_seen), "noise_new: expected ",
                nws_stream_noise_draws((int)d.K, first, frames_seen), " fresh samples");
  } else {
    check_dev(*noise_all, "noise_all");
  }
}

// ---- stateful streaming step (csrc/stream.hip): K new frames of B streams -> out (B, M); all state in `state` ----------
void stream_step(const Tensor& wdesc, const Tensor& fir_design, const OptTensor& plan_t, const OptTensor& tables,
                 const OptTensor& spectrum, Tensor& state, int64_t max_frames, const Tensor& f0, const Tensor& control, bool first,
                 bool final, int64_t frames_seen, int64_t nz_prev_start, double sample_rate, const Tensor& phase_u,
                 const Tensor& rand_phase, const OptTensor& noise_new, const OptTensor& noise_all, const Tensor& ir, Tensor& out,
                 const OptTensor& pre_out) {
  const NwsWeights* w = weights_of(wdesc);
  const StepDims d = check_step_tensors("stream_step", f0, control, &fir_design, state, phase_u, rand_phase, &ir, out);
  const int64_t B = d.B, K = d.K, C = d.C;
  TORCH_CHECK(K >= 1 && K <= max_frames, "stream_step: chunk of ", K, " frames, the stream was sized for ", max_frames);
  check_step_io("stream_step", d, first, final, frames_seen, phase_u, rand_phase, noise_new, noise_all, out, pre_out);
  NwsReverbPlan plan{};
  const bool fft = plan_t.has_value();
  if (fft) {
    TORCH_CHECK(tables.has_value() && spectrum.has_value(), "stream_step: plan without tables / spectrum");
    plan = plan_of(*plan_t);
    check_dev(*tables, "reverb_tables");
    check_dev(*spectrum, "reverb_spectrum");
    check_reverb_buffers(plan, *tables, *spectrum);
  }
  TORCH_CHECK((size_t)state.numel() >= nws_stream_state_bytes((int)B, (int)max_frames, (int)ir.numel(), fft ? &plan : nullptr),
              "stream_step: state blob too small");
  Launch L(f0);
  nws_check(nws_stream_step(w, fir_design.data_ptr<float>(), fft ? &plan : nullptr, fft ? tables->data_ptr() : nullptr,
                            fft ? spectrum->data_ptr() : nullptr, state.data_ptr(), (size_t)state.numel(), (int)B, (int)max_frames,
                            f0.data_ptr<float>(), control.data_ptr<float>(), (int)C, (int)K, first ? 1 : 0, final ? 1 : 0,
                            (long long)frames_seen, (long long)nz_prev_start, (float)sample_rate, phase_u.data_ptr<float>(),
                            rand_phase.data_ptr<float>(), fptr(noise_new), fptr(noise_all),
                            noise_all.has_value() ? (int)noise_all->numel() : 0, ir.data_ptr<float>(), (int)ir.numel(),
                            out.data_ptr<float>(), pre_out.has_value() ? pre_out->data_ptr<float>() : nullptr, L.stream),
            "nws_stream_step");
}

// ---- slot mode of the stateful stream (csrc/stream.hip nws_stream_step_slots): per-slot events in a device int32 (B) buffer ----
void stream_step_slots(const Tensor& wdesc, const Tensor& fir_design, Tensor& state, int64_t max_frames, const Tensor& f0,
                       const Tensor& control, int64_t frames_seen, int64_t nz_prev_start, double sample_rate, const Tensor& phase_u,
                       const Tensor& rand_phase, const OptTensor& noise_new, const OptTensor& noise_all, const Tensor& ir,
                       const Tensor& events, Tensor& out, const OptTensor& pre_out) {
  const NwsWeights* w = weights_of(wdesc);
  const StepDims d = check_step_tensors("stream_step_slots", f0, control, &fir_design, state, phase_u, rand_phase, &ir, out);
  const int64_t B = d.B, K = d.K, C = d.C;
  check_dev(events, "events", at::kInt);
  check_same_device(f0, "f0", events, "events");
  TORCH_CHECK(K >= 1 && K <= 16 && K <= max_frames, "stream_step_slots: hops of 1 .. 16 frames (sized for ", max_frames, "), got ", K);
  TORCH_CHECK(events.numel() == B, "stream_step_slots: events: one int32 word per slot, expected ", B, ", got ", events.numel());
  check_step_io("stream_step_slots", d, frames_seen == 0, false, frames_seen, phase_u, rand_phase, noise_new, noise_all, out, pre_out);
  TORCH_CHECK((size_t)state.numel() >= nws_stream_slot_state_bytes((int)B, (int)max_frames, (int)ir.numel()),
              "stream_step_slots: state blob too small");
  Launch L(f0);
  nws_check(nws_stream_step_slots(w, fir_design.data_ptr<float>(), state.data_ptr(), (size_t)state.numel(), (int)B, (int)max_frames,
                                  f0.data_ptr<float>(), control.data_ptr<float>(), (int)C, (int)K, (long long)frames_seen,
                                  (long long)nz_prev_start, (float)sample_rate, phase_u.data_ptr<float>(), rand_phase.data_ptr<float>(),
                                  fptr(noise_new), fptr(noise_all), noise_all.has_value() ? (int)noise_all->numel() : 0,
                                  ir.data_ptr<float>(), (int)ir.numel(), events.data_ptr<int>(), out.data_ptr<float>(),
                                  pre_out.has_value() ? pre_out->data_ptr<float>() : nullptr, L.stream),
            "nws_stream_step_slots");
}

// ---- the same step on the runtime-size path (csrc/generic.hip nws_g_stream_step): the model descriptor in place of the weights ----
void g_stream_step(const Tensor& gdesc, const OptTensor& plan_t, const OptTensor& tables, const OptTensor& spectrum, Tensor& state,
                   int64_t max_frames, const Tensor& f0, const Tensor& control, bool first, bool final, int64_t frames_seen,
                   int64_t nz_prev_start, double sample_rate, const Tensor& phase_u, const Tensor& rand_phase,
                   const OptTensor& noise_new, const OptTensor& noise_all, Tensor& out, const OptTensor& pre_out) {
  const NwsGenericModel* m = struct_of<NwsGenericModel>(gdesc, "gdesc");
  TORCH_CHECK(m->hop > 0 && m->n_harmonics > 0, "gdesc: not a NwsGenericModel");
  const StepDims d = check_step_tensors("g_stream_step", f0, control, nullptr, state, phase_u, rand_phase, nullptr, out);
  const int64_t B = d.B, K = d.K, C = d.C;
  TORCH_CHECK(K >= 1 && K <= max_frames, "g_stream_step: chunk of ", K, " frames, the stream was sized for ", max_frames);
  check_step_io("g_stream_step", d, first, final, frames_seen, phase_u, rand_phase, noise_new, noise_all, out, pre_out, m->n_harmonics);
  NwsReverbPlan plan{};
  const bool fft = plan_t.has_value();
  if (fft) {
    TORCH_CHECK(tables.has_value() && spectrum.has_value(), "g_stream_step: plan without tables / spectrum");
    plan = plan_of(*plan_t);
    check_dev(*tables, "reverb_tables");
    check_dev(*spectrum, "reverb_spectrum");
    check_reverb_buffers(plan, *tables, *spectrum);
  }
  const size_t need = nws_g_stream_state_bytes(m, (int)B, (int)max_frames, m->ir_len, fft ? &plan : nullptr);
  TORCH_CHECK(need != 0, "g_stream_step: the runtime-size stream does not serve this model (control hop 128, 256 noise taps, an "
              "impulse response below 32768 taps)");
  TORCH_CHECK((size_t)state.numel() >= need, "g_stream_step: state blob too small");
  Launch L(f0);
  nws_check(nws_g_stream_step(m, fft ? &plan : nullptr, fft ? tables->data_ptr() : nullptr, fft ? spectrum->data_ptr() : nullptr,
                              state.data_ptr(), (size_t)state.numel(), (int)B, (int)max_frames, f0.data_ptr<float>(),
                              control.data_ptr<float>(), (int)C, (int)K, first ? 1 : 0, final ? 1 : 0, (long long)frames_seen,
                              (long long)nz_prev_start, (float)sample_rate, phase_u.data_ptr<float>(), rand_phase.data_ptr<float>(),
                              fptr(noise_new), fptr(noise_all), noise_all.has_value() ? (int)noise_all->numel() : 0,
                              out.data_ptr<float>(), pre_out.has_value() ? pre_out->data_ptr<float>() : nullptr, L.stream),
            "nws_g_stream_step");
}

// ---- slot mode on the runtime-size path (csrc/generic.hip nws_g_stream_step_slots) ---------------------------------
void g_stream_step_slots(const Tensor& gdesc, Tensor& state, int64_t max_frames, const Tensor& f0, const Tensor& control,
                         int64_t frames_seen, int64_t nz_prev_start, double sample_rate, const Tensor& phase_u, const Tensor& rand_phase,
                         const OptTensor& noise_new, const OptTensor& noise_all, const Tensor& events, Tensor& out,
                         const OptTensor& pre_out) {
  const NwsGenericModel* m = struct_of<NwsGenericModel>(gdesc, "gdesc");
  TORCH_CHECK(m->hop > 0 && m->n_harmonics > 0, "gdesc: not a NwsGenericModel");
  const StepDims d = check_step_tensors("g_stream_step_slots", f0, control, nullptr, state, phase_u, rand_phase, nullptr, out);
  const int64_t B = d.B, K = d.K, C = d.C;
  check_dev(events, "events", at::kInt);
  check_same_device(f0, "f0", events, "events");
  TORCH_CHECK(K >= 1 && K <= 16 && K <= max_frames, "g_stream_step_slots: hops of 1 .. 16 frames (sized for ", max_frames, "), got ", K);
  TORCH_CHECK(events.numel() == B, "g_stream_step_slots: events: one int32 word per slot, expected ", B, ", got ", events.numel());
  check_step_io("g_stream_step_slots", d, frames_seen == 0, false, frames_seen, phase_u, rand_phase, noise_new, noise_all, out, pre_out,
                m->n_harmonics);
  const size_t need = nws_g_stream_slot_state_bytes(m, (int)B, (int)max_frames, m->ir_len);
  TORCH_CHECK(need != 0, "g_stream_step_slots: the runtime-size slot stream does not serve this model or size (control hop 128, 256 "
              "noise taps, an impulse response below 32768 taps, at most 16 frames per hop)");
  TORCH_CHECK((size_t)state.numel() >= need, "g_stream_step_slots: state blob too small");
  Launch L(f0);
  nws_check(nws_g_stream_step_slots(m, state.data_ptr(), (size_t)state.numel(), (int)B, (int)max_frames, f0.data_ptr<float>(),
                                    control.data_ptr<float>(), (int)C, (int)K, (long long)frames_seen, (long long)nz_prev_start,
                                    (float)sample_rate, phase_u.data_ptr<float>(), rand_phase.data_ptr<float>(), fptr(noise_new),
                                    fptr(noise_all), noise_all.has_value() ? (int)noise_all->numel() : 0, events.data_ptr<int>(),
                                    out.data_ptr<float>(), pre_out.has_value() ? pre_out->data_ptr<float>() : nullptr, L.stream),
            "nws_g_stream_step_slots");
}

// ---- note player (csrc/note_control.hip): the launches in front of and behind a slot stream's hop --------------
// `params`: 16 float64 values on the CPU in the order of _lib.NOTE_PARAMS
NwsNotePlayer note_player_of(const Tensor& params) {
  TORCH_CHECK(params.device().is_cpu() && params.scalar_type() == at::kDouble && params.is_contiguous() && params.numel() == 16,
              "params: expected a CPU float64 tensor of 16 values [attack, decay, release, vib_delay, vib_ramp, drop, silence, "
              "peak_lo, peak_hi, vib_rate, vib_depth, sample_rate, mean0, std0, mean1, std1]");
  const double* p = params.data_ptr<double>();
  for (int i = 0; i < 5; ++i)
    TORCH_CHECK(p[i] >= -1e9 && p[i] <= 1e9 && p[i] == (double)(int)p[i], "params: attack, decay, release, vib_delay and vib_ramp are whole frames, got ", p[i]);
  NwsNotePlayer P{};
  P.attack = (int)p[0], P.decay = (int)p[1], P.release = (int)p[2], P.vib_delay = (int)p[3], P.vib_ramp = (int)p[4];
  P.drop = (float)p[5], P.silence = (float)p[6], P.peak_lo = (float)p[7], P.peak_hi = (float)p[8];
  P.vib_rate = p[9], P.vib_depth = (float)p[10], P.sample_rate = p[11];
  P.mean[0] = (float)p[12], P.std[0] = (float)p[13], P.mean[1] = (float)p[14], P.std[1] = (float)p[15];
  return P;
}

size_t note_state_bytes(const char* op, int64_t B) {
  const size_t nbytes = B >= 1 && B <= 65535 ? nws_note_control_state_bytes((int)B) : 0;
  TORCH_CHECK(nbytes > 0, op, ": unsupported slot count ", B, ": 1 <= B <= 65535");
  return nbytes;
}

void note_control_reset(Tensor& state, int64_t B) {
  check_dev(state, "state", at::kByte);
  const size_t nbytes = note_state_bytes("note_control_reset", B);
  TORCH_CHECK((size_t)state.numel() >= nbytes, "note_control_reset: state blob too small (expected ", nbytes, " bytes for B = ", B,
              ", got ", state.numel(), ")");
  Launch L(state);
  nws_check(nws_note_control_reset(state.data_ptr(), (size_t)state.numel(), (int)B, L.stream), "nws_note_control_reset");
}

void note_control(const Tensor& params, const Tensor& events, const Tensor& notes, Tensor& state, Tensor& f0, Tensor& control) {
  const NwsNotePlayer P = note_player_of(params);
  check_dev(events, "events", at::kInt);
  check_dev(notes, "notes", at::kInt);
  check_dev(state, "state", at::kByte);
  check_dev(f0, "f0");
  check_dev(control, "control");
  check_same_device(f0, "f0", events, "events");
  check_same_device(f0, "f0", notes, "notes");
  check_same_device(f0, "f0", state, "state");
  check_same_device(f0, "f0", control, "control");
  TORCH_CHECK(f0.dim() == 2 && f0.size(0) >= 1, "note_control: expected f0 (B, K), got ", f0.sizes());
  const int64_t B = f0.size(0), K = f0.size(1);
  TORCH_CHECK(K >= 1 && K <= 16, "note_control: a hop has 1 .. 16 frames, got ", K);
  TORCH_CHECK(control.dim() == 3 && control.size(0) == B && control.size(1) == 2 && control.size(2) == K,
              "note_control: expected control (", B, ", 2, ", K, "), got ", control.sizes());
  TORCH_CHECK(events.numel() == B, "note_control: expected ", B, " event words, got ", events.numel());
  TORCH_CHECK(notes.dim() == 2 && notes.size(0) == B && notes.size(1) == 4,
              "note_control: expected the note table as int32 (", B, ", 4) [pitch bits, velocity bits, j_off, 0], got ", notes.sizes());
  TORCH_CHECK(P.release >= 1 && P.vib_ramp >= 1, "note_control: release and vib_ramp are at least one frame");
  const size_t nbytes = note_state_bytes("note_control", B);
  TORCH_CHECK((size_t)state.numel() >= nbytes, "note_control: state blob too small (expected ", nbytes, " bytes for B = ", B, ", got ",
              state.numel(), ")");
  Launch L(f0);
  nws_check(nws_note_control(&P, events.data_ptr<int32_t>(), reinterpret_cast<const NwsNote*>(notes.data_ptr<int32_t>()),
                             state.data_ptr(), (size_t)state.numel(), (int)B, (int)K, f0.data_ptr<float>(),
                             control.data_ptr<float>(), L.stream), "nws_note_control");
}

void voice_mix(const Tensor& o, const Tensor& gain, Tensor& out) {
  check_dev(o, "o");
  check_dev(gain, "gain");
  check_dev(out, "out");
  check_same_device(o, "o", gain, "gain");
  check_same_device(o, "o", out, "out");
  TORCH_CHECK(o.dim() == 2 && o.size(0) >= 1 && o.size(1) >= 1 && o.size(1) <= INT32_MAX, "voice_mix: expected o (B, N), got ", o.sizes());
  const int64_t B = o.size(0), N = o.size(1);
  TORCH_CHECK(B <= 65535, "voice_mix: unsupported slot count ", B, ": 1 <= B <= 65535");
  TORCH_CHECK(gain.dim() == 2 && gain.size(0) == B && (gain.size(1) == 1 || gain.size(1) == 2),
              "voice_mix: expected gain (", B, ", 1 or 2), got ", gain.sizes());
  const int64_t C = gain.size(1);
  TORCH_CHECK(out.dim() == 2 && out.size(0) == C && out.size(1) == N, "voice_mix: expected out (", C, ", ", N, "), got ", out.sizes());
  Launch L(o);
  nws_check(nws_voice_mix(o.data_ptr<float>(), gain.data_ptr<float>(), (int)B, (int)N, (int)C, out.data_ptr<float>(), L.stream),
            "nws_voice_mix");
}

int64_t abi_version() { return nws_abi_version(); }

}  // namespace

TORCH_LIBRARY(newt_hip, m) {
  m.def("abi_version() -> int", &abi_version);
  m.def("forward(Tensor wdesc, Tensor f0, Tensor control, Tensor phase_u, Tensor rand_phase, Tensor noise, Tensor fir_design, "
        "Tensor plan, Tensor reverb_tables, Tensor reverb_spectrum, Tensor(a!) workspace, float sample_rate) -> Tensor", &forward);
  m.def("forward_control(Tensor wdesc, Tensor f0, Tensor control, Tensor(a!) workspace, bool batched_gru) -> ()", &forward_control);
  m.def("forward_audio(Tensor wdesc, Tensor f0, Tensor phase_u, Tensor rand_phase, Tensor noise, Tensor fir_design, Tensor plan, "
        "Tensor reverb_tables, Tensor reverb_spectrum, Tensor(a!) workspace, float sample_rate, Tensor? out, int wait_event, "
        "int record_event) -> Tensor", &forward_audio);
  m.def("forward_audio_pre(Tensor wdesc, Tensor f0, Tensor phase_u, Tensor rand_phase, Tensor noise, Tensor fir_design, Tensor plan, "
        "Tensor reverb_tables, Tensor reverb_spectrum, Tensor(a!) workspace, float sample_rate) -> ()", &forward_audio_pre);
  m.def("forward_audio_blocks(Tensor wdesc, Tensor f0, Tensor phase_u, Tensor rand_phase, Tensor noise, Tensor fir_design, Tensor plan, "
        "Tensor reverb_tables, Tensor reverb_spectrum, Tensor(a!) workspace, float sample_rate, Tensor(b!) out, int[] row0, int[] nrows, "
        "int[] events) -> ()", &forward_audio_blocks);
  m.def("forward_reverb_rows(Tensor fir_design, Tensor plan, Tensor reverb_tables, Tensor reverb_spectrum, Tensor(a!) workspace, int T, "
        "int row0, int nrows, Tensor(b!) out) -> ()", &forward_reverb_rows);
  m.def("phase_carry(Tensor? f0, Tensor? f0_up) -> Tensor", &phase_carry);
  m.def("exciter_newt(Tensor wdesc, Tensor? f0, Tensor? f0_up, Tensor carry, Tensor phase_u, Tensor rand_phase, Tensor? film, "
        "float sample_rate, bool want_exciter, bool want_newt) -> (Tensor, Tensor)", &exciter_newt);
  m.def("oscillator(Tensor f0_up, Tensor phase_u, Tensor rand_phase, float sample_rate) -> Tensor", &oscillator);
  m.def("control_gru(Tensor wdesc, Tensor control, Tensor? h0, bool batched) -> (Tensor, Tensor)", &control_gru);
  m.def("control_gru_grad(Tensor wdesc, Tensor control, Tensor? h0, Tensor gru_out, Tensor grad_out, Tensor? grad_hT, "
        "bool want_params) -> Tensor[]", &control_gru_grad);
  m.def("frame_mlps(Tensor wdesc, Tensor gru_out, Tensor fir_design, bool want_emb, bool want_H) -> (Tensor, Tensor, Tensor, Tensor)",
        &frame_mlps);
  m.def("fir_noise(Tensor fir, Tensor noise, Tensor? add_in, int origin) -> Tensor", &fir_noise);
  m.def("frame_mlps_spec(Tensor wdesc, Tensor gru_out) -> (Tensor, Tensor)", &frame_mlps_spec);
  m.def("fir_noise_spec(Tensor spec, Tensor noise, Tensor? add_in) -> Tensor", &fir_noise_spec);
  m.def("fir_from_h(Tensor H, Tensor fir_design) -> Tensor", &fir_from_h);
  m.def("fir_noise_grad(Tensor noise, Tensor grad_out) -> Tensor", &fir_noise_grad);
  m.def("fir_from_h_grad(Tensor grad_fir, Tensor fir_design) -> Tensor", &fir_from_h_grad);
  m.def("sum_batch_time(Tensor x) -> Tensor", &sum_batch_time);
  m.def("reverb(Tensor plan, Tensor tables, Tensor spectrum, Tensor x) -> Tensor", &reverb);
  m.def("reverb_grad_x(Tensor plan, Tensor tables, Tensor spectrum, Tensor grad_out) -> Tensor", &reverb_grad_x);
  m.def("reverb_grad_ir(Tensor plan, Tensor tables, Tensor x, Tensor grad_out, int ir_len) -> Tensor", &reverb_grad_ir);
  m.def("reverb_linear_chunk(Tensor plan, Tensor tables, Tensor spectrum, Tensor x, Tensor tail_in) -> (Tensor, Tensor)",
        &reverb_linear_chunk);
  m.def("shaper_apply(Tensor wdesc, Tensor x) -> Tensor", &shaper_apply);
  m.def("shaper_table(Tensor wdesc, Tensor like, int size, float tmin, float tmax) -> Tensor", &shaper_table);
  m.def("newt_apply(Tensor wdesc, Tensor exciter, Tensor film) -> Tensor", &newt_apply);
  m.def("newt_grad(Tensor wdesc, Tensor exciter, Tensor film, Tensor grad_out, bool want_exciter, bool want_params) -> Tensor[]",
        &newt_grad);
  m.def("adam_step(Tensor(a!)[] params, Tensor[] grads, Tensor(b!)[] exp_avgs, Tensor(c!)[] exp_avg_sqs, int step, float lr, "
        "float beta1, float beta2, float eps, float max_norm) -> Tensor", &adam_step);
  m.def("grad_pack(Tensor[] tensors, Tensor(a!) out) -> ()", &grad_pack);
  m.def("grad_reduce(Tensor rows, Tensor(a!) out) -> ()", &grad_reduce);
  m.def("td_mlp(Tensor x, Tensor[] weights, Tensor[] biases, Tensor[] ln_w, Tensor[] ln_b, float eps, float slope) -> Tensor", &td_mlp);
  m.def("td_mlp_grad(Tensor x, Tensor grad_y, Tensor[] weights, Tensor[] biases, Tensor[] ln_w, Tensor[] ln_b, float eps, float slope, "
        "bool want_params) -> Tensor[]", &td_mlp_grad);
  m.def("td_layer_norm(Tensor x, Tensor weight, Tensor bias, float eps) -> Tensor", &td_layer_norm);
  m.def("film(Tensor x, Tensor gamma, Tensor beta) -> Tensor", &film);
  m.def("sine(Tensor x) -> Tensor", &sine);
  m.def("forward_generic(Tensor gdesc, Tensor f0, Tensor control, Tensor phase_u, Tensor rand_phase, Tensor noise, Tensor? plan, "
        "Tensor? reverb_tables, Tensor? reverb_spectrum, Tensor(a!) reverb_workspace, Tensor(b!) workspace, float sample_rate) -> Tensor",
        &forward_generic);
  m.def("g_gru(Tensor w_ih, Tensor w_hh, Tensor b_ih, Tensor b_hh, Tensor control, Tensor? h0) -> (Tensor, Tensor)", &g_gru);
  m.def("g_oscillator(Tensor f0_up, Tensor phase_u, Tensor rand_phase, float sample_rate) -> Tensor", &g_oscillator);
  m.def("g_conv1x1(Tensor x, Tensor weight, Tensor? bias) -> Tensor", &g_conv1x1);
  m.def("g_upsample(Tensor x, int hop) -> Tensor", &g_upsample);
  m.def("g_shaper_apply(Tensor sdesc, Tensor x) -> Tensor", &g_shaper_apply);
  m.def("g_shaper_table(Tensor sdesc, Tensor like, int size, float tmin, float tmax) -> Tensor", &g_shaper_table);
  m.def("g_newt_apply(Tensor sdesc, Tensor exciter, Tensor film, Tensor mix_w, Tensor mix_b) -> Tensor", &g_newt_apply);
  m.def("g_newt_grad(Tensor sdesc, Tensor exciter, Tensor film, Tensor grad_out, Tensor mix_w, Tensor mix_b, bool want_exciter, "
        "bool want_params) -> Tensor[]", &g_newt_grad);
  m.def("g_fir_noise(Tensor H, Tensor window, Tensor noise, int hop) -> Tensor", &g_fir_noise);
  m.def("g_reverb_direct(Tensor x, Tensor ir) -> Tensor", &g_reverb_direct);
  m.def("stream_step(Tensor wdesc, Tensor fir_design, Tensor? plan, Tensor? reverb_tables, Tensor? reverb_spectrum, Tensor(a!) state, "
        "int max_frames, Tensor f0, Tensor control, bool first, bool final, int frames_seen, int nz_prev_start, float sample_rate, "
        "Tensor phase_u, Tensor rand_phase, Tensor? noise_new, Tensor? noise_all, Tensor ir, Tensor(b!) out, Tensor(c!)? pre_out) -> ()",
        &stream_step);
  m.def("stream_step_slots(Tensor wdesc, Tensor fir_design, Tensor(a!) state, int max_frames, Tensor f0, Tensor control, int frames_seen, "
        "int nz_prev_start, float sample_rate, Tensor phase_u, Tensor rand_phase, Tensor? noise_new, Tensor? noise_all, Tensor ir, "
        "Tensor events, Tensor(b!) out, Tensor(c!)? pre_out) -> ()",
        &stream_step_slots);
  m.def("g_stream_step(Tensor gdesc, Tensor? plan, Tensor? reverb_tables, Tensor? reverb_spectrum, Tensor(a!) state, int max_frames, "
        "Tensor f0, Tensor control, bool first, bool final, int frames_seen, int nz_prev_start, float sample_rate, Tensor phase_u, "
        "Tensor rand_phase, Tensor? noise_new, Tensor? noise_all, Tensor(b!) out, Tensor(c!)? pre_out) -> ()",
        &g_stream_step);
  m.def("g_stream_step_slots(Tensor gdesc, Tensor(a!) state, int max_frames, Tensor f0, Tensor control, int frames_seen, "
        "int nz_prev_start, float sample_rate, Tensor phase_u, Tensor rand_phase, Tensor? noise_new, Tensor? noise_all, "
        "Tensor events, Tensor(b!) out, Tensor(c!)? pre_out) -> ()",
        &g_stream_step_slots);
  m.def("loudness(Tensor audio, Tensor dft, int n_fft, int hop, float amin, float top_db, bool normalise) -> Tensor", &loudness);
  m.def("loudness_peak_power(Tensor audio, Tensor dft, int n_fft, int hop) -> Tensor", &loudness_peak_power);
  m.def("loudness_stream_reset(Tensor(a!) state, int B, int n_fft, int hop, Tensor initial_power, bool track) -> ()",
        &loudness_stream_reset);
  m.def("loudness_stream_step(Tensor(a!) state, Tensor dft, int n_fft, int hop, int lag, Tensor chunk, int n_seen, bool final, "
        "float amin, float top_db, bool normalise, Tensor(b!) loudness, Tensor(c!) reference_power) -> ()", &loudness_stream_step);
  m.def("loudness_stream_reset_release(Tensor(a!) state, int B, int n_fft, int hop, Tensor floor_power) -> ()",
        &loudness_stream_reset_release);
  m.def("loudness_stream_step_release(Tensor(a!) state, Tensor dft, int n_fft, int hop, int lag, float release_factor, bool track, "
        "Tensor chunk, int n_seen, bool final, float amin, float top_db, bool normalise, Tensor(b!) loudness, "
        "Tensor(c!) reference_power) -> ()", &loudness_stream_step_release);
  m.def("loudness_causal(Tensor audio, Tensor dft, int n_fft, int hop, int lag, float release_factor, Tensor floor_power, bool track, "
        "float amin, float top_db, bool normalise) -> (Tensor, Tensor, Tensor)", &loudness_causal);
  m.def("pyin_table(float sample_rate, float fmin, float fmax, int frame_length, int hop) -> Tensor", &pyin_table);
  m.def("pyin_cmnd(Tensor audio, float sample_rate, float fmin, float fmax, int frame_length, int hop) -> Tensor", &pyin_cmnd);
  m.def("pyin_observe(Tensor yin, Tensor table, float sample_rate, float fmin, float fmax, int frame_length, int hop) -> "
        "(Tensor, Tensor, Tensor, Tensor)", &pyin_observe);
  m.def("pyin_viterbi(Tensor cand_bin, Tensor cand_prob, Tensor count, Tensor voiced_prob, Tensor table, float sample_rate, "
        "float fmin, float fmax, int frame_length, int hop, bool fill_unvoiced, float fill_value) -> (Tensor, Tensor)", &pyin_viterbi);
  m.def("pyin(Tensor audio, Tensor table, float sample_rate, float fmin, float fmax, int frame_length, int hop, bool fill_unvoiced, "
        "float fill_value) -> (Tensor, Tensor, Tensor)", &pyin);
  m.def("pyin_stream_reset(Tensor(a!) state, int B, float sample_rate, float fmin, float fmax, int frame_length, int hop) -> ()",
        &pyin_stream_reset);
  m.def("pyin_stream_step(Tensor(a!) state, Tensor table, float sample_rate, float fmin, float fmax, int frame_length, int hop, "
        "int lag, Tensor chunk, int n_seen, bool final, bool fill_unvoiced, float fill_value, Tensor(b!) f0, "
        "Tensor(c!) voiced_prob, Tensor(d!) states) -> ()", &pyin_stream_step);
  m.def("resample_bank(int sr_in, int sr_out) -> Tensor", &resample_bank);
  m.def("resample(Tensor audio, Tensor bank, int sr_in, int sr_out) -> Tensor", &resample);
  m.def("resample_stream_reset(Tensor(a!) state, int B, int sr_in, int sr_out) -> ()", &resample_stream_reset);
  m.def("resample_stream_step(Tensor(a!) state, Tensor bank, int sr_in, int sr_out, Tensor chunk, bool final, Tensor(b!) out) -> ()",
        &resample_stream_step);
  m.def("note_control_reset(Tensor(a!) state, int B) -> ()", &note_control_reset);
  m.def("note_control(Tensor params, Tensor events, Tensor notes, Tensor(a!) state, Tensor(b!) f0, Tensor(c!) control) -> ()",
        &note_control);
  m.def("voice_mix(Tensor o, Tensor gain, Tensor(a!) out) -> ()", &voice_mix);
  m.def("mfcc_table(float sample_rate, int n_fft, int n_mfcc, int n_mels) -> Tensor", &mfcc_table);
  m.def("stft_loss_dft(int n_fft, int win_length) -> Tensor", &stft_loss_dft);
  m.def("stft_loss(Tensor x, Tensor y, Tensor[] dfts, int[] n_ffts, int[] hops, int[] win_lengths, float w_sc, float w_log_mag, "
        "float w_lin_mag, float eps) -> Tensor[]", &stft_loss);
  m.def("stft_loss_grad(Tensor x, Tensor y, Tensor[] dfts, int[] n_ffts, int[] hops, int[] win_lengths, float w_sc, float w_log_mag, "
        "float w_lin_mag, float eps) -> Tensor", &stft_loss_grad);
  m.def("mfcc(Tensor audio, Tensor dft, Tensor table, float sample_rate, int n_fft, int hop, int n_mfcc, int n_mels) -> Tensor", &mfcc);
}
