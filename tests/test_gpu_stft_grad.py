"""-m gpu: dL/dx of the multi-resolution STFT loss (csrc/stft_grad.hip through losses.py) against the float64 restatement of
the definition (tests/stft_grad_restatement.py).  The distance is the largest per-row ||g - g64||_2 / ||g64||_2.

Two bars.  The spectral-convergence and linear-magnitude terms are well conditioned: the project's parity bar, 1e-4.  The
log-magnitude term weighs every bin by 1 / x_mag, which turns the absolute rounding of a weak bin next to a strong partial into
phase error; torch's own float32 autograd through torch.stft is already 4.7e-5 ... 2.8e-4 / 1.7e-3 from float64 on `signals` at the
two shapes, so no fp32 transform meets 1e-4 there.  For w = (0, 1, 0) and the default (1, 1, 0) the yardstick is computed in the test - the distance of torch's
float32 CPU autograd from the same restatement on the same inputs - and the kernel may be at most 10 x that: it sums 600 - 1200
fp32 products per bin where an FFT has about 11 stages, and rounding grows roughly with the square root of that ratio (an
estimate, not a measurement).

Shapes (the smallest at which each path exists): (1, 1100) is just past the reflect limit of n_fft 2048 - 5, 10 and 23 frames,
both edges fold into the same few samples; (3, 4000) has 81 frames at hop 50 - three frame tiles, the last holding one frame -
and a length no hop divides.

Measured on the MI355X, (1, 1100) then (3, 4000).  Well-conditioned terms, kernel: w = (1, 0, 0) on signals 5.2e-7, 8.4e-7, on
noise_signals 6.9e-7, 5.4e-7; w = (0, 0, 1) on noise_signals 8.5e-7, 5.7e-7; STFTLoss(256, 64, 256, w_sc=1, w_log_mag=0) at (3, 4000) 1.0e-6.
Log-magnitude term and default loss, kernel | torch float32 CPU autograd | ratio:
    w = (0, 1, 0)  noise_signals   1.97e-4 | 1.23e-4 | 1.60     3.98e-4 | 4.03e-4 | 0.99
    w = (0, 1, 0)  signals         1.31e-4 | 4.70e-5 | 2.79     1.92e-4 | 1.62e-3 | 0.12
    w = (1, 1, 0)  noise_signals   1.93e-4 | 1.20e-4 | 1.60     3.92e-4 | 3.96e-4 | 0.99
    w = (1, 1, 0)  signals         1.30e-4 | 4.66e-5 | 2.79     1.90e-4 | 1.60e-3 | 0.12
    w = (1, 1, 0)  all-zero target, signals x                   4.21e-7 | 1.22e-5 | 0.03
The yardstick depends on the host's FFT too (signals at (1, 1100): 4.7e-5 on that machine's CPU, 2.8e-4 on another); the kernel's
figures do not.  Adam, 30 steps at lr 1e-3 on signals(1, 1100): loss 1.1511 -> 0.7371.
The same file passes with NWS_BACKEND=ctypes (the ctypes binding instead of torch.ops)."""
import functools

import numpy as np
import pytest
import torch

import stft_grad_restatement as gr
from gpu_util import dev, record

pytestmark = pytest.mark.gpu

TOL = 1e-4
FACTOR = 10.0
SHAPES = ((1, 1100), (3, 4000))
SIGNALS = {"signals": gr.signals, "noise": gr.noise_signals}


def _nws():
    import nws_amd as nws

    return nws


@functools.lru_cache(maxsize=None)
def _pair(kind, B, N):
    """the inputs of a case, read-only; zero_x / zero_y replace one side of `signals` by zeros"""
    if kind in SIGNALS:
        return SIGNALS[kind](B, N)
    x, y = gr.signals(B, N)
    z = np.zeros_like(x)
    z.setflags(write=False)
    return (z, y) if kind == "zero_x" else (x, z)


@functools.lru_cache(maxsize=None)
def _reference(kind, B, N, w):
    g = gr.grad(*_pair(kind, B, N), w_sc=w[0], w_log_mag=w[1], w_lin_mag=w[2])
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def _yardstick(kind, B, N, w):
    """distance of torch's float32 CPU autograd from the float64 restatement on the same inputs"""
    _, g32 = gr.torch_autograd_grad(*_pair(kind, B, N), torch.float32, w_sc=w[0], w_log_mag=w[1], w_lin_mag=w[2])
    return gr.row_distance(g32, _reference(kind, B, N, w))


def _kernel_grad(kind, B, N, w):
    x, y = _pair(kind, B, N)
    m = _nws().MultiResolutionSTFTLoss(w_sc=w[0], w_log_mag=w[1], w_lin_mag=w[2])
    loss, g = m.loss_and_grad(dev(x), dev(y))
    assert g.shape == (B, N) and g.dtype == torch.float32 and g.is_cuda and loss.dim() == 0
    return g.cpu().numpy()


@pytest.mark.parametrize("B,N", SHAPES)
@pytest.mark.parametrize("kind,w", (("signals", (1.0, 0.0, 0.0)), ("noise", (1.0, 0.0, 0.0)), ("noise", (0.0, 0.0, 1.0))))
def test_well_conditioned_terms_meet_the_parity_bar(kind, w, B, N):
    dist = gr.row_distance(_kernel_grad(kind, B, N, w), _reference(kind, B, N, w))
    print(f"{kind} w {w} ({B}, {N}): kernel {dist:.2e}")
    record(f"stft_grad/{kind}_w{''.join(str(int(v)) for v in w)}_{B}x{N}", row_rel_l2=dist)
    assert dist <= TOL


def test_single_resolution_full_width_window_meets_the_parity_bar():
    x, y = gr.signals(3, 4000)
    _, g = _nws().STFTLoss(256, 64, 256, w_sc=1.0, w_log_mag=0.0).loss_and_grad(dev(x), dev(y))
    dist = gr.row_distance(g.cpu().numpy(), gr.grad(x, y, ((256, 64, 256),), w_sc=1.0, w_log_mag=0.0))
    print(f"single (256, 64, 256) sc (3, 4000): kernel {dist:.2e}")
    record("stft_grad/single_256_sc_3x4000", row_rel_l2=dist)
    assert dist <= TOL


@pytest.mark.parametrize("B,N", SHAPES)
@pytest.mark.parametrize("kind", ("noise", "signals"))
@pytest.mark.parametrize("w", ((0.0, 1.0, 0.0), (1.0, 1.0, 0.0)), ids=("log", "default"))
def test_log_magnitude_term_within_ten_times_torch_float32(w, kind, B, N):
    dist = gr.row_distance(_kernel_grad(kind, B, N, w), _reference(kind, B, N, w))
    yard = _yardstick(kind, B, N, w)
    print(f"{kind} w {w} ({B}, {N}): kernel {dist:.2e}, torch float32 autograd {yard:.2e}, ratio {dist / yard:.2f}")
    record(f"stft_grad/{kind}_w{''.join(str(int(v)) for v in w)}_{B}x{N}", row_rel_l2=dist, torch_f32_row_rel_l2=yard)
    assert dist <= FACTOR * yard


def test_exact_zeros_and_the_all_zero_target():
    B, N, w = 3, 4000, (1.0, 1.0, 0.0)
    x, y = gr.signals(B, N)
    m = _nws().MultiResolutionSTFTLoss()
    zeros = torch.zeros(B, N, device="cuda")
    # every bin of an all-zero x is under the clamp: no gradient passes
    assert torch.equal(m.loss_and_grad(zeros, dev(y))[1], zeros)
    # x = y: sign(0) = 0 and the spectral-convergence term is 0 at a zero norm - no NaN from 0 / 0
    loss, g = m.loss_and_grad(dev(y), dev(y))
    assert float(loss) == 0.0 and torch.equal(g, zeros)
    dist = gr.row_distance(_kernel_grad("zero_y", B, N, w), _reference("zero_y", B, N, w))
    yard = _yardstick("zero_y", B, N, w)
    print(f"all-zero target ({B}, {N}): kernel {dist:.2e}, torch float32 autograd {yard:.2e}, ratio {dist / yard:.2f}")
    record(f"stft_grad/zero_target_{B}x{N}", row_rel_l2=dist, torch_f32_row_rel_l2=yard)
    assert dist <= FACTOR * yard


def test_autograd_carries_the_bits_of_loss_and_grad():
    nws = _nws()
    x, y = (dev(a) for a in gr.signals(3, 4000))
    plain, diff = nws.MultiResolutionSTFTLoss(), nws.MultiResolutionSTFTLoss(differentiable=True)
    want_loss, want = diff.loss_and_grad(x, y)
    assert not want.requires_grad and not want_loss.requires_grad and torch.equal(want_loss, plain(x, y))
    again = plain.loss_and_grad(x, y)                      # whatever the flag; equal bits for equal inputs
    assert torch.equal(again[0], want_loss) and torch.equal(again[1], want)

    leaf = x.clone().requires_grad_()
    loss = diff(leaf, y)
    assert loss.requires_grad and loss.dim() == 0 and torch.equal(loss.detach(), want_loss)
    loss.backward()
    assert torch.equal(leaf.grad, want)
    leaf.grad = None
    (2.0 * diff(leaf, y)).backward()
    assert torch.equal(leaf.grad, 2.0 * want)

    leaf3 = x.unsqueeze(1).clone().requires_grad_()       # (B, 1, N) in, (B, 1, N) out
    diff(leaf3, y.unsqueeze(1)).backward()
    assert leaf3.grad.shape == (3, 1, 4000) and torch.equal(leaf3.grad, want.unsqueeze(1))
    assert diff.loss_and_grad(x.unsqueeze(1), y.unsqueeze(1))[1].shape == (3, 1, 4000)
    with torch.no_grad():                                 # loss_and_grad does not look at the grad mode
        assert torch.equal(diff.loss_and_grad(leaf, y)[1], want)

    with pytest.raises(RuntimeError, match="no backward pass"):
        plain(leaf, y)
    with pytest.raises(RuntimeError, match="no backward pass"):
        diff.components(leaf, y)
    with pytest.raises(RuntimeError, match="the target gets no gradient"):
        diff(leaf, y.clone().requires_grad_())


def test_it_optimises():
    x, y = gr.signals(1, 1100)
    leaf, target = dev(x).requires_grad_(), dev(y)
    m = _nws().MultiResolutionSTFTLoss(differentiable=True)
    opt = torch.optim.Adam([leaf], lr=1e-3)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss = m(leaf, target)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    first, last = float(losses[0]), float(m(leaf.detach(), target))
    print(f"Adam, 30 steps at lr 1e-3 on signals(1, 1100): loss {first:.4f} -> {last:.4f}")
    record("stft_grad/adam_30_steps", first=first, last=last)
    assert last < first
