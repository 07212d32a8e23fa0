"""The float64 restatement of the noise branch's backward (tests/fir_noise_grad_restatement.py) against itself and
against torch's float64 autograd through the reference expression (models/modules/generators.py:21-35).  No GPU."""
import numpy as np
import pytest
import torch

import fir_noise_grad_restatement as nr

SHAPES = ((1, 2), (3, 5), (2, 9))


@pytest.mark.parametrize("B,T", SHAPES)
def test_the_two_forms_agree(B, T):
    H, u, g = nr.inputs(B, T)
    a, b = nr.grad_taps_explicit(u, g), nr.grad_taps_fft(u, g)
    assert a.shape == b.shape == (B, T, 256)
    assert nr.worst_row(b, a) <= 1e-12


@pytest.mark.parametrize("B,T", SHAPES)
def test_the_restatement_is_torchs_float64_gradient(B, T):
    H, u, g = nr.inputs(B, T)
    du64, dH64 = nr.torch_autograd_grads(H, u, g, torch.float64)
    du, dH = nr.grad_fir(u, g), nr.grad_H(u, g)
    assert du.shape == (B, T, 128) and dH.shape == (B, 129, T)
    assert nr.worst_row(du, du64) <= 1e-9 and nr.worst_row(dH, dH64) <= 1e-9
    # and the forward restatement is the reference's forward (the transpose identities of the GPU tests lean on it)
    out, _ = nr.torch_reference(torch.tensor(np.array(H), dtype=torch.float64), torch.tensor(np.array(u), dtype=torch.float64),
                                torch.hann_window(256, dtype=torch.float64))
    assert nr.worst_row(nr.forward(H, u), out.numpy()) <= 1e-12


def test_zero_gradient_in_zero_gradient_out():
    H, u, g = nr.inputs(3, 5)
    z = np.zeros_like(g)
    assert not nr.grad_taps_explicit(u, z).any() and not nr.grad_taps_fft(u, z).any() and not nr.grad_H(u, z).any()


def test_fold_is_the_gradient_of_the_stored_half_row():
    """<full_rows(v), dh> = <v, fold(dh)> for every half row v: fold is the transpose of the mirror that makes a full row"""
    rng = np.random.default_rng(5)
    dh, v = rng.standard_normal((2, 3, 256)), rng.standard_normal((2, 3, 128))
    assert abs(np.sum(nr.full_rows(v) * dh) - np.sum(v * nr.fold(dh))) <= 1e-12 * np.linalg.norm(v) * np.linalg.norm(dh)
    du = nr.fold(dh)
    assert np.array_equal(du[..., 0], dh[..., 128]) and np.array_equal(du[..., 5], dh[..., 133] + dh[..., 123])
    # the forward through the half rows of a symmetric window's taps is the forward through the full rows
    H, u, g = nr.inputs(2, 9)
    h = nr.taps(H)
    assert np.max(np.abs(nr.full_rows(h[..., 128:]) - h)) <= 1e-15
    # transpose identity of the restatement itself: <forward(h), g> = <h, dh>
    lhs, rhs = np.sum(nr.forward_from_taps(h, u) * g), np.sum(h * nr.grad_taps_fft(u, g))
    assert abs(lhs - rhs) <= 1e-12 * np.linalg.norm(h) * np.linalg.norm(g)


def test_half_row_contraction_is_the_full_one_for_the_periodic_hann():
    D = nr.design_matrix()
    sym = max(np.max(np.abs(D[128 - d] - D[128 + d])) for d in range(1, 128))
    assert sym <= 4e-18 and np.max(np.abs(D[0])) <= 4e-18
    H, u, g = nr.inputs(3, 5)
    dh = nr.grad_taps_fft(u, g)
    assert nr.worst_row(nr.grad_H_from_half(nr.fold(dh)), nr.grad_H_from_full(dh)) <= 1e-14
    # a window without the symmetry: the two differ, which is why the runtime-size path gets no gradient from these kernels
    w = nr.hann_periodic() * (1.0 + 0.3 * np.arange(256) / 256)
    assert nr.worst_row(nr.grad_H_from_half(nr.fold(dh), w), nr.grad_H_from_full(dh, w)) > 1e-3


def test_two_real_frames_through_one_complex_transform():
    """The identity the kernel uses: with Z = DFT(g_a + i g_b), M[k] = conj Z[-k], S = (conj X_a + conj X_b) / 2 and
    D = (conj X_a - conj X_b) / 2, IDFT(Z S + M D) = dh_a + i dh_b."""
    H, u, g = nr.inputs(1, 2)
    gh, x = nr.g_hat(g)[0], nr.noise_frames(u, 2)
    Z = np.fft.fft(gh[0:256] + 1j * gh[128:384])
    M = np.conj(Z[(-np.arange(256)) % 256])
    Xa, Xb = np.fft.fft(x[0]), np.fft.fft(x[1])
    p = np.fft.ifft(Z * (np.conj(Xa) + np.conj(Xb)) / 2 + M * (np.conj(Xa) - np.conj(Xb)) / 2)
    dh = nr.grad_taps_explicit(u, g)[0]
    assert nr.rel_l2(p.real, dh[0]) <= 1e-12 and nr.rel_l2(p.imag, dh[1]) <= 1e-12
