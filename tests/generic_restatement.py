"""Plain numpy float64 restatements of two stages of the runtime-size path (csrc/generic.hip nws_g_gru, csrc/stages.hip
nws_td_mlp), any sizes, no torch in the arithmetic: the yard-stick the stage tests of test_gpu_generic_variants.py hold the
kernels to, itself held to torch in float64 by test_cpu_generic_variants.py."""
import numpy as np


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def gru_float64(w_ih, w_hh, b_ih, b_hh, control, h0=None):
    """torch.nn.GRU(C_in, H, batch_first=True) (gate order r, z, n; h' = (h - n) z + n) on the FIRST C_in channels of
    control (B, C_total, T), C_in = w_ih.shape[1].  Returns (out (B, T, H), hT (B, H))."""
    Wi, Wh, bi, bh = _f64(w_ih), _f64(w_hh), _f64(b_ih), _f64(b_hh)
    H, C_in = Wh.shape[1], Wi.shape[1]
    control = _f64(control)
    B, C_total, T = control.shape
    assert C_total >= C_in and Wi.shape[0] == 3 * H and Wh.shape[0] == 3 * H
    h = np.zeros((B, H)) if h0 is None else _f64(h0).reshape(B, H).copy()
    out = np.zeros((B, T, H))

    def sig(x):
        return 1.0 / (1.0 + np.exp(-x))

    for t in range(T):
        gi = control[:, :C_in, t] @ Wi.T + bi
        gh = h @ Wh.T + bh
        r, z = sig(gi[:, :H] + gh[:, :H]), sig(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = np.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        h = (h - n) * z + n
        out[:, t] = h
    return out, h


def td_mlp_float64(x, weights, biases, ln_g, ln_b, eps=1e-5, slope=0.01):
    """TimeDistributedMLP on (B, C, T): [Conv1x1 -> LayerNorm over channels (biased variance) -> LeakyReLU] for every layer but
    the last, which is a bare Conv1x1.  weights[i]: (C_out, C_in) or (C_out, C_in, 1); ln_g / ln_b: one entry per hidden layer."""
    x = _f64(x)
    depth = len(weights)
    for i in range(depth):
        W = _f64(weights[i]).reshape(np.shape(weights[i])[0], -1)
        x = np.einsum("oc,bct->bot", W, x) + _f64(biases[i])[None, :, None]
        if i < depth - 1:
            mean = x.mean(axis=1, keepdims=True)
            var = ((x - mean) ** 2).mean(axis=1, keepdims=True)
            x = (x - mean) / np.sqrt(var + eps) * _f64(ln_g[i])[None, :, None] + _f64(ln_b[i])[None, :, None]
            x = np.where(x > 0.0, x, slope * x)
    return x
