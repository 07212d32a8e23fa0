"""Float64 numpy restatement of the control encoder's backward, written from the definition and not from the
kernels.  Reference forward (models/neural_waveshaping.py:17-26; torch's nn.GRU, gate order [r; z; n], then Conv1d(k=1)) per
utterance b, t = 0 .. T-1, x_t in R^2, h_{-1} = h0 (zeros when absent), H = 128:

    r[j] = sigmoid(sum_c W_ih[j, c] x_t[c] + b_ih[j] + sum_k W_hh[j, k] h_{t-1}[k] + b_hh[j])
    z[j] = sigmoid(sum_c W_ih[H + j, c] x_t[c] + b_ih[H + j] + sum_k W_hh[H + j, k] h_{t-1}[k] + b_hh[H + j])
    q[j] = sum_k W_hh[2H + j, k] h_{t-1}[k] + b_hh[2H + j]
    n[j] = tanh(sum_c W_ih[2H + j, c] x_t[c] + b_ih[2H + j] + r[j] q[j])
    h_t[j] = (1 - z[j]) n[j] + z[j] h_{t-1}[j]            emb[b, e, t] = sum_j W_p[e, j] h_t[j] + b_p[e]

Backward for G_t = dL/d(h_t) and an optional dL/d(h_T), in two forms that must agree: `backward_direct` walks the chain rule gate by
gate; `backward_coef` first forms the coefficients that depend on the forward only,

    c_n = (1 - z)(1 - n^2)    c_z = (h_{t-1} - n) z (1 - z)    c_q = c_n r    c_r = c_n q r (1 - r)

and then  dh_t = G_t + carry_{t+1},  u_t = [c_r; c_z; c_n] dh_t,  v_t = [c_r; c_z; c_q] dh_t,  carry_t = z dh_t + W_hh^T v_t,
dW_ih = sum u_t (x) x_t,  db_ih = sum u_t,  dW_hh = sum v_t (x) h_{t-1},  db_hh = sum v_t,  dL/d(x_t) = W_ih^T u_t,  dL/d(h0) = carry_0.

Also the cases, the deterministic parameters and inputs of the tests, the distance they use, and torch's autograd through
nn.GRU + Conv1d in a given dtype."""
import functools
import os

import numpy as np

H = 128
# (B, T): the minimum (h0 is the only history); one carried step; an odd batch, one frame past a 32-frame tile (the only length
# the backward kernels stage by); the training length; one frame block past the forward's 1024-frame staging; 66 (utterance,
# chunk) units, so nine dW_hh partials: a second trip of the reduction's p += 8 and a count that is no multiple of eight
SHAPES = ((1, 1), (1, 2), (3, 33), (2, 500), (1, 1030), (3, 700))
SETS = ("packaged", "default")
# (parameter set, (B, T), with h0 and grad_hT)
CASES = tuple((s, bt, st) for s in SETS for bt in SHAPES for st in (True, False))
IDS = [f"{s}-{b}x{t}-{'state' if st else 'nostate'}" for s, (b, t), st in CASES]
NAMES = ("x", "h0", "W_ih", "W_hh", "b_ih", "b_hh")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "weights_vn.npz")


def _seed(*ints):
    return int(np.random.SeedSequence([int(i) for i in ints]).generate_state(1)[0])


@functools.lru_cache(maxsize=None)
def params(which):
    """(W_ih (384, 2), W_hh (384, 128), b_ih, b_hh, W_p (128, 128), b_p) as float32: 'packaged' = embedding.* of
    tests/golden/weights_vn.npz; 'default' = torch's default nn.GRU / Conv1d initialisation under a fixed seed"""
    if which == "packaged":
        z = np.load(GOLDEN)
        keys = [f"embedding.gru.{k}" for k in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]
        out = [z[k].astype(np.float32) for k in keys]
        return tuple(out + [z["embedding.proj.weight"].astype(np.float32).reshape(H, H), z["embedding.proj.bias"].astype(np.float32)])
    import torch

    assert which == "default"
    gen_state = torch.random.get_rng_state()
    torch.manual_seed(1234)
    gru, proj = torch.nn.GRU(2, H, batch_first=True), torch.nn.Conv1d(H, H, 1)
    torch.random.set_rng_state(gen_state)
    out = [p.detach().numpy().copy() for p in (gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0)]
    return tuple(out + [proj.weight.detach().numpy().reshape(H, H).copy(), proj.bias.detach().numpy().copy()])


def inputs(which, B, T, state, seed=0):
    """(x (B, 2, T), h0 (B, 128) or None, G (B, T, 128) = dL/d(gru_out), grad_hT (B, 128) or None) as float32.
    'packaged': x[b, c, t] = 0.5 + 0.25 sin(2 pi t / (97 (1, 1.7)[c]) + b) + 0.02 normal - the range and smoothness of the normalised
    F0 and loudness the model is fed (under white noise the packaged recurrence is chaotic and float32 itself is 1e-4 .. 6e-3 from
    float64); 'default': x normal.  h0 = 0.5 normal, grad_hT and G normal."""
    rng = np.random.default_rng(_seed(2, seed, SETS.index(which), B, T, int(state)))
    if which == "packaged":
        t = np.arange(T)[None, None, :]
        per = 97.0 * np.array([1.0, 1.7])[None, :, None]
        x = 0.5 + 0.25 * np.sin(2 * np.pi * t / per + np.arange(B)[:, None, None]) + 0.02 * rng.standard_normal((B, 2, T))
    else:
        x = rng.standard_normal((B, 2, T))
    G = rng.standard_normal((B, T, H))
    h0 = 0.5 * rng.standard_normal((B, H)) if state else None
    ghT = rng.standard_normal((B, H)) if state else None
    f32 = lambda a: None if a is None else a.astype(np.float32)
    return f32(x), f32(h0), f32(G), f32(ghT)


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def _sigmoid(a):
    return 1.0 / (1.0 + np.exp(-a))


def forward(x, h0, W_ih, W_hh, b_ih, b_hh):
    """-> dict of (B, T, 128) float64 arrays: h (= gru_out), hprev, r, z, n, q"""
    x, h0, W_ih, W_hh, b_ih, b_hh = map(_f64, (x, h0, W_ih, W_hh, b_ih, b_hh))
    B, _, T = x.shape
    out = {k: np.zeros((B, T, H)) for k in ("h", "hprev", "r", "z", "n", "q")}
    h = np.zeros((B, H)) if h0 is None else h0.copy()
    for t in range(T):
        gi = np.einsum("jc,bc->bj", W_ih, x[:, :, t]) + b_ih
        gh = np.einsum("jk,bk->bj", W_hh, h) + b_hh
        r = _sigmoid(gi[:, 0:H] + gh[:, 0:H])
        z = _sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        q = gh[:, 2 * H:]
        n = np.tanh(gi[:, 2 * H:] + r * q)
        out["hprev"][:, t], out["r"][:, t], out["z"][:, t], out["n"][:, t], out["q"][:, t] = h, r, z, n, q
        h = (1.0 - z) * n + z * h
        out["h"][:, t] = h
    return out


def backward_direct(x, h0, G, ghT, W_ih, W_hh, b_ih, b_hh):
    """the chain rule gate by gate -> (dx (B, 2, T), dh0 (B, 128), dW_ih, dW_hh, db_ih, db_hh)"""
    F = forward(x, h0, W_ih, W_hh, b_ih, b_hh)
    x, G, ghT, W_ih, W_hh = map(_f64, (x, G, ghT, W_ih, W_hh))
    B, _, T = x.shape
    dx = np.zeros((B, 2, T))
    dW_ih, dW_hh, db_ih, db_hh = np.zeros((3 * H, 2)), np.zeros((3 * H, H)), np.zeros(3 * H), np.zeros(3 * H)
    carry = np.zeros((B, H)) if ghT is None else ghT.copy()
    for t in range(T - 1, -1, -1):
        r, z, n, q, hprev = (F[k][:, t] for k in ("r", "z", "n", "q", "hprev"))
        dh = G[:, t] + carry
        dn = dh * (1.0 - z)                       # h = (1 - z) n + z hprev
        dz = dh * (hprev - n)
        da_n = dn * (1.0 - n * n)                 # n = tanh(a_n), a_n = i_n + r q
        dr = da_n * q
        dq = da_n * r
        da_r = dr * r * (1.0 - r)
        da_z = dz * z * (1.0 - z)
        d_in = np.concatenate([da_r, da_z, da_n], axis=1)       # (B, 384): gradient of the input-side pre-activations
        d_hid = np.concatenate([da_r, da_z, dq], axis=1)        # of the hidden-side pre-activations
        dW_ih += np.einsum("bj,bc->jc", d_in, x[:, :, t])
        db_ih += d_in.sum(axis=0)
        dW_hh += np.einsum("bj,bk->jk", d_hid, hprev)
        db_hh += d_hid.sum(axis=0)
        dx[:, :, t] = np.einsum("jc,bj->bc", W_ih, d_in)
        carry = dh * z + np.einsum("jk,bj->bk", W_hh, d_hid)
    return dx, carry, dW_ih, dW_hh, db_ih, db_hh


def coefficients(F):
    z, r, n, q, hprev = F["z"], F["r"], F["n"], F["q"], F["hprev"]
    c_n = (1.0 - z) * (1.0 - n * n)
    return {"z": z, "c_n": c_n, "c_z": (hprev - n) * z * (1.0 - z), "c_q": c_n * r, "c_r": c_n * q * r * (1.0 - r)}


def backward_coef(x, h0, G, ghT, W_ih, W_hh, b_ih, b_hh):
    """the coefficient form: a parallel pass for the coefficients, the serial dh_t, then parallel sums"""
    F = forward(x, h0, W_ih, W_hh, b_ih, b_hh)
    c = coefficients(F)
    x, G, ghT, W_ih, W_hh = map(_f64, (x, G, ghT, W_ih, W_hh))
    B, _, T = x.shape
    dh = np.zeros((B, T, H))
    carry = np.zeros((B, H)) if ghT is None else ghT.copy()
    for t in range(T - 1, -1, -1):
        dh[:, t] = G[:, t] + carry
        v = np.concatenate([c["c_r"][:, t], c["c_z"][:, t], c["c_q"][:, t]], axis=1) * np.tile(dh[:, t], (1, 3))
        carry = c["z"][:, t] * dh[:, t] + np.einsum("jk,bj->bk", W_hh, v)
    u = np.concatenate([c["c_r"], c["c_z"], c["c_n"]], axis=2) * np.tile(dh, (1, 1, 3))       # (B, T, 384)
    v = np.concatenate([c["c_r"], c["c_z"], c["c_q"]], axis=2) * np.tile(dh, (1, 1, 3))
    dW_ih = np.einsum("btj,bct->jc", u, x)
    dW_hh = np.einsum("btj,btk->jk", v, F["hprev"])
    dx = np.einsum("jc,btj->bct", W_ih, u)
    return dx, carry, dW_ih, dW_hh, u.sum(axis=(0, 1)), v.sum(axis=(0, 1))


def module_backward(x, h0, g_emb, ghT, P):
    """ControlModule: grad_emb (B, 128, T) -> (dx, dh0, dW_ih, dW_hh, db_ih, db_hh, dW_p, db_p) through proj and the recurrence"""
    W_ih, W_hh, b_ih, b_hh, W_p, b_p = P
    F = forward(x, h0, W_ih, W_hh, b_ih, b_hh)
    g = _f64(g_emb)
    G = np.einsum("ej,bet->btj", _f64(W_p), g)
    dW_p = np.einsum("bet,btj->ej", g, F["h"])
    return backward_coef(x, h0, G, ghT, W_ih, W_hh, b_ih, b_hh) + (dW_p, g.sum(axis=(0, 2)))


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    den = np.sqrt(np.sum(b * b))
    num = np.sqrt(np.sum((a - b) ** 2))
    return float(num / den) if den > 0 else float(num)


def torch_modules(P, dtype):
    """(nn.GRU(2, 128, batch_first), nn.Conv1d(128, 128, 1)) on the CPU with the parameters P in `dtype`"""
    import torch

    gru, proj = torch.nn.GRU(2, H, batch_first=True).to(dtype), torch.nn.Conv1d(H, H, 1).to(dtype)
    with torch.no_grad():
        for p, a in zip((gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0), P[:4]):
            p.copy_(torch.as_tensor(np.asarray(a), dtype=dtype))
        proj.weight.copy_(torch.as_tensor(np.asarray(P[4]), dtype=dtype).reshape(H, H, 1))
        proj.bias.copy_(torch.as_tensor(np.asarray(P[5]), dtype=dtype))
    return gru, proj


def torch_autograd_grads(x, h0, G, ghT, P, dtype, g_emb=None):
    """torch's CPU autograd through nn.GRU (and, with g_emb (B, 128, T) in place of G, through Conv1d behind it) in `dtype`:
    [dx, dh0, dW_ih, dW_hh, db_ih, db_hh] (+ [dW_p, db_p]) as float64 arrays"""
    import torch

    gru, proj = torch_modules(P, dtype)
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)
    xt = t(x).transpose(1, 2).contiguous().requires_grad_()                 # (B, T, 2)
    B = xt.shape[0]
    h0t = (t(h0) if h0 is not None else torch.zeros(B, H, dtype=dtype)).reshape(1, B, H).requires_grad_()
    out, hT = gru(xt, h0t)
    if g_emb is None:
        loss = (out * t(G)).sum()
    else:
        loss = (proj(out.transpose(1, 2)) * t(g_emb)).sum()
    if ghT is not None:
        loss = loss + (hT[0] * t(ghT)).sum()
    leaves = [xt, h0t, gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0]
    if g_emb is not None:
        leaves += [proj.weight, proj.bias]
    grads = torch.autograd.grad(loss, leaves)
    outs = [g.detach().double().numpy() for g in grads]
    outs[0] = outs[0].transpose(0, 2, 1)
    outs[1] = outs[1].reshape(B, H)
    if g_emb is not None:
        outs[6] = outs[6].reshape(H, H)
    return outs


@functools.lru_cache(maxsize=None)
def reference(which, B, T, state):
    """(float64 restatement [dx, dh0, dW_ih, dW_hh, db_ih, db_hh], distance of torch's float32 CPU autograd from it per tensor),
    on inputs(which, B, T, state); computed once per case and shared"""
    import torch

    P = params(which)
    x, h0, G, ghT = inputs(which, B, T, state)
    want = backward_coef(x, h0, G, ghT, *P[:4])
    got = torch_autograd_grads(x, h0, G, ghT, P, torch.float32)
    return want, [rel_l2(g, w) for g, w in zip(got, want)]
