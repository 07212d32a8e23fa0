"""Float64 numpy restatement of the frame MLP's backward, written from the definition and not from the kernels.
Reference forward (models/modules/dynamic.py:11-40) per frame (b, t), layers i = 0 .. depth-1, a_{-1} = x:

    z_i[o]  = sum_k W_i[o, k] a_{i-1}[k] + b_i[o]
    n_i[c]  = (z_i[c] - mean_c z_i) rstd_i,   rstd_i = 1 / sqrt(var_c z_i + eps)     (biased variance, i < depth-1)
    v_i[c]  = gamma_i[c] n_i[c] + beta_i[c],  a_i[c] = v_i[c] if v_i[c] > 0 else slope v_i[c]
    y       = z_{depth-1}

and for g = dL/dy, dz_{depth-1} = g, walking i downwards:

    dW_i[o, k]  = sum_{b,t} dz_i[b, o, t] a_{i-1}[b, k, t]      db_i[o] = sum_{b,t} dz_i[b, o, t]
    da_{i-1}[k] = sum_o W_i[o, k] dz_i[o]                       (da_{-1} = dL/dx)
    dv_i[c]     = da_i[c] (1 if v_i[c] > 0 else slope)          (torch's convention at v = 0: slope)
    dbeta_i[c]  = sum_{b,t} dv_i[b, c, t]     dgamma_i[c] = sum_{b,t} dv_i[b, c, t] n_i[b, c, t]     dn_i[c] = gamma_i[c] dv_i[c]
    dz_i[c]     = rstd_i (dn_i[c] - mean_c dn_i - n_i[c] mean_c(dn_i n_i))

Also the deterministic parameters and inputs of the tests, the distance they use, and torch's autograd through the reference
expression (conv1d, layer_norm, leaky_relu)."""
import functools

import numpy as np

EPS, SLOPE = 1e-5, 0.01
MARGIN = 1e-3

# (in, hidden, out, depth) and the (B, T) each one is run at (tests/test_gpu_td_mlp_grad.py says why)
PACKAGED = ((128, 128, 129, 4), (128, 128, 256, 4))
SIZES = PACKAGED + ((5, 7, 3, 3), (40, 72, 33, 3), (6, 6, 9, 1))
CASES = (tuple((s, bt) for s in SIZES for bt in ((1, 1), (3, 33))) + tuple((s, (2, 500)) for s in PACKAGED)
         + (((5, 7, 3, 3), (3, 700)),))


def widths(sizes):
    """[(cout, cin)] per layer"""
    cin, hidden, cout, depth = sizes
    w = [cin] + [hidden] * (depth - 1) + [cout]
    return [(w[i + 1], w[i]) for i in range(depth)]


def _seed(*ints):
    return int(np.random.SeedSequence([int(i) for i in ints]).generate_state(1)[0])


def params(sizes, seed=0):
    """(W, b, gamma, beta): lists of float32 arrays.  W ~ normal / sqrt(cin); b, beta ~ 0.1 normal; gamma ~ 1 + 0.1 normal, so that
    the LayerNorm's affine part is never the identity"""
    rng = np.random.default_rng(_seed(1, seed, *sizes))
    W, b, gam, bet = [], [], [], []
    shapes = widths(sizes)
    for i, (cout, cin) in enumerate(shapes):
        W.append((rng.standard_normal((cout, cin)) / np.sqrt(cin)).astype(np.float32))
        b.append((0.1 * rng.standard_normal(cout)).astype(np.float32))
        if i < len(shapes) - 1:
            gam.append((1.0 + 0.1 * rng.standard_normal(cout)).astype(np.float32))
            bet.append((0.1 * rng.standard_normal(cout)).astype(np.float32))
    return W, b, gam, bet


def _f64(arrays):
    return [np.asarray(a, dtype=np.float64) for a in arrays]


def forward_all(x, W, b, gam, bet, eps=EPS, slope=SLOPE):
    """float64 forward that keeps what the backward needs: (y, a[-1 .. depth-2] as a list starting with x, n, rstd, v)"""
    W, b, gam, bet = _f64(W), _f64(b), _f64(gam), _f64(bet)
    a = [np.asarray(x, dtype=np.float64)]
    n, rstd, v = [], [], []
    depth = len(W)
    for i in range(depth):
        z = np.einsum("ok,bkt->bot", W[i], a[-1]) + b[i][None, :, None]
        if i == depth - 1:
            return z, a, n, rstd, v
        mean = z.mean(axis=1, keepdims=True)
        var = ((z - mean) ** 2).mean(axis=1, keepdims=True)
        r = 1.0 / np.sqrt(var + eps)
        ni = (z - mean) * r
        vi = gam[i][None, :, None] * ni + bet[i][None, :, None]
        n.append(ni)
        rstd.append(r)
        v.append(vi)
        a.append(np.where(vi > 0, vi, slope * vi))


def forward(x, W, b, gam, bet, eps=EPS, slope=SLOPE):
    return forward_all(x, W, b, gam, bet, eps, slope)[0]


def backward(x, g, W, b, gam, bet, eps=EPS, slope=SLOPE):
    """(dx, dW, db, dgamma, dbeta) in float64, the lists in layer order"""
    _, a, n, rstd, v = forward_all(x, W, b, gam, bet, eps, slope)
    Wd, gamd = _f64(W), _f64(gam)
    depth = len(W)
    dW, db, dgam, dbet = [None] * depth, [None] * depth, [None] * (depth - 1), [None] * (depth - 1)
    dz = np.asarray(g, dtype=np.float64)
    for i in range(depth - 1, -1, -1):
        dW[i] = np.einsum("bot,bkt->ok", dz, a[i])                 # a[i] is a_{i-1}
        db[i] = np.einsum("bot->o", dz)
        da = np.einsum("ok,bot->bkt", Wd[i], dz)
        if i == 0:
            return da, dW, db, dgam, dbet
        j = i - 1
        dv = da * np.where(v[j] > 0, 1.0, slope)
        dbet[j] = np.einsum("bct->c", dv)
        dgam[j] = np.einsum("bct,bct->c", dv, n[j])
        dn = gamd[j][None, :, None] * dv
        m1 = dn.mean(axis=1, keepdims=True)
        m2 = (dn * n[j]).mean(axis=1, keepdims=True)
        dz = rstd[j] * (dn - m1 - n[j] * m2)


def min_abs_v(x, W, b, gam, bet):
    """(B, T): the smallest |v_i| of each frame over layers and channels (inf for depth 1)"""
    v = forward_all(x, W, b, gam, bet)[4]
    out = np.full((np.shape(x)[0], np.shape(x)[2]), np.inf)
    for vi in v:
        out = np.minimum(out, np.abs(vi).min(axis=1))
    return out


@functools.lru_cache(maxsize=None)
def _inputs(sizes, B, T, seed):
    P = params(sizes, seed)
    rng = np.random.default_rng(_seed(2, seed, B, T, *sizes))
    x = rng.standard_normal((B, sizes[0], T)).astype(np.float32)
    g = rng.standard_normal((B, sizes[2], T)).astype(np.float32)
    rounds = 0
    while True:
        bad = min_abs_v(x, *P) < MARGIN
        if not bad.any():
            break
        rounds += 1
        for bb, tt in zip(*np.nonzero(bad)):
            x[bb, :, tt] = rng.standard_normal(sizes[0]).astype(np.float32)
    x.setflags(write=False)
    g.setflags(write=False)
    return x, g, rounds


def inputs(sizes, B, T, seed=0):
    """(x (B, in, T), g (B, out, T)) float32, normal, seeded, for the net params(sizes, seed).  LeakyReLU' jumps at 0: an fp32
    forward that lands on the other side of a float64 v changes that gradient by a factor of 100, which would be a property of
    the input and not of the kernel - so any frame with some |v_i| < 1e-3 in the float64 forward (three orders above the fp32
    forward error) gets a fresh draw, until there is none."""
    return _inputs(tuple(sizes), B, T, seed)[:2]


def redraw_rounds(sizes, B, T, seed=0):
    return _inputs(tuple(sizes), B, T, seed)[2]


def rel_l2(a, ref):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(a - ref) / np.linalg.norm(ref))


def flat(dx, dW, db, dgam, dbet):
    """the order the op returns: [dx] + dW + db + dgamma + dbeta"""
    return [dx] + list(dW) + list(db) + list(dgam) + list(dbet)


def names(depth):
    return (["x"] + [f"W{i}" for i in range(depth)] + [f"b{i}" for i in range(depth)] + [f"gamma{i}" for i in range(depth - 1)]
            + [f"beta{i}" for i in range(depth - 1)])


def torch_reference(x, W, b, gam, bet, eps=EPS, slope=SLOPE):
    """the reference expression on torch tensors of one dtype"""
    import torch

    F = torch.nn.functional
    for i in range(len(W)):
        x = F.conv1d(x, W[i][:, :, None], b[i])
        if i < len(W) - 1:
            x = F.leaky_relu(F.layer_norm(x.transpose(1, 2), (x.shape[1],), gam[i], bet[i], eps).transpose(1, 2), slope)
    return x


def torch_autograd_grads(x, g, W, b, gam, bet, dtype):
    """[dx] + dW + db + dgamma + dbeta from torch's CPU autograd through the reference expression in `dtype`, as numpy arrays"""
    import torch

    leaf = lambda a: torch.tensor(np.array(a), dtype=dtype, requires_grad=True)
    xt = leaf(x)
    Wt, bt, gt, lt = ([leaf(a) for a in lst] for lst in (W, b, gam, bet))
    y = torch_reference(xt, Wt, bt, gt, lt)
    y.backward(torch.tensor(np.array(g), dtype=dtype))
    return [t.grad.numpy() for t in [xt] + Wt + bt + gt + lt]


@functools.lru_cache(maxsize=None)
def reference(sizes, B, T, seed=0):
    """(float64 gradients in the op's order, the relative L2 of torch's float32 CPU autograd from each); read-only, shared"""
    import torch

    P = params(sizes, seed)
    x, g = inputs(sizes, B, T, seed)
    want = flat(*backward(x, g, *P))
    f32 = torch_autograd_grads(x, g, *P, torch.float32)
    for a in want:
        a.setflags(write=False)
    return want, [rel_l2(a, w) for a, w in zip(f32, want)]
