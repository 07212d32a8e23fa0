"""-m gpu: the backward of the oscillator branch at any bank size (csrc/g_newt_grad.hip through the g_newt_grad op, NEWT.vjp and
NEWT.differentiable on the runtime-size path) against torch's float64 autograd through the reference expression
(tests/g_newt_grad_restatement.py, which lists the size sets (S, W, D), the shapes (B, T) and the inputs).

Bar, for every returned tensor of the op and of NEWT.vjp: the relative L2 from float64 is at most 10 x the distance of torch's
float32 CPU autograd from the same float64 result on the same inputs (floored at 2^-24, one float32 rounding), and never beyond the
project's parity bar, 1e-4 (FACTOR, CAP of test_gpu_newt_grad.py).  The kernel's FiLM parameters come from the forward MLP kernel's
own float32 film; that is part of what is measured.

The measured figures (kernel | torch float32 CPU autograd | ratio per case) are in DESIGN.md 3.20."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import g_newt_grad_restatement as gr
from gpu_util import dev, record

pytestmark = pytest.mark.gpu

FACTOR = 10.0
CAP = 1e-4
UNSUPPORTED, BAD_ARG = -1, -2


def _nws():
    import nws_amd as nws

    return nws


def _binding():
    from nws_amd.engine import binding

    return binding()


@functools.lru_cache(maxsize=None)
def _module(S, W, D):
    """a NEWT of the size set with the restatement's parameters on the device"""
    m = gr.new_module(S, W, D)
    m.load_state_dict({k: torch.as_tensor(np.array(v)) for k, v in gr.params(S, W, D).items()})
    return m.cuda()


def _op(sizes, exc, film, g, want_exciter=True, want_params=True):
    m = _module(*sizes)
    with torch.no_grad():
        return list(_binding().g_newt_grad(m._g_shaper(), exc, film, g, m.mixer[0].weight.detach(), m.mixer[0].bias.detach(),
                                           want_exciter, want_params))


def _check(tag, names, got, want, yard):
    dists = {}
    for name, o in zip(names, got):
        w = want[name]
        assert tuple(o.shape) == w.shape and o.dtype == torch.float32 and o.is_cuda and not o.requires_grad, name
        dists[name] = gr.rel_l2(o.cpu().numpy(), w)
        print(f"{tag} {name}: kernel {dists[name]:.2e} | torch float32 autograd {yard[name]:.2e} | ratio {dists[name] / yard[name]:.2f}")
    worst = max(names, key=lambda n: dists[n] / yard[n])
    record(f"g_newt_grad/{tag}", worst=worst, worst_kernel=dists[worst], worst_torch_f32=yard[worst], worst_ratio=dists[worst] / yard[worst],
           **{n: d for n, d in dists.items()}, **{n + "_torch_f32": yard[n] for n in names})
    return dists


@pytest.mark.parametrize("sizes,shape", gr.CASES, ids=gr.IDS)
def test_every_gradient_against_float64(sizes, shape):
    (S, W, D), (B, T) = sizes, shape
    exciter, emb, g = gr.inputs(S, W, D, B, T)
    want, yard = gr.reference(S, W, D, B, T)
    m = _module(S, W, D)
    ed, cd, gd = dev(exciter), dev(emb), dev(g)
    with torch.no_grad():
        film = m.mlp(cd)
    op_names, rate_keys, param_keys = gr.op_names(D), gr.rate_keys(D), gr.param_keys(D)
    out = _op(sizes, ed, film, gd)
    assert len(out) == len(op_names) == 2 * D + 5
    tag = f"{S}x{W}x{D}_{B}x{T}"
    d_op = _check(f"op_{tag}", op_names, out, want, yard)
    if (S, W, D) == (64, 8, 4):
        ge, gemb, grads = m.vjp(gd, ed, cd)               # NEWT.vjp takes this size set to newt_grad: the same bar, their distance
        assert m._need_backward() is True
        mutual = {n: gr.rel_l2(o.cpu().numpy(), grads[n].cpu().numpy() if n in grads else ge.cpu().numpy())
                  for n, o in zip(op_names[1:], out[1:])}
        print("g_newt_grad against newt_grad:", " ".join(f"{n} {v:.2e}" for n, v in mutual.items()))
        record(f"g_newt_grad/against_newt_grad_{B}x{T}", **mutual)
    else:
        ge, gemb, grads = m.vjp(gd, ed, cd)
        assert m._need_backward() is False
        assert torch.equal(ge, out[1]) and all(torch.equal(grads[k], o) for k, o in zip(rate_keys, out[2:]))    # vjp = the op, key by key
    assert set(grads) == set(param_keys) == set(k for k, _ in m.named_parameters())
    names = ("exciter", "emb") + param_keys
    d_vjp = _check(f"vjp_{tag}", names, [ge, gemb] + [grads[k] for k in param_keys], want, yard)

    # exact cases: equal inputs, equal bits; fewer outputs leave the others' bits alone; no gradient in, none out
    again = _op(sizes, ed, film, gd)
    assert all(torch.equal(a, o) for a, o in zip(again, out))
    only = _op(sizes, ed, film, gd, want_exciter=True, want_params=False)
    assert len(only) == 2 and torch.equal(only[0], out[0]) and torch.equal(only[1], out[1])
    only = _op(sizes, ed, film, gd, want_exciter=False, want_params=True)
    assert len(only) == 2 * D + 4 and torch.equal(only[0], out[0]) and all(torch.equal(a, o) for a, o in zip(only[1:], out[2:]))
    only = _op(sizes, ed, film, gd, want_exciter=False, want_params=False)
    assert len(only) == 1 and torch.equal(only[0], out[0])
    for we, wp in ((True, True), (False, False)):
        for o in _op(sizes, ed, film, torch.zeros_like(gd), we, wp):
            assert torch.equal(o, torch.zeros_like(o))
    ge0, gemb0, none = m.vjp(gd, ed, cd, want_params=False, want_exciter=False)
    assert ge0 is None and none == {} and torch.equal(gemb0, gemb)

    for dists, names_ in ((d_op, op_names), (d_vjp, names)):
        for name in names_:
            assert dists[name] <= FACTOR * yard[name] and dists[name] <= CAP, (name, dists[name], yard[name])


# ---- refusals: decided on the host, before any launch -------------------------------------------------------------------------------
def _raw(sizes, exc, film, g, null=(), ws_short=False, drop_param=None, hop=128, width=None, depth=None):
    """nws_g_newt_grad through ctypes: (return code, every output tensor filled with NaN beforehand, the workspace)"""
    from nws_amd import _lib

    S, W, D = sizes
    B, _, N = exc.shape
    T = film.shape[2]
    m = _module(*sizes)
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    outs = [nan(B, 4 * S, T), nan(B, S, N)] + [nan(*sh) for sh in _lib.g_newt_grad_shapes(S, W, D)]
    L = _lib.lib()
    d = _lib.NwsShaperDesc.from_buffer_copy(m._g_shaper().numpy())
    nbytes = L.nws_g_newt_grad_workspace_bytes(C.byref(d), B, T, 1)
    assert nbytes > L.nws_g_newt_grad_workspace_bytes(C.byref(d), B, T, 0) > 0
    if width is not None:
        d.width = width
    if depth is not None:
        d.depth = depth
    ws = torch.full((nbytes,), 0x7f, dtype=torch.uint8, device="cuda")
    a = dict(exciter=exc.data_ptr(), film=film.data_ptr(), grad_out=g.data_ptr(), grad_film=outs[0].data_ptr(), ws=ws.data_ptr())
    for k in null:
        a[k] = None
    gp = [o.data_ptr() for o in outs[2:]]
    if drop_param is not None:
        gp[drop_param] = None
    gp += [None] * 4                                       # room for a descriptor that claims a greater depth
    rc = L.nws_g_newt_grad(C.byref(d), m.mixer[0].weight.data_ptr(), m.mixer[0].bias.data_ptr(), a["exciter"], a["film"], a["grad_out"],
                           B, T, hop, outs[1].data_ptr(), a["grad_film"], (C.c_void_p * len(gp))(*gp), a["ws"],
                           nbytes - 4 if ws_short else nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, outs, ws


def test_refusals_return_before_any_launch():
    sizes, (B, T) = (5, 3, 3), (3, 3)
    exciter, emb, g = gr.inputs(*sizes, B, T)
    ed, gd = dev(exciter), dev(g)
    with torch.no_grad():
        film = _module(*sizes).mlp(dev(emb))
    refused = [(dict(null=(k,)), BAD_ARG) for k in ("exciter", "film", "grad_out", "grad_film", "ws")]
    refused += [(dict(ws_short=True), BAD_ARG), (dict(drop_param=3), BAD_ARG), (dict(drop_param=2 * 3 + 2), BAD_ARG),
                (dict(width=17), UNSUPPORTED), (dict(depth=5), UNSUPPORTED), (dict(hop=64), UNSUPPORTED)]
    for kw, code in refused:
        rc, outs, ws = _raw(sizes, ed, film, gd, **kw)
        assert rc == code, (kw, rc)
        assert all(torch.isnan(o).all() for o in outs), kw                   # untouched
        assert bool((ws == 0x7f).all()), kw
    rc, outs, _ = _raw(sizes, ed, film, gd)                                   # and a valid call right after gives the op's bits
    assert rc == 0
    assert all(torch.equal(a, o) for a, o in zip(outs, _op(sizes, ed, film, gd)))


# ---- autograd -----------------------------------------------------------------------------------------------------------------------
def test_autograd_carries_the_bits_of_vjp():
    sizes, (B, T) = (5, 3, 3), (3, 3)
    plain = _module(*sizes)
    mod = copy.deepcopy(plain)
    mod.differentiable = True
    exciter, emb, g = gr.inputs(*sizes, B, T)
    ed, cd, gd = dev(exciter), dev(emb), dev(g)
    with torch.no_grad():
        want_y = plain(ed, cd)
    want_e, want_c, want = plain.vjp(gd, ed, cd)

    # the flag off: today's forward - no graph, and an input that requires grad is refused
    assert plain.differentiable is False and not plain(ed, cd).requires_grad
    for args in ((ed.clone().requires_grad_(), cd), (ed, cd.clone().requires_grad_())):
        with pytest.raises(RuntimeError, match="inference-only"):
            plain(*args)

    e_leaf, c_leaf = ed.clone().requires_grad_(), cd.clone().requires_grad_()
    y = mod(e_leaf, c_leaf)
    assert y.requires_grad and torch.equal(y.detach(), want_y)               # the flag-less module's bits
    (y * gd).sum().backward()
    assert torch.equal(e_leaf.grad, want_e) and torch.equal(c_leaf.grad, want_c)
    named = dict(mod.named_parameters())
    assert set(named) == set(want) and len(named) == 14 + 2 * 3 + 3
    for k, p in named.items():
        assert p.grad is not None and p.grad.shape == p.shape and torch.equal(p.grad, want[k].view_as(p)), k

    # no parameter requires grad: the data gradients alone, the same bits; nothing requires grad: the plain forward
    for p in mod.parameters():
        p.requires_grad_(False)
        p.grad = None
    e_leaf.grad = c_leaf.grad = None
    (mod(e_leaf, cd) * gd).sum().backward()
    assert torch.equal(e_leaf.grad, want_e) and c_leaf.grad is None and all(p.grad is None for p in mod.parameters())
    assert not mod(ed, cd).requires_grad and torch.equal(mod(ed, cd), want_y)
    with torch.no_grad():                                                     # vjp does not look at the flag or the grad mode
        assert torch.equal(mod.vjp(gd, ed, cd)[1], want_c) and not mod(e_leaf, cd).requires_grad
    # one parameter alone: the inputs and the others get nothing
    mod.shaping_fn.net[2].weight.requires_grad_(True)
    y = mod(ed, cd)
    assert y.requires_grad
    (y * gd).sum().backward()
    assert torch.equal(mod.shaping_fn.net[2].weight.grad, want["shaping_fn.net.2.weight"])
    assert all(p.grad is None for k, p in mod.named_parameters() if k != "shaping_fn.net.2.weight")
    # hooks on an inner module: the flagged forward refuses, the plain one runs the modules one by one
    h = mod.mixer[0].register_forward_hook(lambda *a: None)
    with pytest.raises(RuntimeError, match="hooks"):
        mod(ed, cd)
    h.remove()
    # the lookup table has no backward
    fast = _nws().FastNEWT(plain)
    with pytest.raises(RuntimeError, match="lookup table has no backward"):
        fast.differentiable = True
    with pytest.raises(RuntimeError, match="lookup table has no backward"):
        fast.vjp(gd, ed, cd)
    assert fast.differentiable is False and fast(ed, cd).shape == want_y.shape
