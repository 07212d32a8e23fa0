"""-m gpu: the gradient exchange's kernels (csrc/grad_reduce.hip through both bindings) against their numpy restatement
(tests/grad_reduce_restatement.py), and parallel.GradientAverager with no process group on the packaged model.

The kernels' operations are IEEE - exact conversions to float64, additions in rank order, one division, one rounding to float32 -
so the bar is EQUAL BITS, np.array_equal on the uint32 views, not a tolerance.

Cases (tensor sizes, C = 1024 the kernels' chunk): 'edges' [1, 3, C - 1, C, C + 1]; 'tables' 65 tensors of 5 elements and one of
2 C + 1, past one 64-entry table; 'model' the 48 shapes of the packaged model and one loss element.  W in {1, 2, 3, 8}: 3 because its
division is not exact.  Values normal x 10^U(-6, 3); by hand a NaN, +Inf and -Inf (each in a column of its own: IEEE 754 leaves the
sign of the NaN that Inf - Inf generates open, and the host's differs from the GPU's), columns of +0 and -0 and denormals.  The
sources of a pack are views at an odd element offset of one flat buffer: 4-byte aligned only.

The bindings are both exercised in one pass; with NWS_BACKEND=ctypes the file passes through the ctypes binding alone."""
import copy
import functools
import importlib
import os
import re

import numpy as np
import pytest
import torch

import grad_reduce_restatement as gr
from gpu_util import build_model, dev

pytestmark = pytest.mark.gpu

BAD_ARG, UNSUPPORTED = -2, -1
WHICH = ("ctypes",) if os.environ.get("NWS_BACKEND") == "ctypes" else ("ops", "ctypes")
WORLDS = (1, 2, 3, 8)
PATTERN = -7.25


def _nws():
    import nws_amd as nws

    return nws


@functools.lru_cache(maxsize=None)
def _bindings():
    from nws_amd._cops import CtypesOps
    from nws_amd.engine import binding

    b = binding()
    return {"ctypes": b} if isinstance(b, CtypesOps) else {"ops": b, "ctypes": CtypesOps()}


@functools.lru_cache(maxsize=None)
def _model_shapes():
    return tuple(tuple(p.shape) for p in build_model(fast=False).parameters())


def _shapes(case):
    if case == "edges":
        return [(1,), (3,), (gr.C - 1,), (gr.C,), (gr.C + 1,)]
    if case == "tables":
        return [(5,)] * 65 + [(2 * gr.C + 1,)]
    shapes = list(_model_shapes()) + [(1,)]           # the 48 gradients and the loss
    assert len(shapes) == 49 and sum(int(np.prod(s)) for s in shapes) == 266946
    return shapes


@functools.lru_cache(maxsize=None)
def _rows(case, W):
    """(W, P) float32: what the W ranks pack - computed once, shared, never written"""
    P = sum(int(np.prod(s)) for s in _shapes(case))
    rng = np.random.default_rng(1000 * W + len(case))
    rows = (rng.standard_normal((W, P)) * 10.0 ** rng.uniform(-6, 3, (W, P))).astype(np.float32)
    last = W - 1
    rows[0, 0] = np.nan                                # propagates
    rows[last, 1] = np.inf
    rows[0, 2] = -np.inf
    rows[:, 3] = 0.0                                   # +0 everywhere but one -0: +0
    rows[0, 3] = -0.0
    rows[:, 4] = -0.0                                  # -0 everywhere: -0
    rows[:, 5] = 0.0                                   # one smallest denormal among zeros: the division rounds a denormal
    rows[last, 5] = np.float32(1e-45)
    rows[:, 6] = np.float32(3e-39)                     # denormals everywhere
    rows[:, 7] = np.float32(3.0e38)                    # the float64 sum passes float32's range, the mean is back inside it
    rows.setflags(write=False)
    return rows


def _views(row, shapes):
    """device views of one rank's values at an odd element offset of a flat buffer"""
    flat = torch.empty(row.size + 1, device="cuda")
    flat[1:] = dev(row.copy())
    views, off = [], 1
    for s in shapes:
        n = int(np.prod(s))
        views.append(flat[off:off + n].view(s))
        off += n
    assert views[0].data_ptr() % 8 == 4
    return views


def _bits(t):
    return gr.bits(t.cpu().numpy())


@pytest.mark.parametrize("W", WORLDS)
@pytest.mark.parametrize("case", ["edges", "tables", "model"])
@pytest.mark.parametrize("which", WHICH)
def test_pack_and_reduce_equal_the_restatement(which, case, W):
    b = _bindings()[which]
    shapes, rows_np = _shapes(case), _rows(case, W)
    P = rows_np.shape[1]
    stride = -(-P // 4) * 4 + 4                        # rows longer than what is packed: the tail stays as it was
    rows = torch.full((W, stride), PATTERN, device="cuda")
    for r in range(W):
        b.grad_pack(_views(rows_np[r], shapes), rows[r])
    got = rows.cpu().numpy()
    want = np.stack([gr.pack([rows_np[r]]) for r in range(W)])
    assert np.array_equal(gr.bits(got[:, :P]), gr.bits(want)) and np.all(got[:, P:] == PATTERN)
    out = torch.full((P + 3,), PATTERN, device="cuda")
    b.grad_reduce(rows, out[:P])
    mean = gr.reduce(rows_np)
    assert np.array_equal(_bits(out[:P]), gr.bits(mean)), np.flatnonzero(_bits(out[:P]) != gr.bits(mean))[:8]
    assert np.all(out[P:].cpu().numpy() == PATTERN)
    assert np.isnan(mean[0]) and mean[1] == np.inf and mean[2] == -np.inf and np.isfinite(mean[7])
    if W == 1:
        assert np.array_equal(_bits(out[:P]), gr.bits(rows_np[0]))                 # the row's own bits
    again = torch.full((P,), PATTERN, device="cuda")                                # two calls on equal inputs: equal bits
    b.grad_reduce(rows, again)
    assert np.array_equal(_bits(again), _bits(out[:P]))
    fewer = torch.full((P,), PATTERN, device="cuda")                                # out shorter than the stride: the first n columns
    b.grad_reduce(rows, fewer[:5])
    assert np.array_equal(_bits(fewer[:5]), gr.bits(mean[:5])) and np.all(fewer[5:].cpu().numpy() == PATTERN)


@pytest.mark.parametrize("which", WHICH)
def test_operators_refuse_what_adam_step_refuses(which):
    b = _bindings()[which]
    x, rows, out = torch.zeros(12, device="cuda"), torch.zeros(2, 12, device="cuda"), torch.zeros(12, device="cuda")
    for call in (lambda: b.grad_pack([x.cpu()], out), lambda: b.grad_pack([x], out.cpu()), lambda: b.grad_reduce(rows.cpu(), out),
                 lambda: b.grad_reduce(rows, out.cpu())):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for call in (lambda: b.grad_pack([x.double()], out), lambda: b.grad_pack([x], out.double()),
                 lambda: b.grad_reduce(rows.double(), out), lambda: b.grad_reduce(rows, out.double())):
        with pytest.raises(RuntimeError, match="expected Float"):
            call()
    for call in (lambda: b.grad_pack([x.view(3, 4).t()], out), lambda: b.grad_pack([x], torch.zeros(24, device="cuda")[::2]),
                 lambda: b.grad_reduce(torch.zeros(12, 2, device="cuda").t(), out), lambda: b.grad_reduce(rows, torch.zeros(24, device="cuda")[::2])):
        with pytest.raises(RuntimeError, match="contiguous"):
            call()
    for call in (lambda: b.grad_pack([], out), lambda: b.grad_pack([x, x], out), lambda: b.grad_pack([x[:0]], out),
                 lambda: b.grad_pack([x], out.view(3, 4)), lambda: b.grad_reduce(rows, torch.zeros(13, device="cuda")),
                 lambda: b.grad_reduce(rows.view(-1), out), lambda: b.grad_reduce(rows, out[:0])):
        with pytest.raises(RuntimeError):
            call()
    assert float(out.abs().sum()) == 0.0


def test_refusals_through_the_c_abi_leave_out_untouched():
    from nws_amd import _lib

    L = _lib.lib()
    W, shapes = 3, _shapes("edges")
    rows_np = _rows("edges", W)
    P = rows_np.shape[1]
    rows = dev(rows_np.copy())
    out = torch.full((P,), PATTERN, device="cuda")
    dst = torch.full((P,), PATTERN, device="cuda")
    views = _views(rows_np[0], shapes)
    recs = (_lib.NwsGradTensor * len(views))(*[_lib.NwsGradTensor(v.data_ptr(), v.numel()) for v in views])
    st = torch.cuda.current_stream().cuda_stream
    red = lambda world, n, stride, o: L.nws_grad_reduce(rows.data_ptr(), world, n, stride, o, st)
    assert red(0, P, P, out.data_ptr()) == BAD_ARG and red(W, 0, P, out.data_ptr()) == BAD_ARG
    assert red(W, P, P - 1, out.data_ptr()) == BAD_ARG and red(W, P, P, None) == BAD_ARG
    assert L.nws_grad_reduce(None, W, P, P, out.data_ptr(), st) == BAD_ARG
    assert red(W, P, P, rows.data_ptr() + 4 * P) == BAD_ARG                        # out is row 1
    assert red(1025, P, P, out.data_ptr()) == UNSUPPORTED
    assert L.nws_grad_pack(recs, len(views), dst.data_ptr(), P - 1, st) == BAD_ARG
    assert L.nws_grad_pack(recs, 0, dst.data_ptr(), P, st) == BAD_ARG and L.nws_grad_pack(recs, len(views), None, P, st) == BAD_ARG
    recs[2].n = 0
    assert L.nws_grad_pack(recs, len(views), dst.data_ptr(), P, st) == BAD_ARG
    recs[2].n = views[2].numel()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == PATTERN) and np.all(dst.cpu().numpy() == PATTERN)
    assert np.array_equal(_bits(rows), gr.bits(rows_np))
    # a valid call right after
    assert L.nws_grad_pack(recs, len(views), dst.data_ptr(), P, st) == 0 and red(W, P, P, out.data_ptr()) == 0
    assert np.array_equal(_bits(dst), gr.bits(rows_np[0])) and np.array_equal(_bits(out), gr.bits(gr.reduce(rows_np)))


@pytest.mark.parametrize("which", WHICH)
def test_gradient_averager_without_a_process_group(which):
    """world size 1 on the packaged model after one training_step + backward at (2, 16): the averaged gradient is the gradient, as
    views into one buffer, and nws.optim.Adam steps on the views as it does on the gradients themselves"""
    nws = _nws()
    par = importlib.import_module(nws.__name__ + ".parallel")
    g = torch.Generator().manual_seed(11)
    batch = {"f0": dev(180.0 + 400.0 * torch.rand(2, 1, 16, generator=g)), "control": dev(torch.randn(2, 2, 16, generator=g)),
             "audio": dev(0.1 * torch.randn(2, 128 * 16, generator=g))}
    model = build_model(fast=False)
    model.differentiable = True
    torch.cuda.manual_seed(0)
    loss = model.training_step(batch, 0)
    loss.backward()
    before = [p.grad.clone() for p in model.parameters()]
    twin = copy.deepcopy(model)
    for p, gp in zip(twin.parameters(), before):
        p.grad = gp.clone()
    av = par.GradientAverager(list(model.named_parameters()), kernels=_bindings()[which])
    assert (av.world, av.rank, av.P, av.stride, tuple(av.rows.shape)) == (1, 0, 266945, 266948, (1, 266948))
    back = av.average(loss.detach().reshape(1))
    assert torch.equal(back, loss.detach().reshape(1)) and back.data_ptr() == av.mean.data_ptr() + 4 * av.P
    off = 0
    for p, gp in zip(model.parameters(), before):
        assert torch.equal(p.grad, gp) and p.grad.shape == p.shape
        assert p.grad.data_ptr() == av.mean.data_ptr() + 4 * off                    # views into one buffer, in order
        off += p.numel()
    av.check_in_sync()
    opts = [nws.optim.Adam(m.parameters(), lr=1e-4, max_grad_norm=2.0) for m in (model, twin)]
    for opt in opts:
        opt.step()
    assert torch.equal(opts[0].last_grad_norm, opts[1].last_grad_norm)
    for (k, p), q, gp in zip(model.named_parameters(), twin.parameters(), before):
        assert torch.equal(p, q), k
        assert torch.equal(p.grad, gp), k                                          # the step does not rewrite the views
    opts[0].zero_grad(set_to_none=True)
    assert all(p.grad is None for p in model.parameters())
    # a missing gradient, a tensor of another dtype: refused by name before anything is packed
    names = [k for k, _ in model.named_parameters()]
    with pytest.raises(RuntimeError, match=re.escape(names[0]) + " has no gradient"):
        av.average(loss.detach().reshape(1))
    tensors = [p.detach() for p in model.parameters()]
    tensors[5] = tensors[5].double()
    with pytest.raises(RuntimeError, match=re.escape(names[5]) + ".*float64"):
        av.check_in_sync(tensors)
