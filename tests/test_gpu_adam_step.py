"""-m gpu: the optimiser step (csrc/adam_step.hip through both bindings, nws.optim.Adam) against the float64
restatement of its definition (tests/adam_step_restatement.py).

Cases (tensor sizes, C = 1024 the kernel's chunk): 'edges' [1, 3, C - 1, C, C + 1]; 'tables' 65 tensors of 5 elements and one of
2 C + 1, past one 64-entry table; 'strided' one tensor of 257 chunks + 7 elements, the second trip of the strided sum over the
partials; 'model' the 48 shapes of the packaged model.  Parameters 1e-3 normal, every tensor's gradient at its own scale
10^U(-6, 1), the set rescaled to a total norm of 4, 0.5 and 3 at steps 1, 2, 3: clipped (max_norm 2), not clipped, clipped; the
learning rate halves after step 2.  The states are views into one buffer at an odd element offset: 4-byte aligned only.

Bar, for dp = p' - p, m' and v' of every tensor at every step (relative L2 from the restatement started from the state the step
started from) and for total (relative error): at most 10 x the distance of torch's float32 CPU clip_grad_norm_ + Adam from the same
restatement on the same inputs (computed here, floored at 2^-24, one float32 rounding), and never beyond 1e-4 (FACTOR, CAP of the
other gradient tests).  The measured figures (kernel | torch | ratio per case) are in DESIGN.md 3.19.

The bindings are both exercised in one pass; with NWS_BACKEND=ctypes the file passes through the ctypes binding alone."""
import copy
import functools
import math
import os

import numpy as np
import pytest
import torch

import adam_step_restatement as ar
from gpu_util import dev, record

pytestmark = pytest.mark.gpu

FACTOR = 10.0
CAP = 1e-4
FLOOR = 2.0 ** -24
BAD_ARG = -2
HYPER = (ar.BETAS[0], ar.BETAS[1], ar.EPS)
WHICH = ("ctypes",) if os.environ.get("NWS_BACKEND") == "ctypes" else ("ops", "ctypes")


def _nws():
    import nws_amd as nws

    return nws


@functools.lru_cache(maxsize=None)
def _bindings():
    from nws_amd._cops import CtypesOps
    from nws_amd.engine import binding

    b = binding()
    return {"ctypes": b} if isinstance(b, CtypesOps) else {"ops": b, "ctypes": CtypesOps()}


def _binding(which):
    return _bindings()[which]


@functools.lru_cache(maxsize=None)
def _yardstick(case):
    """torch float32 on the CPU and the restatement started from torch's own state at every step"""
    tt = ar.torch_trajectory(case, torch.float32)
    return tt, ar.trajectory(case, start=[before for before, _ in tt])


def _state(case):
    """device tensors: parameters, and zero states as views at an odd element offset of one buffer"""
    p0, steps = ar.inputs(case)
    ps = [dev(a) for a in p0]
    n = sum(a.size for a in p0)
    flat = torch.zeros(2 * n + 1, device="cuda")
    ms, vs, off = [], [], 1
    for a in p0:
        ms.append(flat[off:off + a.size].view(a.shape))
        vs.append(flat[n + off:n + off + a.size].view(a.shape))
        off += a.size
    assert ms[0].data_ptr() % 8 == 4
    return ps, ms, vs, [[dev(g) for g in gs] for gs in steps]


def _host(ts):
    return [t.cpu().numpy().astype(np.float64) for t in ts]


def _three_steps(b, case, max_norm=ar.MAX_NORM):
    """-> [(start state, (params, exp_avgs, exp_avg_sqs, total) after the step)] as float64 arrays, and the device state"""
    ps, ms, vs, steps = _state(case)
    out = []
    for t, (lr, gs) in enumerate(zip(ar.LRS, steps), start=1):
        start = (_host(ps), _host(ms), _host(vs))
        total = b.adam_step(ps, gs, ms, vs, t, lr, *HYPER, max_norm)
        assert total.shape == () and total.dtype == torch.float32 and total.is_cuda
        out.append((start, (_host(ps), _host(ms), _host(vs), float(total))))
    return out, (ps, ms, vs, steps)


def _distances(run, ref):
    """per step: {quantity: [relative L2 per tensor]} and the total's relative error"""
    per_step = []
    for ((p0, _, _), (p, m, v, total)), (rp, rm, rv, rt) in zip(run, ref):
        d = {"dp": [ar.rel_l2(a - s, r - s) for a, r, s in zip(p, rp, p0)], "m": [ar.rel_l2(a, r) for a, r in zip(m, rm)],
             "v": [ar.rel_l2(a, r) for a, r in zip(v, rv)], "total": [abs(total - float(rt)) / float(rt)]}
        per_step.append(d)
    return per_step


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("case", ar.CASES)
def test_three_steps_against_the_restatement(case, which):
    b = _binding(which)
    run, _ = _three_steps(b, case)
    mine = _distances(run, ar.trajectory(case, start=[s for s, _ in run]))
    tt, tref = _yardstick(case)
    yard = _distances(tt, tref)
    totals = [r[1][3] for r in run]
    assert totals[0] > ar.MAX_NORM and totals[1] < ar.MAX_NORM and totals[2] > ar.MAX_NORM       # clipped, not clipped, clipped
    failures, summary = [], {}
    for q in ("dp", "m", "v", "total"):
        worst = (0.0, 0.0, 0.0)
        for t in range(ar.STEPS):
            for k, (dk, dt) in enumerate(zip(mine[t][q], yard[t][q])):
                ratio = dk / max(dt, FLOOR)
                worst = max(worst, (ratio, dk, dt))
                if not (dk <= FACTOR * max(dt, FLOOR) and dk <= CAP):
                    failures.append((q, t + 1, k, dk, dt))
        print(f"adam_step {case} [{which}] {q}: kernel {worst[1]:.2e} | torch float32 CPU {worst[2]:.2e} | ratio {worst[0]:.2f}")
        summary.update({q + "_kernel": worst[1], q + "_torch_f32": worst[2], q + "_ratio": worst[0]})
    record(f"adam_step/{case}_{which}", **summary)
    assert not failures, failures[:8]


@pytest.mark.parametrize("which", WHICH)
def test_exact_cases(which):
    b = _binding(which)
    case = "tables"
    run, (ps, ms, vs, steps) = _three_steps(b, case)
    again, (ps2, ms2, vs2, _) = _three_steps(b, case)
    for xs, ys in ((ps, ps2), (ms, ms2), (vs, vs2)):                       # equal inputs, equal bits
        assert all(torch.equal(x, y) for x, y in zip(xs, ys))
    assert [r[1][3] for r in run] == [r[1][3] for r in again]
    _, want_steps = ar.inputs(case)                                        # the gradients were read, not rewritten
    assert all(torch.equal(g.cpu(), torch.as_tensor(w)) for gs, ws in zip(steps, want_steps) for g, w in zip(gs, ws))
    # max_norm = inf: the bits of any max_norm above the total
    inf, _ = _three_steps(b, case, math.inf)
    big, _ = _three_steps(b, case, 1e30)
    for (_, (p, m, v, t)), (_, (p2, m2, v2, t2)) in zip(inf, big):
        assert t == t2 and all(np.array_equal(x, y) for xs, ys in ((p, p2), (m, m2), (v, v2)) for x, y in zip(xs, ys))
    assert any(not np.array_equal(x, y) for x, y in zip(inf[0][1][1], run[0][1][1]))          # and not the clipped ones
    # g = 0 with zero state: p keeps its bits, the states stay zero, total is 0
    ps, ms, vs, steps = _state(case)
    before = [p.clone() for p in ps]
    versions = [(p._version, m._version, v._version) for p, m, v in zip(ps, ms, vs)]
    total = b.adam_step(ps, [torch.zeros_like(p) for p in ps], ms, vs, 1, ar.LR, *HYPER, ar.MAX_NORM)
    assert float(total) == 0.0 and all(torch.equal(a, p) for a, p in zip(before, ps))
    assert all(not m.any() and not v.any() for m, v in zip(ms, vs))
    # the version counters rose: the caches of derived tables key on them
    assert all(p._version > a and m._version > c and v._version > d for (a, c, d), p, m, v in zip(versions, ps, ms, vs))
    # tensors absent from the call are untouched: every second tensor, and the total is theirs alone
    ps, ms, vs, steps = _state(case)
    before = ([p.clone() for p in ps], [m.clone() for m in ms], [v.clone() for v in vs])
    some = list(range(0, len(ps), 2))
    pick = lambda xs: [xs[k] for k in some]
    total = b.adam_step(pick(ps), pick(steps[0]), pick(ms), pick(vs), 1, ar.LR, *HYPER, ar.MAX_NORM)
    want = ar.total_norm([ar.inputs(case)[1][0][k] for k in some])
    assert abs(float(total) - float(want)) <= FACTOR * FLOOR * float(want)
    for k in range(len(ps)):
        same = [torch.equal(before[0][k], ps[k]), torch.equal(before[1][k], ms[k]), torch.equal(before[2][k], vs[k])]
        assert same == [k % 2 == 1] * 3, k


@pytest.mark.parametrize("which", WHICH)
def test_op_refuses(which):
    b = _binding(which)
    p, g, m, v = (torch.ones(4, 3, device="cuda") for _ in range(4))
    args = (1, ar.LR, *HYPER, ar.MAX_NORM)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        b.adam_step([p.cpu()], [g.cpu()], [m.cpu()], [v.cpu()], *args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        b.adam_step([p], [g], [m.cpu()], [v], *args)
    with pytest.raises(RuntimeError, match="(?i)float"):
        b.adam_step([p.double()], [g.double()], [m.double()], [v.double()], *args)
    with pytest.raises(RuntimeError, match="contiguous"):
        b.adam_step([p.t()], [g.t()], [m.t()], [v.t()], *args)
    with pytest.raises(RuntimeError, match="shape"):
        b.adam_step([p], [g.view(3, 4)], [m], [v], *args)
    with pytest.raises(RuntimeError, match="grads"):
        b.adam_step([p], [], [m], [v], *args)
    with pytest.raises(RuntimeError, match="no tensors"):
        b.adam_step([], [], [], [], *args)
    with pytest.raises(RuntimeError, match="step counts from 1"):
        b.adam_step([p], [g], [m], [v], 0, *args[1:])
    assert all(torch.equal(t, torch.ones_like(t)) for t in (p, g, m, v))


# ---- the optimiser class ----------------------------------------------------------------------------------------------------------------
def test_optimizer_steps_like_the_op_and_skips_parameters_without_a_gradient():
    nws = _nws()
    case = "edges"
    p0, steps = ar.inputs(case)
    leaves = [torch.nn.Parameter(dev(a)) for a in p0] + [torch.nn.Parameter(torch.ones(7, device="cuda"))]
    opt = nws.optim.Adam([{"params": leaves[:2]}, {"params": leaves[2:]}], lr=ar.LR, betas=ar.BETAS, eps=ar.EPS, max_grad_norm=ar.MAX_NORM)
    sched = torch.optim.lr_scheduler.StepLR(opt, 2, 0.5)
    ps, ms, vs, gsteps = _state(case)
    versions = [p._version for p in leaves]
    for t, (lr, gs) in enumerate(zip(ar.LRS, gsteps), start=1):
        for p, g in zip(leaves, gs):
            p.grad = g.clone()
        opt.step()
        sched.step()
        total = _bindings()[next(iter(_bindings()))].adam_step(ps, gs, ms, vs, t, lr, *HYPER, ar.MAX_NORM)
        assert torch.equal(opt.last_grad_norm, total) and opt.last_grad_norm.is_cuda               # over both groups together
        assert all(torch.equal(p.grad, g) for p, g in zip(leaves, gs))                             # .grad is not rewritten
    for k, p in enumerate(leaves[:-1]):
        s = opt.state[p]
        assert torch.equal(p.detach(), ps[k]) and torch.equal(s["exp_avg"], ms[k]) and torch.equal(s["exp_avg_sq"], vs[k])
        assert int(s["step"]) == 3 and p._version > versions[k]
    last = leaves[-1]                                                                              # never had a gradient
    assert torch.equal(last.detach(), torch.ones(7, device="cuda")) and last not in opt.state and last._version == versions[-1]
    # its state dict loads into torch.optim.Adam, which continues on the GPU within float32 of our next step
    sd = copy.deepcopy(opt.state_dict())                      # state_dict() hands out the optimiser's own tensors
    assert set(sd["state"]) == {0, 1, 2, 3, 4}
    twins = [torch.nn.Parameter(p.detach().clone()) for p in leaves]
    theirs = torch.optim.Adam([{"params": twins[:2]}, {"params": twins[2:]}], lr=ar.LR)
    theirs.load_state_dict(sd)
    for p, q, g in zip(leaves, twins, gsteps[1]):
        p.grad, q.grad = g.clone(), g.clone()
    before = [p.detach().clone() for p in leaves]
    opt.step()
    theirs.step()                                                                                  # total 0.5 < 2: no clipping needed
    for p, q, s in zip(leaves[:-1], twins, before):
        assert ar.rel_l2((p.detach() - s).cpu().numpy(), (q.detach() - s).cpu().numpy()) <= CAP


# ---- refusals: decided on the host, before any launch ------------------------------------------------------------------------------------
def _raw(tensors, step=1, null_total=False, ws_short=False, ws_null=False, n=None, null_field=None, zero_n=False):
    """nws_adam_step through ctypes on NaN-filled tensors: (return code, the tensors, total, workspace)"""
    from nws_amd import _lib

    L = _lib.lib()
    recs = (_lib.NwsAdamTensor * len(tensors))()
    for k, (p, g, m, v) in enumerate(tensors):
        f = dict(param=p.data_ptr(), grad=g.data_ptr(), exp_avg=m.data_ptr(), exp_avg_sq=v.data_ptr())
        if null_field is not None and k == 1:
            f[null_field] = None
        recs[k] = _lib.NwsAdamTensor(f["param"], f["grad"], f["exp_avg"], f["exp_avg_sq"], 0 if zero_n and k == 1 else p.numel())
    nbytes = L.nws_adam_workspace_bytes(recs, len(tensors)) or 8 * len(tensors)
    ws = torch.full((nbytes,), 0x7f, dtype=torch.uint8, device="cuda")
    total = torch.full((), float("nan"), device="cuda")
    rc = L.nws_adam_step(recs, len(tensors) if n is None else n, step, ar.LR, *HYPER, ar.MAX_NORM, None if null_total else total.data_ptr(),
                         None if ws_null else ws.data_ptr(), nbytes - 8 if ws_short else nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, total, ws


def test_refusals_return_before_any_launch():
    sizes = (5, ar.C + 1, 3)
    make = lambda fill: [tuple(torch.full((n,), fill, device="cuda") for _ in range(4)) for n in sizes]
    for kw in (dict(step=0), dict(null_total=True), dict(ws_short=True), dict(ws_null=True), dict(n=0), dict(null_field="param"),
               dict(null_field="grad"), dict(null_field="exp_avg"), dict(null_field="exp_avg_sq"), dict(zero_n=True)):
        tensors = make(float("nan"))
        rc, total, ws = _raw(tensors, **kw)
        assert rc == BAD_ARG, (kw, rc)
        assert all(torch.isnan(t).all() for row in tensors for t in row) and bool(torch.isnan(total)), kw      # untouched
        assert bool((ws == 0x7f).all()), kw
    # and a valid call right after gives the op's bits
    g = torch.Generator().manual_seed(2)
    rows = [tuple(dev(a) for a in (1e-3 * torch.randn(n, generator=g), torch.randn(n, generator=g), torch.zeros(n), torch.zeros(n)))
            for n in sizes]
    twin = [tuple(t.clone() for t in row) for row in rows]
    rc, total, _ = _raw(rows)
    assert rc == 0
    cols = list(zip(*twin))
    want = _bindings()[next(iter(_bindings()))].adam_step(list(cols[0]), list(cols[1]), list(cols[2]), list(cols[3]), 1, ar.LR, *HYPER,
                                                           ar.MAX_NORM)
    assert torch.equal(total, want) and all(torch.equal(a, b) for ra, rb in zip(rows, twin) for a, b in zip(ra, rb))
