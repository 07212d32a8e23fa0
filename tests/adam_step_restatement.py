"""Float64 numpy restatement of the optimiser step (csrc/adam_step.hip), every step named: the arithmetic of
torch.nn.utils.clip_grad_norm_(max_norm, 2.0) followed by torch.optim.Adam (weight_decay 0, no amsgrad, no maximize).

    total = sqrt(sum_k sum_i g_k[i]^2)                 float64 sums, rounded once to `norm_dtype`
    c     = min(max_norm / (total + 1e-6), 1)          in `norm_dtype`
    gc    = c g
    m'    = m + (1 - beta1)(gc - m)
    v'    = beta2 v + (1 - beta2) gc^2
    p'    = p - (lr / (1 - beta1^t)) m' / (sqrt(v') / sqrt(1 - beta2^t) + eps)

`norm_dtype` is float32 for what the kernel (and torch on float32 tensors) computes - the norm and the clip coefficient are float32
numbers there - and float64 for the comparison with torch in float64.  Also the shared cases, inputs and references of
tests/test_cpu_adam_step.py and tests/test_gpu_adam_step.py: three steps under StepLR(2, 0.5), the first and third clipped."""
import functools
import importlib

import numpy as np

C = 1024            # elements per workgroup and per partial (NWS_ADAM_CHUNK)
THREADS = 256       # threads that share the sum over the partials
TABLE = 64          # tensors per launch (NWS_ADAM_TABLE)
LR, BETAS, EPS, MAX_NORM = 1e-3, (0.9, 0.999), 1e-8, 2.0
STEPS = 3
LRS = (LR, LR, 0.5 * LR)                 # StepLR(step_size 2, gamma 0.5), stepped after every optimiser step
TOTALS = (4.0, 0.5, 3.0)                 # the gradients' norm at each step: clipped, not clipped, clipped
CASES = ("edges", "tables", "strided", "model")


def total_norm(grads, norm_dtype=np.float32):
    sq = 0.0
    for g in grads:
        g64 = np.asarray(g, dtype=np.float64).reshape(-1)
        sq += float(np.dot(g64, g64))
    return norm_dtype(np.sqrt(sq))


def clip_coefficient(total, max_norm, norm_dtype=np.float32):
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = norm_dtype(max_norm) / (norm_dtype(total) + norm_dtype(1e-6))
    return np.minimum(ratio, norm_dtype(1.0))           # a NaN stays a NaN


def adam_step(params, grads, exp_avgs, exp_avg_sqs, step, lr, beta1, beta2, eps, max_norm, norm_dtype=np.float32):
    """-> (params', exp_avgs', exp_avg_sqs', total) as float64 arrays (total in `norm_dtype`); nothing is modified"""
    total = total_norm(grads, norm_dtype)
    c = float(clip_coefficient(total, max_norm, norm_dtype))
    bias_correction1 = 1.0 - beta1 ** step
    bias_correction2 = 1.0 - beta2 ** step
    step_size = lr / bias_correction1
    out_p, out_m, out_v = [], [], []
    for p, g, m, v in zip(params, grads, exp_avgs, exp_avg_sqs):
        p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
        clipped = c * g
        m_new = m + (1.0 - beta1) * (clipped - m)
        v_new = beta2 * v + (1.0 - beta2) * clipped * clipped
        denom = np.sqrt(v_new) / np.sqrt(bias_correction2) + eps
        out_p.append(p - step_size * (m_new / denom))
        out_m.append(m_new)
        out_v.append(v_new)
    return out_p, out_m, out_v, total


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@functools.lru_cache(maxsize=None)
def model_shapes():
    """the 48 parameter shapes of the packaged model"""
    pkg = importlib.import_module("neural-waveshaping-synthesis_amd")
    pkg.ensure_default_config()
    shapes = tuple(tuple(p.shape) for p in pkg.NeuralWaveshaping().parameters())
    assert len(shapes) == 48 and sum(int(np.prod(s)) for s in shapes) == 266945
    return shapes


def shapes(case):
    if case == "edges":                  # the chunk's edges
        return ((1,), (3,), (C - 1,), (C,), (C + 1,))
    if case == "tables":                 # past one 64-entry table
        return ((5,),) * 65 + ((2 * C + 1,),)
    if case == "strided":                # more chunks than the partial sum has threads: its second trip
        return (((THREADS + 1) * C + 7,),)
    return model_shapes()


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(params, [grads of step 1, 2, 3]) as float32 arrays: parameters 1e-3 normal (at |p| ~ 1 the float32 rounding of p + dp alone
    hides the update), every tensor's gradient at a scale of its own, 10^U(-6, 1), the set rescaled to the step's total norm"""
    rng = np.random.default_rng(1900 + CASES.index(case))
    shp = shapes(case)
    params = [(1e-3 * rng.standard_normal(s)).astype(np.float32) for s in shp]
    steps = []
    for want in TOTALS:
        gs = [(10.0 ** rng.uniform(-6.0, 1.0)) * rng.standard_normal(s) for s in shp]
        scale = want / float(total_norm(gs, np.float64))
        steps.append([(scale * g).astype(np.float32) for g in gs])
    return params, steps


def trajectory(case, max_norm=MAX_NORM, norm_dtype=np.float32, start=None):
    """the restatement's [(params, exp_avgs, exp_avg_sqs, total) after step 1, 2, 3]; each step starts from `start` if given (a
    list of three (params, exp_avgs, exp_avg_sqs): the float32 state the code under test started that step from), else from the
    restatement's own previous step"""
    p, steps = inputs(case)
    m, v = [np.zeros(a.shape) for a in p], [np.zeros(a.shape) for a in p]
    out = []
    for t, (lr, grads) in enumerate(zip(LRS, steps), start=1):
        if start is not None:
            p, m, v = start[t - 1]
        p, m, v, total = adam_step(p, grads, m, v, t, lr, BETAS[0], BETAS[1], EPS, max_norm, norm_dtype)
        out.append((p, m, v, total))
    return out


def torch_trajectory(case, dtype, max_norm=MAX_NORM):
    """clip_grad_norm_ + torch.optim.Adam under StepLR(2, 0.5) on the CPU in `dtype`: [(state before the step as three lists of
    arrays, (params, exp_avgs, exp_avg_sqs, total) after it)] for steps 1, 2, 3"""
    import torch

    p0, steps = inputs(case)
    ps = [torch.nn.Parameter(torch.tensor(a, dtype=dtype)) for a in p0]
    opt = torch.optim.Adam(ps, lr=LR, betas=BETAS, eps=EPS)
    sched = torch.optim.lr_scheduler.StepLR(opt, 2, 0.5)
    arrays = lambda key: [opt.state[p][key].numpy().copy() if opt.state[p] else np.zeros(tuple(p.shape)) for p in ps]
    out = []
    for grads in steps:
        before = ([p.detach().numpy().copy() for p in ps], arrays("exp_avg"), arrays("exp_avg_sq"))
        for p, g in zip(ps, grads):
            p.grad = torch.tensor(g, dtype=dtype)
        total = torch.nn.utils.clip_grad_norm_(ps, max_norm, 2.0)
        opt.step()
        sched.step()
        out.append((before, ([p.detach().numpy().copy() for p in ps], arrays("exp_avg"), arrays("exp_avg_sq"), float(total))))
    return out
