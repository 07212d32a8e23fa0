"""No GPU: the gradient exchange of data-parallel training (csrc/grad_reduce.hip, parallel.GradientAverager, scripts/train.py --gpus;
DESIGN.md 3.22): the restatement against torch.mean in float64, the C ABI's refusals - all decided before a launch, so asked for
without a device - the sharding rule of the loop as a pure function, and GradientAverager over gloo at world size 2 on CPU
tensors with the restatement in the kernels' place."""
import datetime
import importlib
import importlib.util
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import grad_reduce_restatement as gr
from conftest import ROOT

PKG = "neural-waveshaping-synthesis_amd"
_lib = importlib.import_module(PKG + "._lib")
par = importlib.import_module(PKG + ".parallel")
ds = importlib.import_module(PKG + ".dataset")
BAD_ARG, UNSUPPORTED = -2, -1


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 2, 3, 8])
def test_restatement_is_the_mean_in_float64(W):
    rng = np.random.default_rng(W)
    rows = (rng.standard_normal((W, 1001)) * 10.0 ** rng.uniform(-6, 3, (W, 1001))).astype(np.float32)
    got = gr.reduce(rows)
    want = torch.mean(torch.from_numpy(rows).double(), dim=0).numpy()
    assert got.dtype == np.float32 and got.shape == (1001,)
    # the restatement's one rounding to float32 (half an ulp: 2^-24 relative) on top of 1e-12 of the largest addend between two
    # float64 summation orders
    assert np.all(np.abs(got.astype(np.float64) - want) <= 2.0 ** -24 * np.abs(want) + 1e-12 * np.abs(rows).max(axis=0))
    assert np.array_equal(gr.bits(gr.reduce(rows, 7)), gr.bits(got[:7]))
    if W == 1:
        assert np.array_equal(gr.bits(got), gr.bits(rows[0]))
    parts = [rows[0, :5].reshape(5), rows[0, 5:11].reshape(2, 3), rows[0, 11:12]]
    assert np.array_equal(gr.bits(gr.pack(parts)), gr.bits(rows[0, :12]))


def test_restatement_constants_are_the_kernels():
    assert (gr.C, gr.TABLE, gr.MAX_WORLD) == (_lib.ADAM_CHUNK, _lib.ADAM_TABLE, _lib.GRAD_MAX_WORLD)
    header = open(os.path.join(ROOT, "include", "nws_hip.h")).read()
    assert f"#define NWS_GRAD_MAX_WORLD {gr.MAX_WORLD}\n" in header and "#define NWS_ABI_VERSION 6" in header
    spec = importlib.util.spec_from_file_location("nws_build", os.path.join(ROOT, PKG, "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert "grad_reduce.hip" in build.SOURCES and "-fno-slp-vectorize" in build.EXTRA_FLAGS["grad_reduce.hip"]
    assert "-ffp-contract=off" in build.FLAGS and not any("fast-math" in f for f in build.FLAGS)
    source = open(os.path.join(ROOT, PKG, "csrc", "grad_reduce.hip")).read()
    assert "atomic" not in source.replace("no atomics", "")


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def _records(ns, null=None):
    recs = (_lib.NwsGradTensor * max(1, len(ns)))()
    for k, n in enumerate(ns):
        recs[k] = _lib.NwsGradTensor(None if null == k else 0x1000 * (k + 1), n)
    return recs


def test_bad_arguments_return_codes_without_touching_the_gpu():
    """every refusal is decided on the host, before the first launch: the pointers here are never dereferenced"""
    L = _lib.lib()
    pack = L.nws_grad_pack
    ok = _records([5, gr.C + 1])
    assert pack(ok, 0, 0x9000, 2000, None) == BAD_ARG and pack(ok, -1, 0x9000, 2000, None) == BAD_ARG
    assert pack(None, 2, 0x9000, 2000, None) == BAD_ARG and pack(ok, 2, None, 2000, None) == BAD_ARG
    assert pack(_records([5, gr.C + 1], null=1), 2, 0x9000, 2000, None) == BAD_ARG
    assert pack(_records([5, 0]), 2, 0x9000, 2000, None) == BAD_ARG
    assert pack(ok, 2, 0x9000, gr.C + 5, None) == BAD_ARG and pack(ok, 2, 0x9000, 0, None) == BAD_ARG      # dst_elems < sum n
    assert pack(_records([(1 << 40) + 1]), 1, 0x9000, 1 << 41, None) == UNSUPPORTED
    red = L.nws_grad_reduce
    rows, out, n, stride = 0x100000, 0x900000, 1000, 1004
    assert red(None, 2, n, stride, out, None) == BAD_ARG and red(rows, 2, n, stride, None, None) == BAD_ARG
    assert red(rows, 0, n, stride, out, None) == BAD_ARG and red(rows, -1, n, stride, out, None) == BAD_ARG
    assert red(rows, 2, 0, stride, out, None) == BAD_ARG
    assert red(rows, 2, n, n - 1, out, None) == BAD_ARG                                                     # row_stride < n
    for inside in (rows, rows + 4, rows + 4 * stride, rows + 4 * (2 * stride - 1)):                          # out inside the rows
        assert red(rows, 2, n, stride, inside, None) == BAD_ARG, hex(inside)
    assert red(rows, 2, n, stride, rows - 4, None) == BAD_ARG                                               # out reaches into them
    assert red(rows, 1025, n, stride, out, None) == UNSUPPORTED
    for name in ("nws_grad_pack", "nws_grad_reduce"):
        assert name in _lib.EXPORTED_SYMBOLS
    assert L.nws_abi_version() == 6


def test_operators_refuse_cpu_tensors():
    """no CPU fallback: the ctypes twin refuses before it loads anything; the op layer's text is the same check_dev"""
    cops = importlib.import_module(PKG + "._cops").CtypesOps()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cops.grad_pack([torch.zeros(3)], torch.zeros(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cops.grad_reduce(torch.zeros(2, 4), torch.zeros(4))


# ---- the sharding rule --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("W", [1, 2, 3, 8])
def test_sharding_rule(W, b):
    for count in range(1, 14):
        names = [f"i{k}" for k in range(count)]
        frames = {n: (16 if k % 3 else 24) for k, n in enumerate(names)}           # two frame lengths mixed
        order = [names[i] for i in np.random.RandomState(count).permutation(count)]
        groups = ds.group_names(order, frames, W * b)
        assert sorted(n for g in groups for n in g) == sorted(names)
        assert all(len({frames[n] for n in g}) == 1 and 1 <= len(g) <= W * b for g in groups)
        per_rank = [ds.rank_batches(groups, W, r) for r in range(W)]
        kept = [g for g in groups if len(g) >= W]
        assert all(left == len(groups) - len(kept) for _, left in per_rank)         # dropped exactly when n < W
        assert len({len(mine) for mine, _ in per_rank}) == 1                        # every rank: the same number of steps
        for k, g in enumerate(kept):
            shards = [per_rank[r][0][k] for r in range(W)]
            assert all(len(s) >= 1 for s in shards)
            assert [n for s in shards for n in s] == g                              # every item on exactly one rank, in order
            assert [len(s) for s in shards] == [hi - lo for lo, hi in (par.shard_bounds(len(g), W, r) for r in range(W))]
        if W == 1:
            assert per_rank[0] == (groups, 0) and groups == ds.group_names(order, frames, b)      # today's batches


def test_groups_are_the_batches_of_the_dataset(tmp_path):
    root = tmp_path / "data"
    os.makedirs(root / "train" / "control")
    np.save(root / "data_mean.npy", np.zeros((2, 1)))
    np.save(root / "data_std.npy", np.ones((2, 1)))
    for k, name in enumerate("abcde"):
        np.save(root / "train" / "control" / f"control_{name}.npy", np.full((2, 16 if k % 2 else 24), float(k), dtype=np.float32))
    data = ds.ControlDataset(str(root), "train")
    order = ["d", "a", "e", "b", "c"]
    assert data.groups(order, 2) == [["d", "b"], ["a", "e"], ["c"]]
    got = list(data.batches(order, 2))
    assert [bt["names"] for bt in got] == data.groups(order, 2) and got[1]["control"].shape == (2, 2, 24)
    assert np.array_equal(data.collate(["a", "e"])["control"], got[1]["control"])


# ---- GradientAverager over gloo -----------------------------------------------------------------------------------------------------
SHAPES = {"a": (3, 2), "b": (5,), "c": (1,)}


def _grads(rank, step):
    g = torch.Generator().manual_seed(100 * step + rank)
    return {k: torch.randn(s, generator=g) * 10.0 ** float(torch.randint(-5, 3, (1,), generator=g)) for k, s in SHAPES.items()}


def _loss(rank, step):
    return torch.tensor([0.3 + rank + 0.1 * step], dtype=torch.float32)


def _worker(rank, world, port, tmp):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    torch.set_num_threads(1)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    try:
        g = torch.Generator().manual_seed(7)                # every rank: the same parameters
        params = {k: torch.nn.Parameter(torch.randn(s, generator=g)) for k, s in SHAPES.items()}
        av = par.GradientAverager(list(params.items()), extra=1, kernels=gr.kernels())       # check_in_sync passes
        out = {"stride": np.array([av.stride, av.P, av.world, av.rank])}

        def step(s):
            for k, p in params.items():
                p.grad = _grads(rank, s)[k]
            mean_loss = av.average(_loss(rank, s))
            lo, hi = av.mean.data_ptr(), av.mean.data_ptr() + 4 * av.stride
            assert all(lo <= p.grad.data_ptr() < hi and p.grad.shape == p.shape for p in params.values())
            out[f"loss{s}"] = mean_loss.clone().numpy()
            out[f"grad{s}"] = np.concatenate([p.grad.numpy().reshape(-1) for p in params.values()])

        step(0)
        av.check_in_sync()
        if rank == 1:
            with torch.no_grad():
                params["b"][3] += 1e-3
        try:
            av.check_in_sync()
            out["desync"] = np.array("no error")
        except RuntimeError as e:
            out["desync"] = np.array(str(e))
        if rank == 1:
            with torch.no_grad():
                params["b"].copy_(torch.load(os.path.join(tmp, "b.pt")))
        av.check_in_sync()
        # a missing gradient raises before any collective: rank 1 does not call average() here and is not left waiting, and the
        # next exchange pairs step 1 with step 1
        if rank == 0:
            for k, p in params.items():
                p.grad = None if k == "c" else _grads(rank, 1)[k]
            try:
                av.average(_loss(rank, 1))
                out["none"] = np.array("no error")
            except RuntimeError as e:
                out["none"] = np.array(str(e))
        step(1)
        np.savez(os.path.join(tmp, f"rank{rank}.npz"), **out)
    finally:
        dist.destroy_process_group()


def test_gradient_averager_two_ranks_on_gloo(tmp_path):
    g = torch.Generator().manual_seed(7)
    start = {k: torch.randn(s, generator=g) for k, s in SHAPES.items()}
    torch.save(start["b"], tmp_path / "b.pt")
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    got = [dict(np.load(tmp_path / f"rank{r}.npz")) for r in range(2)]
    P = sum(int(np.prod(s)) for s in SHAPES.values())
    for r in range(2):
        assert P == 12 and got[r]["stride"].tolist() == [16, P, 2, r]               # 12 + 1 rounded up to a multiple of 4
    for s in (0, 1):
        rows = np.stack([np.concatenate([gr.pack([_grads(r, s)[k].numpy() for k in SHAPES]), _loss(r, s).numpy()]) for r in range(2)])
        want = gr.reduce(rows)
        for r in range(2):
            assert np.array_equal(gr.bits(got[r][f"grad{s}"]), gr.bits(want[:P])), (s, r)
            assert np.array_equal(gr.bits(got[r][f"loss{s}"]), gr.bits(want[P:P + 1]))
        mean_loss = (np.float64(_loss(0, s).numpy()[0]) + np.float64(_loss(1, s).numpy()[0])) / 2.0
        assert got[0][f"loss{s}"][0] == np.float32(mean_loss)                       # the extra element: the mean of the losses
    for r in range(2):                                                              # both ranks see the same rows: both raise
        msg = str(got[r]["desync"])
        assert "out of sync" in msg and "first in b (element 3)" in msg and "1 elements differ" in msg, msg
    msg = str(got[0]["none"])
    assert "c has no gradient" in msg, msg
    assert "none" not in got[1]
