"""-m gpu: the kernel variants of the runtime-size path (csrc/generic.hip, csrc/stages.hip) that the launch code picks by size
and the sweep of test_gpu_generic.py never reaches - tiles per wave, the second M-tile, the four-channel epilogue, the
thread-per-sample buckets, the wide-phase branch, the grid-stride loops, every GRU bucket and its edges, MLP widths across
K-chunks and M-tiles.  End-to-end cases (tests/generic_variants.py) run NeuralWaveshaping.forward against the oracle on the
same state dict and draws, with a silent reverb, and first assert through nws_debug_generic_exciter_plan that they launch the
variant they are named for; stage cases run the ops against the float64 restatements of tests/generic_restatement.py."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import generic_variants as gv
from generic_restatement import gru_float64, td_mlp_float64
from gpu_util import dev, maxabs, record

pytestmark = pytest.mark.gpu

UNSUPPORTED = -1          # NWS_ERR_UNSUPPORTED (include/nws_hip.h)


def _binding():
    return importlib.import_module("neural-waveshaping-synthesis_amd.engine").binding()


# ---- end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(gv.CASES))
def test_variant_end_to_end(name):
    """Bars: the random sweep's whole-signal bar (RMS error <= 1e-4 and <= 1e-5 x max(RMS(ref), 1e-3)) and the same 1e-5 x scale
    per block of 512 samples of every row (the largest span one workgroup writes): an error confined to one 32-sample tile shows
    from a relative size of 4e-5 (tests/test_cpu_generic_variants.py measures what each modelled defect does to both)."""
    c = gv.CASES[name]
    B, T = c["B"], c["T"]
    with gv.configured(c) as nws:
        m, w = gv.build_model(nws, name)
        m = m.cuda()
        assert not m._engine.specialised()
        f0, control, pu, nz = gv.inputs(name)
        for mode in c["modes"]:
            fast = mode == "fast"
            if fast:
                m.newt = nws.FastNEWT(m.newt, **gv.TABLE)
            p = gv.exciter_plan(m._engine.generic.model_desc().struct, B, T)
            gv.assert_plan(name, mode, p)
            ref = gv.make_oracle(w, c, fast)(f0, control, pu, nz).numpy()
            with torch.no_grad():
                y = m(dev(f0), dev(control), phase_u=dev(pu), noise=dev(nz)).cpu().numpy()
            e, worst, scale = gv.errors(y, ref)
            extra = {}
            if name == "wide":
                phase_end = 2 * np.pi * float(np.repeat(f0[0, 0].astype(np.float64), c["hop"]).sum()) / gv.SR
                assert phase_end * 33 > 6.0e6 * 1.1, phase_end              # the wide branch really is taken (16 K16 + 1 = 33)
                extra = dict(max_abs_err=maxabs(y, ref), phase_end=phase_end)
            print(f"{name} {mode}: rms_err {e:.3e} worst_block {worst:.3e} bar {gv.REL_BAR * scale:.3e} plan {p}")
            record(f"generic_variant_{name}_{mode}", rms_err=e, worst_block_rms_err=worst, out_rms=scale, bar=gv.REL_BAR * scale,
                   tpw=p["tpw"], lds=p["lds"], **extra)
            assert np.isfinite(y).all()
            assert e <= gv.ABS_BAR and e <= gv.REL_BAR * scale, (name, mode, e, scale)
            assert worst <= gv.REL_BAR * scale, (name, mode, worst, scale)
            if name == "wide":
                assert extra["max_abs_err"] <= 2e-5, extra               # test_exciter_wide_phase_path's bar for the fused kernel


def test_shaper_apply_grid_stride_row():
    """nws_g_shaper_apply caps its grid at 4096 workgroups of 128 samples: a row of 524 288 + 133 samples sends the first two
    workgroups round their loop a second time (the second with 5 live samples).  Width 16 through the LDS-column sin-MLP
    against the oracle at the stand-alone shaper's bar (2e-5, test_gpu_generic.py); the table lookup bit for bit on the
    module's own table."""
    c = gv.CASES["film16_long"]
    N = 4096 * 128 + 133
    with gv.configured(c) as nws:
        m, w = gv.build_model(nws, "film16_long")
        m = m.cuda()
        x = torch.randn(1, c["S"], N, generator=torch.Generator().manual_seed(16))
        with torch.no_grad():
            ye = m.newt.shaping_fn(x.cuda()).cpu().numpy()
        e = maxabs(ye, gv.make_oracle(w, c, False).exact_shaper(x).numpy())
        m.newt = nws.FastNEWT(m.newt, **gv.TABLE)
        with torch.no_grad():
            yl = m.newt.shaping_fn(x.cuda()).cpu().numpy()
        o = gv.make_oracle(w, c, True)
        o._table = m.newt.lookup_table.detach().cpu()
        record("generic_variant_shaper_apply_long", exact_max_abs_err=e, tail_max_abs_err=maxabs(ye[..., 4096 * 128:], gv.make_oracle(w, c, False).exact_shaper(x[..., 4096 * 128:]).numpy()))
        assert e <= 2e-5, e
        assert np.array_equal(yl, o.lut_shaper(x).numpy())


@pytest.mark.parametrize("control_size", [1, 3])
def test_front_end_refuses_a_control_size_other_than_two(control_size):
    """nws_forward_generic takes any control_size; the Python front end refuses every one but 2, on purpose: the reference's
    get_embedding feeds control[:, 0:2] to the GRU whatever ControlModule.control_size says, so its own forward fails for any
    other size and there is nothing to be a drop-in for.  (C_in = 1, 3, 5, 44 ... run through the recurrence itself below.)"""
    c = gv.CASES["control_extra"]
    with gv.configured(c) as nws:
        nws.gin.parse_config(f"ControlModule.control_size = {control_size}")
        m = nws.NeuralWaveshaping().eval().cuda()
        f0, control, pu, nz = gv.inputs("control_extra")
        with pytest.raises(RuntimeError, match="control_size"):
            m(dev(f0), dev(control), phase_u=dev(pu), noise=dev(nz))


# ---- stages: the recurrence ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden,c_in", sorted(k for k in gv.GRU_PLANS if k != (128, 2)))
def test_g_gru_sizes_against_float64(hidden, c_in):
    """B = 3, T in {1, 2, 37}; each T plain and with C_total = C_in + 2 channels and a non-zero h0 (hT checked).  Bar: the
    project's own for the default recurrence - max-abs against float64 <= max(5e-6, 3 x the error of torch.nn.GRU in fp32 on the
    CPU against the same float64).  (16, 70) is the size this test found wrong: more input channels than the register kernel's 64
    threads stage per frame - 1.97 before the chooser sent it to g_gru_kernel, 3e-7 after."""
    p = gv.gru_plan(hidden, c_in)
    assert (p["kernel"], p["kq"], p["threads"]) == gv.GRU_PLANS[(hidden, c_in)], p
    torch.manual_seed(1000 * hidden + c_in)
    gru = torch.nn.GRU(c_in, hidden, batch_first=True)
    names = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
    w = [getattr(gru, n).detach() for n in names]
    wd = [t.cuda().contiguous() for t in w]
    B, worst = 3, {}
    for T in (1, 2, 37):
        for extra, with_h0 in ((0, False), (2, True)):
            control = torch.randn(B, c_in + extra, T)
            h0 = 0.5 * torch.randn(B, hidden) if with_h0 else None
            ref, ref_hT = gru_float64(*[t.numpy() for t in w], control.numpy(), None if h0 is None else h0.numpy())
            with torch.no_grad():
                t32, t32_hT = gru(control[:, :c_in].transpose(1, 2).contiguous(), None if h0 is None else h0[None])
            out, hT = _binding().g_gru(*wd, control.cuda().contiguous(), None if h0 is None else h0.cuda())
            torch.cuda.synchronize()
            assert out.shape == (B, T, hidden) and hT.shape == (B, hidden)
            e, e_t = maxabs(out.cpu().numpy(), ref), maxabs(t32.numpy(), ref)
            eh, eh_t = maxabs(hT.cpu().numpy(), ref_hT), maxabs(t32_hT[0].numpy(), ref_hT)
            worst[f"T{T}_{'h0_extra' if with_h0 else 'plain'}"] = f"{e:.2e}/{e_t:.2e} hT {eh:.2e}/{eh_t:.2e}"
            assert torch.isfinite(out).all()
            assert e <= max(5e-6, 3.0 * e_t), (hidden, c_in, T, with_h0, e, e_t)
            assert eh <= max(5e-6, 3.0 * eh_t), (hidden, c_in, T, with_h0, eh, eh_t)
    print(hidden, c_in, worst)
    record(f"generic_variant_gru_h{hidden}_c{c_in}", kernel=p["kernel"], kq=p["kq"], **worst)      # kernel error / torch-fp32 error


# ---- stages: TimeDistributedMLP -----------------------------------------------------------------------------------------------
MLP_SIZES = [(33, 47, 40, 3), (40, 40, 33, 4), (100, 64, 129, 4), (130, 200, 70, 2), (96, 96, 96, 1), (24, 24, 24, 8), (600, 600, 5, 2)]


def _torch_mlp(x, ws, bs, gs, ls):
    """the same net evaluated by torch in fp32 on the CPU: the yard-stick for what fp32 can do"""
    F = torch.nn.functional
    for i in range(len(ws)):
        x = F.conv1d(x, ws[i][:, :, None], bs[i])
        if i < len(ws) - 1:
            x = F.leaky_relu(F.layer_norm(x.transpose(1, 2), (x.shape[1],), gs[i], ls[i]).transpose(1, 2))
    return x


def _offset_view(t):
    """the same values in a contiguous view that starts 4 bytes into its storage (16-byte alignment lost)"""
    buf = torch.empty(t.numel() + 1, device="cuda")
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("sizes", MLP_SIZES, ids=lambda s: "x".join(map(str, s)))
def test_td_mlp_sizes_against_float64(sizes):
    """B = 2, T in {1, 31, 32, 33, 65}; once more (T = 33) with every weight tensor 4 bytes off 16-byte alignment, which must take
    the scalar weight loads and give the same bits.  Bar: max-abs against float64 <= max(floor, 3 x torch-fp32's error) x max(1,
    max |ref|), floor = the class's existing bar: 1e-5 for one layer, 5e-5 with LayerNorms."""
    in_size, hidden, out_size, depth = sizes
    ws, bs, gs, ls = gv.random_mlp(*sizes, seed=sum(sizes))
    dw, db, dg, dl = ([t.cuda() for t in lst] for lst in (ws, bs, gs, ls))
    floor = 1e-5 if depth == 1 else 5e-5
    g = torch.Generator().manual_seed(depth)
    measured = {}
    for T in (1, 31, 32, 33, 65):
        x = torch.randn(2, in_size, T, generator=g)
        ref = td_mlp_float64(x.numpy(), *[[t.numpy() for t in lst] for lst in (ws, bs, gs, ls)])
        e_t = maxabs(_torch_mlp(x, ws, bs, gs, ls).numpy(), ref)
        y = _binding().td_mlp(x.cuda(), dw, db, dg, dl, 1e-5, 0.01)
        torch.cuda.synchronize()
        assert y.shape == (2, out_size, T) and torch.isfinite(y).all()
        e = maxabs(y.cpu().numpy(), ref)
        measured[f"T{T}"] = f"{e:.2e}/{e_t:.2e}"
        assert e <= max(floor, 3.0 * e_t) * max(1.0, float(np.abs(ref).max())), (sizes, T, e, e_t)
        if T == 33:
            y2 = _binding().td_mlp(x.cuda(), [_offset_view(t) for t in dw], db, dg, dl, 1e-5, 0.01)
            torch.cuda.synchronize()
            assert torch.equal(y2, y), (sizes, maxabs(y2.cpu().numpy(), y.cpu().numpy()))
    print(sizes, measured)
    record("generic_variant_td_mlp_" + "x".join(map(str, sizes)), **measured)                        # kernel error / torch-fp32 error


def _raw_td_mlp(x, ws, bs, gs, ls, in_size, hidden, out_size, depth):
    """nws_td_mlp through ctypes: the return code itself"""
    _lib = importlib.import_module("neural-waveshaping-synthesis_amd._lib")

    def arr(ts):
        return (C.c_void_p * 16)(*[t.data_ptr() for t in ts])

    B, _, T = x.shape
    y = torch.full((B, out_size, T), float("nan"), device="cuda")
    rc = _lib.lib().nws_td_mlp(x.data_ptr(), B, in_size, hidden, out_size, depth, T, arr(ws), arr(bs), arr(gs), arr(ls), 1e-5, 0.01,
                               y.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, y


@pytest.mark.parametrize("sizes", [(24, 24, 24, 9), (700, 700, 5, 2)], ids=["depth9", "width700"])
def test_td_mlp_refusals_return_before_any_launch(sizes):
    """depth 9 (the kernel's argument block holds 8 layers) and a width whose two activation planes exceed 160 KB of LDS (612 is
    the widest that fits): NWS_ERR_UNSUPPORTED, the output untouched, and a valid call right after gives the right answer."""
    in_size, hidden, out_size, depth = sizes
    ws, bs, gs, ls = ([t.cuda() for t in lst] for lst in gv.random_mlp(*sizes, seed=9))
    x = torch.randn(2, in_size, 5, generator=torch.Generator().manual_seed(9)).cuda()
    rc, y = _raw_td_mlp(x, ws, bs, gs, ls, *sizes)
    assert rc == UNSUPPORTED, rc
    assert torch.isnan(y).all()
    ok = (24, 24, 24, 3)
    ws, bs, gs, ls = gv.random_mlp(*ok, seed=3)
    x = torch.randn(2, 24, 5, generator=torch.Generator().manual_seed(3))
    rc, y = _raw_td_mlp(x.cuda(), *[[t.cuda() for t in lst] for lst in (ws, bs, gs, ls)], *ok)
    assert rc == 0, rc
    ref = td_mlp_float64(x.numpy(), *[[t.numpy() for t in lst] for lst in (ws, bs, gs, ls)])
    assert maxabs(y.cpu().numpy(), ref) <= 5e-5 * max(1.0, float(np.abs(ref).max()))
