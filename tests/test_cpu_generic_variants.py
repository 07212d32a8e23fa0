"""No GPU: what test_gpu_generic_variants.py rests on.  The float64 restatements of the GRU and of TimeDistributedMLP equal
torch in float64; every end-to-end case selects the kernel variant it is named for (the plan queries of
include/nws_hip_debug.h are host arithmetic); and the block-wise bar of those cases trips on a defect confined to one tile,
one M-tile, one output channel or one partial tile, on the oracle's own signal at the very shapes the GPU cases use."""
import numpy as np
import pytest
import torch

import generic_variants as gv
from generic_restatement import gru_float64, td_mlp_float64


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("H,C_in,C_total,B,T", [(5, 3, 3, 2, 9), (33, 1, 4, 3, 17), (128, 2, 2, 1, 40)])
def test_gru_restatement_equals_torch_float64(H, C_in, C_total, B, T):
    torch.manual_seed(H)
    gru = torch.nn.GRU(C_in, H, batch_first=True).double()
    control = torch.randn(B, C_total, T, dtype=torch.float64)
    h0 = 0.5 * torch.randn(B, H, dtype=torch.float64)
    w = [getattr(gru, n).detach().numpy() for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]
    for start in (None, h0):
        with torch.no_grad():
            want, hT = gru(control[:, :C_in].transpose(1, 2), None if start is None else start[None])
        out, last = gru_float64(*w, control.numpy(), None if start is None else start.numpy())
        assert _rel(out, want.numpy()) <= 1e-12 and _rel(last, hT[0].numpy()) <= 1e-12


@pytest.mark.parametrize("sizes", [(33, 47, 40, 3), (96, 96, 96, 1), (7, 130, 5, 8)])
def test_td_mlp_restatement_equals_the_oracle_in_float64(sizes):
    from oracle.newt_oracle import OracleNEWT

    in_size, hidden, out_size, depth = sizes
    ws, bs, gs, ls = gv.random_mlp(*sizes, seed=sum(sizes), dtype=torch.float64)
    w = {}
    for i in range(depth):
        w[f"p.net.{3 * i}.weight"], w[f"p.net.{3 * i}.bias"] = ws[i][:, :, None], bs[i]
        if i < depth - 1:
            w[f"p.net.{3 * i + 1}.layer_norm.weight"], w[f"p.net.{3 * i + 1}.layer_norm.bias"] = gs[i], ls[i]
    o = OracleNEWT.__new__(OracleNEWT)          # td_mlp reads the state dict only
    o.w = w
    x = torch.randn(2, in_size, 37, dtype=torch.float64)
    with torch.no_grad():
        want = o.td_mlp(x, "p").numpy()
    got = td_mlp_float64(x.numpy(), [t.numpy() for t in ws], [t.numpy() for t in bs], [t.numpy() for t in gs], [t.numpy() for t in ls])
    assert got.shape == (2, out_size, 37) and _rel(got, want) <= 1e-12


@pytest.mark.parametrize("name", sorted(gv.CASES))
def test_every_case_selects_the_variant_it_is_named_for(name):
    c = gv.CASES[name]
    for mode in c["modes"]:
        gv.assert_plan(name, mode, gv.exciter_plan(gv.size_only_desc(c, mode == "fast"), c["B"], c["T"]))


def test_gru_plan_reports_the_recurrence_per_size():
    """(128, 44): W_ih (3 x 128 x 44 floats) does not fit the 64 KB the register kernel stages it in; (16, 70): more input
    channels than the register kernel has threads to stage a frame with (64)."""
    for (hidden, c_in), want in gv.GRU_PLANS.items():
        p = gv.gru_plan(hidden, c_in)
        assert (p["kernel"], p["kq"], p["threads"]) == want, (hidden, c_in, p)


@pytest.fixture(scope="module")
def defect_runs():
    """case -> (oracle, stages) of the FastNEWT oracle on the case's model and inputs"""
    runs = {}
    for name in set(gv.DEFECTS.values()):
        c = gv.CASES[name]
        with gv.configured(c) as nws:
            _, w = gv.build_model(nws, name)
        o, st = gv.make_oracle(w, c, True), {}
        o(*gv.inputs(name), stages=st)
        runs[name] = (o, st)
    return runs


def test_the_defect_model_without_a_defect_is_the_oracle(defect_runs):
    for name, (o, st) in defect_runs.items():
        y = gv.defective_output(o, st, None)
        assert np.array_equal(y, st["y"].numpy()), name            # silent reverb: the output IS the pre-reverb signal
        assert gv.passes(y, st["y"].numpy())


@pytest.mark.parametrize("defect", sorted(gv.DEFECTS))
def test_block_wise_bar_trips_on_a_defect(defect_runs, defect):
    """Factor by which each defect misses the bar (1e-5 x max(RMS(ref), 1e-3)), whole-signal | worst block of 512 samples:
        film_frame_early       (tpw4_hop25,   one 32-sample tile of one row of B = 64, N = 7700)    2.2e2x  |  6.9e3x
        shapers_32_up_dropped  (mt2_s48,      16 of 48 shapers, every sample)                       7.8e4x  |  8.0e4x
        channel_3_dropped      (oct4_oc4_mt2, one of four channels, every sample)                   7.8e3x  |  8.2e3x
        row_tail_zero          (mt2_s33,      16 samples of one row of B = 2, N = 368)              4.4e4x  |  6.2e4x
    None of these slips through either bar at these sizes.  The tile defect is the one the block-wise bar exists for: the
    whole-signal figure dilutes its 32 samples in 64 x 7700 (a factor 124, the block figure only 4), so a tile error of 4e-5 of
    the signal level already trips the block bar while the whole-signal bar starts at 1.2e-3."""
    name = gv.DEFECTS[defect]
    o, st = defect_runs[name]
    ref = st["y"].numpy()
    e, worst, scale = gv.errors(gv.defective_output(o, st, defect), ref)
    print(defect, name, f"whole {e / (gv.REL_BAR * scale):.3g}x  block {worst / (gv.REL_BAR * scale):.3g}x")
    assert worst >= 10 * gv.REL_BAR * scale, (defect, worst, scale)
    assert not gv.passes(gv.defective_output(o, st, defect), ref)
