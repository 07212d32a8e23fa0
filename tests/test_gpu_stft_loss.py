"""-m gpu: the multi-resolution STFT loss (csrc/stft_loss.hip through losses.py and the model's evaluation hooks) against the
float64 restatement of the definition (tests/stft_loss_restatement.py).

Bound: 1e-4 relative on the scalar and on every component (sc_r, log_r, lin_r) - the project's parity bar.  The kernel's
transform is an fp32 matrix product; each component is a sum over thousands of magnitudes taken in fp64, so the distance
is a few fp32 roundings.  Measured on the MI355X, largest relative distance over scalar and components:
    (1, 1100) 4.5e-7   (3, 4000) 3.8e-7   (2, 16000) 6.8e-8   all-zero target 6.4e-8   (256, 64, 256) 5.7e-8   model 1.5e-8
(every figure per component: DESIGN.md 3.12).

Shapes (the smallest at which each path exists): (1, 1100) is barely past the reflect limit of n_fft 2048 and has 5 frames at
hop 240; (3, 4000) has 81 frames at hop 50 - three frame tiles, the last with one frame - and a length no hop divides;
(2, 16000) eleven frame tiles at hop 50; (8, 16000), checked on its own, gives the finalise kernel 440 records of one
resolution, more than its 256 threads take in one pass.
The same file passes with NWS_BACKEND=ctypes (the ctypes binding instead of torch.ops)."""
import numpy as np
import pytest
import torch

import stft_loss_restatement as sr
from gpu_util import build_model, dev, record

pytestmark = pytest.mark.gpu

TOL = 1e-4


def _losses():
    import nws_amd as nws

    return nws


def _check(name, got_loss, got_comp, want_loss, want_comp):
    got_loss, got_comp = float(got_loss), np.asarray(got_comp.cpu(), dtype=np.float64)
    rel_loss = abs(got_loss - want_loss) / abs(want_loss)
    rel_comp = np.abs(got_comp - want_comp) / np.abs(want_comp)
    print(f"{name}: loss {got_loss:.9g} (f64 {want_loss:.9g}, rel {rel_loss:.2e}); components rel\n{rel_comp}")
    record("stft_loss/" + name, loss=got_loss, loss_f64=want_loss, rel_loss=rel_loss, rel_components_max=float(rel_comp.max()))
    assert got_comp.shape == want_comp.shape
    assert rel_loss <= TOL, (got_loss, want_loss)
    assert rel_comp.max() <= TOL, rel_comp


@pytest.mark.parametrize("B,N", sr.SHAPES)
def test_default_resolutions_against_the_restatement(B, N):
    x, y = sr.signals(B, N)
    m = _losses().MultiResolutionSTFTLoss()
    xd, yd = dev(x), dev(y)
    loss, comp = m(xd, yd), m.components(xd, yd)
    assert loss.is_cuda and loss.dim() == 0 and loss.dtype == torch.float32 and comp.shape == (3, 3)
    want_loss, want_comp = sr.reference(B, N)
    _check(f"default_{B}x{N}", loss, comp, want_loss, want_comp)
    # not symmetric: the spectral convergence is normalised by the target
    assert abs(float(m(yd, xd)) - float(loss)) > 1e-3 * float(loss)


def test_more_records_than_the_finalise_kernel_has_threads():
    B, N = 8, 16000           # (512, 50, 240): 11 frame tiles x 5 groups of M-tiles x 8 rows = 440 records
    x, y = sr.signals(B, N)
    m = _losses().MultiResolutionSTFTLoss()
    want_loss, want_comp = sr.reference(B, N)
    _check(f"default_{B}x{N}", m(dev(x), dev(y)), m.components(dev(x), dev(y)), want_loss, want_comp)


def test_all_zero_target_sits_on_the_clamp():
    x, _ = sr.signals(3, 4000)
    y = np.zeros_like(x)
    m = _losses().MultiResolutionSTFTLoss()
    _check("zero_target", m(dev(x), dev(y)), m.components(dev(x), dev(y)), sr.loss(x, y), sr.components(x, y))


def test_identical_signals_give_exactly_zero_and_calls_repeat_to_the_bit():
    x, y = sr.signals(3, 4000)
    m = _losses().MultiResolutionSTFTLoss()
    xd, yd = dev(x), dev(y)
    assert float(m(yd, yd)) == 0.0
    assert torch.equal(m.components(yd, yd), torch.zeros(3, 3, device="cuda"))
    a, b = m(xd, yd), m(xd, yd)
    assert torch.equal(a, b) and torch.equal(m.components(xd, yd), m.components(xd, yd))
    # (B, 1, N) is viewed as (B, N)
    c = m(xd.unsqueeze(1), yd.unsqueeze(1))
    assert c.dim() == 0 and torch.equal(a, c)
    assert torch.equal(m.components(xd.unsqueeze(1), yd.unsqueeze(1)), m.components(xd, yd))


def test_single_resolution_full_width_window_and_linear_term():
    x, y = sr.signals(3, 4000)
    res = ((256, 64, 256),)
    nws = _losses()
    m = nws.STFTLoss(256, 64, 256, w_lin_mag=1.0)
    xd, yd = dev(x), dev(y)
    comp = m.components(xd, yd)
    assert comp.shape == (1, 3)
    _check("single_256_lin", m(xd, yd), comp, sr.loss(x, y, res, w_lin_mag=1.0), sr.components(x, y, res))
    # the default resolutions with the linear term switched on
    m3 = nws.MultiResolutionSTFTLoss(w_lin_mag=1.0)
    want = sr.reference(3, 4000)[1]
    _check("default_lin", m3(xd, yd), m3.components(xd, yd), float(want.sum() / 3), want)


def test_refusals():
    nws = _losses()
    m = nws.MultiResolutionSTFTLoss()
    x = torch.zeros(1, 1024, device="cuda")
    with pytest.raises(RuntimeError, match="N > n_fft / 2"):          # n_fft 2048 cannot reflect-pad 1024 samples
        m(x, x)
    with pytest.raises(ValueError, match="power of two"):
        nws.STFTLoss(fft_size=1000, win_length=1000)
    x, y = (torch.from_numpy(np.array(a)) for a in sr.signals(1, 1100))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x, y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x.cuda(), y)
    with pytest.raises(RuntimeError, match="same shape"):
        m(x.cuda(), y.cuda()[:, :-1])
    with pytest.raises(RuntimeError, match="no backward pass"):
        m(x.cuda().requires_grad_(), y.cuda())
    with pytest.raises(RuntimeError, match="160 KB"):                 # two tiles of 31 * 700 + 2048 samples do not fit the LDS
        nws.STFTLoss(2048, 700, 2048)(torch.zeros(1, 4096, device="cuda"), torch.zeros(1, 4096, device="cuda"))
    with pytest.raises(TypeError):
        m(x.cuda().double(), y.cuda().double())


def test_model_test_step_is_the_loss_of_its_own_render():
    nws = _losses()
    model = build_model(fast=True)
    g = torch.Generator().manual_seed(5)
    B, T = 2, 16
    f0 = (180.0 + 400.0 * torch.rand(B, 1, T, generator=g)).cuda()
    control = torch.randn(B, 2, T, generator=g).cuda()
    audio = (0.1 * torch.randn(B, 128 * T, generator=g)).cuda()
    torch.cuda.manual_seed(77)
    phase_u = torch.rand_like(model.osc.rand_phase)                 # the two hidden draws of forward(), in its order
    noise = torch.rand(128 * T - 1, device="cuda")
    torch.cuda.manual_seed(77)
    batch = {"audio": audio.double(), "f0": f0.double(), "control": control.double()}       # _run_step casts with .float()
    loss = model.test_step(batch, 0)
    assert loss.dim() == 0 and loss.is_cuda and not loss.requires_grad
    with torch.no_grad():
        recon = model(f0, control, phase_u=phase_u, noise=noise)
        want = nws.MultiResolutionSTFTLoss()(recon, audio)
    assert torch.equal(loss, want)
    torch.cuda.manual_seed(77)
    assert torch.equal(model.validation_step(batch, 0), want)
    f64 = sr.loss(recon.cpu().numpy(), audio.cpu().numpy())
    rel = abs(float(loss) - f64) / f64
    print(f"model: test_step {float(loss):.9g}, f64 restatement of the same render {f64:.9g}, rel {rel:.2e}")
    record("stft_loss/model", loss=float(loss), loss_f64=f64, rel_loss=rel)
    assert rel <= TOL
    with pytest.raises(RuntimeError, match="one length"):
        model.test_step({"audio": audio[:, :-128], "f0": f0, "control": control}, 0)


def test_evaluate_dataset_script_scores_a_split(tmp_path):
    """scripts/evaluate_dataset.py in-process on a three-item split (one item without audio): per-batch losses, their
    batch-size-weighted mean, and the same figures again on a second run (the draws are seeded)."""
    import importlib.util
    import os
    import re

    from click.testing import CliRunner

    from conftest import ROOT

    g = np.random.default_rng(3)
    T = 16
    root = tmp_path / "data"
    for sub in ("control", "audio"):
        os.makedirs(root / "test" / sub)
    np.save(root / "data_mean.npy", np.array([[300.0], [0.5]]))
    np.save(root / "data_std.npy", np.array([[80.0], [0.2]]))
    for name in ("a", "b", "c", "d"):
        np.save(root / "test" / "control" / f"control_{name}.npy", g.standard_normal((2, T)).astype(np.float32))
        if name != "d":
            np.save(root / "test" / "audio" / f"audio_{name}.npy", (0.1 * g.standard_normal(128 * T)).astype(np.float32))
    ckpt = os.path.join(ROOT, "tests", "golden", "weights_vn.npz")
    spec = importlib.util.spec_from_file_location("evaluate_dataset", os.path.join(ROOT, "scripts", "evaluate_dataset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = ["--model-checkpoint", ckpt, "--dataset-root", str(root), "--batch-size", "2", "--use-fastnewt"]
    first = CliRunner().invoke(mod.main, args)
    assert first.exit_code == 0, first.output
    assert "1 of 4 items of 'test' have no target audio" in first.output
    batch = [(int(n), float(v)) for n, v in re.findall(r"batch \d+: (\d+) items of 16 frames, loss ([0-9.]+)", first.output)]
    assert [n for n, _ in batch] == [2, 1]
    mean = float(re.search(r"test/loss ([0-9.]+)", first.output).group(1))
    assert mean == pytest.approx((2 * batch[0][1] + batch[1][1]) / 3, abs=2e-6)
    assert "weighted by batch size" in first.output
    assert all(np.isfinite(v) and v > 0 for _, v in batch)
    second = CliRunner().invoke(mod.main, args)
    assert second.output == first.output
